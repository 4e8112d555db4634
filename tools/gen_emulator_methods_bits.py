"""Write tests/golden/emulator_methods_bits.npz: the outputs of the calls of tests/test_emulator_methods_bits_gpu.py, as the built library and the front give them.

    python tools/gen_emulator_methods_bits.py [--out tests/golden/emulator_methods_bits.npz]

Run on an MI355X against the commit whose results are to be pinned.  The test module holds the calls (its ``method_entries``) and regenerates the inputs from
seeded numpy, so the file holds outputs only: per test one flat array and the names and shapes of its entries.  Every call is run twice; an entry whose two
runs differ or that holds a value that is not finite is not recorded: the run stops and nothing is written."""
import argparse
import os
import sys

import numpy as np

from gen_emulator_front_bits import ROOT, toy_emulators      # (which puts the repository and tests/ on the path)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'emulator_methods_bits.npz'))
    args = parser.parse_args()
    import test_emulator_methods_bits_gpu as t
    emulators = toy_emulators()
    recorded, count = {}, 0
    for which in ('taylor', 'mlp'):
        group = 'methods_%s' % which
        first, second = t.method_entries(emulators[which]), t.method_entries(emulators[which])
        for name, value in first.items():
            if not (np.array_equal(value, second[name]) and np.isfinite(value).all()):
                sys.exit('%s.%s: two runs differ (or the result is not finite); nothing written' % (group, name))
        recorded[group + '.entries'], recorded[group] = t.flatten(first)
        count += len(first)
    np.savez_compressed(args.out, **recorded)
    print('%d entries, %d bytes of arrays, written to %s (%d bytes)' % (count, sum(v.nbytes for v in recorded.values()), args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
