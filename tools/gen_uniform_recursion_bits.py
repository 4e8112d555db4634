"""Write tests/golden/uniform_recursion_bits.npz: the outputs of the calls of tests/test_uniform_recursion_bits_gpu.py, as the built library gives them.

    python tools/gen_uniform_recursion_bits.py [--out tests/golden/uniform_recursion_bits.npz]

Run on an MI355X against the build whose results are to be pinned.  The test module holds the calls (its ``groups``) and takes the inputs from the case
builders of tests/splice_truth.py, tests/spline_truth.py and tests/brieden_truth.py, so the file holds outputs only: per test SHA-256 digests (32 bytes)
of the output rows (of 64 rows each where an entry has more than 256) and the names and shapes of its entries.  Every call is run twice; an entry whose
two runs differ is not recorded: the run stops and nothing is written."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'uniform_recursion_bits.npz'))
    args = parser.parse_args()
    import test_uniform_recursion_bits_gpu as t
    calls = t.groups()
    recorded, count = {}, 0
    for group, fn in calls:
        first, second = fn(), fn()
        for name, value in first.items():
            if not np.array_equal(value.view('u1'), second[name].view('u1')):      # (bytes: a NaN row holds NaN on purpose)
                sys.exit('%s.%s: two runs differ; nothing written' % (group, name))
        recorded[group + '.entries'], recorded[group] = t.digests(first)
        count += len(recorded[group])
    np.savez_compressed(args.out, **recorded)
    print('%d digests in %d groups, written to %s (%d bytes)' % (count, len(calls), args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
