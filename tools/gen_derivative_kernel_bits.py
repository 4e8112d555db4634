"""Write tests/golden/derivative_kernel_bits.npz: the outputs of the calls of tests/test_derivative_kernel_bits_gpu.py, as the built library gives them.

    python tools/gen_derivative_kernel_bits.py [--out tests/golden/derivative_kernel_bits.npz]

Run on an MI355X against the build whose results are to be pinned.  The test module holds the calls (its ``mlp_entries`` and ``taylor_entries``) and
regenerates the inputs from seeded numpy, so the file holds outputs only: per test one flat array and the names and shapes of its entries.  Every call is
run twice; an entry whose two runs differ is not recorded: the run stops and nothing is written."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'derivative_kernel_bits.npz'))
    args = parser.parse_args()
    import test_derivative_kernel_bits_gpu as t
    from test_emulator_front_bits_gpu import flatten
    calls = [('mlp%d' % H, lambda H=H, y=y: t.mlp_entries(H, y)) for H, y in t.MLP_CASES] + [('taylor', t.taylor_entries)]
    recorded, count = {}, 0
    for group, fn in calls:
        first, second = fn(), fn()
        for name, value in first.items():
            if not (np.array_equal(value, second[name]) and np.isfinite(value).all()):
                sys.exit('%s.%s: two runs differ (or the result is not finite); nothing written' % (group, name))
        recorded[group + '.entries'], recorded[group] = flatten(first)
        count += len(first)
    np.savez_compressed(args.out, **recorded)
    print('%d entries, %d bytes of arrays, written to %s (%d bytes)' % (count, sum(v.nbytes for v in recorded.values()), args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
