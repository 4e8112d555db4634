"""Write tests/golden/analytic_front_bits.npz: the inputs and outputs of the calls of tests/test_analytic_front_bits_gpu.py, as the built library gives them.

    python tools/gen_analytic_front_bits.py [--out tests/golden/analytic_front_bits.npz]

Run on an MI355X against the build whose results are to be pinned.  The test module holds the calls (``engine_entries``, ``common_entries``,
``large_entries``) and draws the inputs (``draw_inputs``: fixed seed), which are stored as ``in.*``; per group one flat array of outputs and the names
and shapes of its entries.  Every group is run twice; if an entry's two runs differ, or an entry is not finite, nothing is written."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'analytic_front_bits.npz'))
    args = parser.parse_args()
    import test_analytic_front_bits_gpu as t
    recorded = t.draw_inputs()
    f = t.wallish_filter()
    calls = [(engine, lambda engine=engine: t.engine_entries(recorded, engine, f)) for engine in t.ENGINES]
    calls += [('common', lambda: t.common_entries(recorded)), ('large', lambda: t.large_entries(recorded, f))]
    count = 0
    for group, fn in calls:
        first, second = fn(), fn()
        for name, value in first.items():
            if not (np.array_equal(value, second[name]) and np.isfinite(value).all()):
                sys.exit('%s.%s: two runs differ (or the result is not finite); nothing written' % (group, name))
        recorded[group + '.entries'], recorded[group] = t.flatten(first)
        count += len(first)
    np.savez_compressed(args.out, **recorded)
    print('%d entries, %d bytes of arrays, written to %s (%d bytes)' % (count, sum(v.nbytes for v in recorded.values()), args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
