"""Write tests/golden/row_transform_bits.npz: the outputs of the calls of tests/test_row_transform_bits_gpu.py, as the built library gives them.

    python tools/gen_row_transform_bits.py [--out tests/golden/row_transform_bits.npz]

Run on an MI355X against the build whose results are to be pinned.  The test module holds the calls (its ``*_entries``) and regenerates the inputs from
seeded numpy, so the file holds outputs only: per test one SHA-256 digest (32 bytes) per output row and the names and shapes of its entries.  Every call
is run twice; an entry whose two runs differ is not recorded: the run stops and nothing is written."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'row_transform_bits.npz'))
    args = parser.parse_args()
    import test_row_transform_bits_gpu as t
    f = t.wallish_filter()
    calls = [('dst%d' % n, lambda n=n: t.dst_entries(n)) for n in t.DST_SIZES] + [('rfft', t.rfft_entries)]
    calls += [('analytic.' + engine, lambda engine=engine: t.analytic_entries(engine, f)) for engine in t.ENGINES]
    calls += [('sigma.' + engine, lambda engine=engine: t.sigma_entries(engine)) for engine in t.ENGINES]
    calls += [('spline', t.spline_entries), ('geospline', t.geospline_entries)]
    recorded, count = {}, 0
    for group, fn in calls:
        first, second = fn(), fn()
        for name, value in first.items():
            if not np.array_equal(value.view('u1'), second[name].view('u1')):      # (bytes: rows screened out hold NaN on purpose)
                sys.exit('%s.%s: two runs differ; nothing written' % (group, name))
        recorded[group + '.entries'], recorded[group] = t.digests(first)
        count += len(recorded[group])
    np.savez_compressed(args.out, **recorded)
    print('%d rows in %d groups, written to %s (%d bytes)' % (count, len(calls), args.out, os.path.getsize(args.out)))


if __name__ == '__main__':
    main()
