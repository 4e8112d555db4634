"""Print the seeds of tests/vjp2_reference.py (MLP_SEEDS, TAYLOR_SEEDS): per case the first seed, from 0, at which the rounding level of the float64
restatement of the contracted second derivative is at most 32 floors.

    python tools/search_vjp2_seeds.py [--most 64] [--jobs 8]

Runs on the CPU.  The cap is that of tests/test_vjp2_host.py, which is the judge; a case that needs no redraw is not printed as a table entry."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import vjp2_reference as cr  # noqa: E402


def first_seed(job):
    kind, case, most = job
    tried = []
    for seed in range(most):
        tried.append(cr.level((cr.mlp_case if kind == 'mlp' else cr.taylor_case)(**dict(case, seed=seed))[1]))
        if tried[-1] <= cr.CAP:
            return kind, case, seed, tried
    return kind, case, None, tried


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--most', type=int, default=64)
    parser.add_argument('--jobs', type=int, default=8)
    args = parser.parse_args()
    strip = lambda case: {name: value for name, value in case.items() if name != 'seed'}  # noqa: E731
    jobs = [('mlp', strip(case), args.most) for case in cr.mlp_cases()] + [('taylor', strip(case), args.most) for case in cr.taylor_cases()]
    tables = {'mlp': {}, 'taylor': {}}
    with multiprocessing.Pool(args.jobs) as pool:
        for kind, case, seed, tried in pool.imap(first_seed, jobs):
            print('%-6s %-60s seed %s   levels tried: %s' % (kind, cr.case_id(case), seed, ' '.join('%.1f' % level for level in tried)), flush=True)
            if seed:
                tables[kind][cr.case_id(case)] = seed
    print('MLP_SEEDS = %r' % tables['mlp'])
    print('TAYLOR_SEEDS = %r' % tables['taylor'])


if __name__ == '__main__':
    main()
