"""Print the seeds of tests/jvp2_reference.py (MLP_SEEDS, TAYLOR_SEEDS): per case the first seed, from 0, at which the rounding level of the float64
restatement of the second directional derivative is at most 32 floors with v = u AND with the second tangent set.

    python tools/search_jvp2_seeds.py [--most 64] [--jobs 8]

Runs on the CPU.  The cap is that of tests/test_jvp2_host.py, which is the judge; a case that needs no redraw is not printed."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import jacobian_reference as jr  # noqa: E402
import jvp2_reference as sr  # noqa: E402


def worst(kind, case, seed):
    """the larger of the two levels, in floors"""
    config, truth = (sr.mlp_config, sr.mlp_truth) if kind == 'mlp' else (sr.taylor_config, sr.taylor_truth)
    cfg = config(**dict(case, seed=seed))
    return max(float(jr.levels(*truth(cfg, mixed))[1].max()) / jr.FLOOR for mixed in (False, True))


def first_seed(job):
    kind, case, most = job
    tried = []
    for seed in range(most):
        tried.append(worst(kind, case, seed))
        if tried[-1] <= 32.:
            return kind, case, seed, tried
    return kind, case, None, tried


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--most', type=int, default=64)
    parser.add_argument('--jobs', type=int, default=8)
    args = parser.parse_args()
    strip = lambda case: {name: value for name, value in case.items() if name != 'seed'}  # noqa: E731
    jobs = [('mlp', strip(case), args.most) for case in sr.MLP_CASES + sr.MLP_RANGE_CASES] + [('taylor', strip(case), args.most) for case in sr.TAYLOR_CASES]
    with multiprocessing.Pool(args.jobs) as pool:
        for kind, case, seed, tried in pool.imap(first_seed, jobs):
            print('%-6s %-60s seed %s   levels tried: %s' % (kind, sr.case_id(case), seed, ' '.join('%.1f' % level for level in tried)), flush=True)


if __name__ == '__main__':
    main()
