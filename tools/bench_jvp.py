"""Batched Jacobian-vector products of the emulators (``jvp``) against the only route there was before them: the full Jacobian on the device, then its
contraction with the tangents.

    python tools/bench_jvp.py [--batch 10000] [--ndim 8] [--nhidden 64 64 64] [--outputs 1024] [--order 3] [--repeats 20] [--warmup 3] [--only mlp|taylor]
                              [--once] [--out FILE]

MLP: B = 10^4 parameter points, ndim = 8, hidden (64, 64, 64), silu, M = 1024 outputs, synthetic weights, y operation log10.  Taylor: 8 parameters at
order 3 (165 terms), M = 1024, synthetic coefficients.  For K = 1 and K = ndim directions per point, timed with HIP events on the current stream, both
routes alternating in one run after warm-up calls, median and spread of the repeats:

  jvp               : ``engine.jvp(X, tan)``: B K rows of the tangent kernel (MLP) or of the GEMM (Taylor), (B, K, M) stored
  jacobian + einsum : ``torch.einsum('bki,bic->bkc', tan, engine.jacobian(X))``: B ndim rows and a (B, ndim, M) array written and read back
  jacobian          : ``engine.jacobian(X)`` alone, the yardstick of K = ndim (the jvp with identity tangents computes the same rows)

At K = 1 the jvp is ndim times fewer rows and bytes; at K = ndim parity with ``jacobian`` is the expectation.  No ratio is required: the script reports.
``--once`` runs each route once after the warm-up and times nothing: the run to put under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.
Needs neither the reference nor the oracle."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(torch, lines, engine, X, tan, M, repeats, warmup, once):
    K = int(tan.shape[1])
    routes = [('jvp', lambda: engine.jvp(X, tan)), ('jacobian + einsum', lambda: torch.einsum('bki,bic->bkc', tan, engine.jacobian(X))),
              ('jacobian', lambda: engine.jacobian(X))]
    out, out_route = (fn() for name, fn in routes[:2])
    scale = torch.einsum('bki,bic->bkc', tan.abs(), engine.jacobian(X).abs())
    lines.append('K = %d: largest distance of the two routes: %.2e of sum_i |tan| |J|' % (K, float(((out - out_route).abs() / scale).max())))
    del scale, out, out_route
    for _ in range(warmup):
        for name, fn in routes:
            fn()
    torch.cuda.synchronize()
    if once:
        for name, fn in routes[:2]:
            fn()
        torch.cuda.synchronize()
        return
    times = {name: [] for name, fn in routes}
    for _ in range(repeats):
        for name, fn in routes:      # alternating
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop))
    for name, t in times.items():
        t = np.array(t)
        lines.append('  %-20s median %8.3f ms  (min %8.3f, max %8.3f over %d)' % (name, np.median(t), t.min(), t.max(), len(t)))
    median = {name: np.median(t) for name, t in times.items()}
    B, ndim = (int(n) for n in X.shape)
    lines.append('  jacobian + einsum / jvp = %.2f, jacobian / jvp = %.2f (rows: B ndim / B K = %.1f); the Jacobian the jvp avoids: %.0f MB'
                 % (median['jacobian + einsum'] / median['jvp'], median['jacobian'] / median['jvp'], ndim / float(K), 8e-6 * B * ndim * M))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=10000)
    parser.add_argument('--ndim', type=int, default=8)
    parser.add_argument('--nhidden', type=int, nargs='+', default=[64, 64, 64])
    parser.add_argument('--outputs', type=int, default=1024)
    parser.add_argument('--order', type=int, default=3)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--only', choices=['mlp', 'taylor'], default=None)
    parser.add_argument('--once', action='store_true')
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine, TaylorEmulatorEngine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    B, M, ndim, nhidden = args.batch, args.outputs, args.ndim, tuple(args.nhidden)
    lines = []
    if args.only != 'taylor':
        engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
        lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
        ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
        engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
        engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
        engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
        X = torch.as_tensor(rng.uniform(lo, hi, (B, ndim)), device=dev)
        lines.append('MLP emulator: B = %d points, ndim = %d, hidden %s, M = %d outputs, silu, y operation log10, float64' % (B, ndim, nhidden, M))
        for K in (1, ndim):
            compare(torch, lines, engine, X, torch.as_tensor((hi - lo) * rng.normal(0., 1., (B, K, ndim)), device=dev), M, args.repeats, args.warmup, args.once)
    if args.only != 'mlp':
        powers = np.array([p for total in range(args.order + 1) for p in itertools.product(range(args.order + 1), repeat=ndim) if sum(p) == total], dtype='i4')
        taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
        Xt = torch.as_tensor(rng.uniform(0.4, 0.6, (B, ndim)), device=dev)
        lines.append('Taylor emulator: B = %d points, ndim = %d, order %d (%d terms), M = %d outputs, float64' % (B, ndim, args.order, len(powers), M))
        for K in (1, ndim):
            compare(torch, lines, taylor, Xt, torch.as_tensor(rng.normal(0., 1., (B, K, ndim)), device=dev), M, args.repeats, args.warmup, args.once)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
