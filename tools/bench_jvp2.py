"""Batched second directional derivatives of the emulators (``jvp2``), with v = u and with a second tangent set, beside two ``jvp`` calls -- the cost of
the central difference of ``jvp`` that was the only route to second order before (context, not a target: that route loses five or more digits).

    python tools/bench_jvp2.py [--batch 10000] [--ndim 8] [--directions 8] [--nhidden 32 32 32] [--outputs 256] [--order 3] [--repeats 20] [--warmup 3]
                               [--yoperation log10|none] [--only mlp|taylor] [--once] [--out FILE]

MLP: B = 10^4 parameter points, ndim = 8, K = 8 pairs of directions per point, silu, M = 256 outputs, synthetic weights, with the y operation log10 (the
entry point then runs the jvp kernel once per tangent set for the chain rule) and without.  Taylor: 8 parameters at order 3 (165 terms), M = 256,
synthetic coefficients.  Timed with HIP events on the current stream, the routes alternating in one run after warm-up calls, median and spread of the
repeats, and the time per row (B K rows):

  jvp2 (v = u)  : ``engine.jvp2(X, u)``
  jvp2 (mixed)  : ``engine.jvp2(X, u, v)``
  jvp           : ``engine.jvp(X, u)``, one call
  2 x jvp       : ``engine.jvp(X + h v, u)`` and ``engine.jvp(X - h v, u)``, the two calls of a central difference (the subtraction is not timed)

Also printed: the distance of jvp2 from that central difference at h = 1e-4 of the scales, relative to the block's largest entry (context: it shows the
digits the difference route loses).  ``--once`` runs each route once after the warm-up and times nothing: the run to put under
``rocprofv3 --kernel-trace --stats`` for the per-kernel times.  Needs neither the reference nor the oracle."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compare(torch, lines, engine, X, u, v, h, repeats, warmup, once):
    B, K = int(u.shape[0]), int(u.shape[1])
    Xp, Xm = (X[:, None, :] + sign * h * v for sign in (1., -1.))      # (B, K, ndim): a point per pair
    flat = lambda a: a.reshape(B * K, -1)      # noqa: E731
    routes = [('jvp2 (v = u)', lambda: engine.jvp2(X, u)), ('jvp2 (mixed)', lambda: engine.jvp2(X, u, v)), ('jvp', lambda: engine.jvp(X, u)),
              ('2 x jvp', lambda: (engine.jvp(flat(Xp), flat(u)), engine.jvp(flat(Xm), flat(u))))]
    mixed = engine.jvp2(X, u, v)
    plus, minus = routes[3][1]()
    difference = ((plus - minus) / (2. * h)).reshape(mixed.shape)
    top = mixed.abs().amax(dim=0)
    lines.append('K = %d: largest distance of jvp2 (mixed) from the central difference of jvp at h = %.0e: %.2e of the block\'s largest entry'
                 % (K, h, float(((mixed - difference).abs().amax(dim=0) / top).max())))
    del mixed, plus, minus, difference
    for _ in range(warmup):
        for name, fn in routes:
            fn()
    torch.cuda.synchronize()
    if once:
        for name, fn in routes:
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
        lines.append('  %-14s median %8.3f ms  (min %8.3f, max %8.3f over %d)  %7.2f ns per row' % (name, np.median(t), t.min(), t.max(), len(t), 1e6 * np.median(t) / (B * K)))
    median = {name: np.median(t) for name, t in times.items()}
    lines.append('  jvp2 (v = u) / jvp = %.2f, jvp2 (mixed) / jvp = %.2f, jvp2 (mixed) / 2 x jvp = %.2f'
                 % (median['jvp2 (v = u)'] / median['jvp'], median['jvp2 (mixed)'] / median['jvp'], median['jvp2 (mixed)'] / median['2 x jvp']))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=10000)
    parser.add_argument('--ndim', type=int, default=8)
    parser.add_argument('--directions', type=int, default=8)
    parser.add_argument('--nhidden', type=int, nargs='+', default=[32, 32, 32])
    parser.add_argument('--outputs', type=int, default=256)
    parser.add_argument('--order', type=int, default=3)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--yoperation', choices=['log10', 'none'], default='log10')
    parser.add_argument('--only', choices=['mlp', 'taylor'], default=None)
    parser.add_argument('--once', action='store_true')
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine, TaylorEmulatorEngine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    B, M, ndim, K, nhidden = args.batch, args.outputs, args.ndim, args.directions, tuple(args.nhidden)
    lines = []
    if args.only != 'taylor':
        log10 = args.yoperation == 'log10'
        engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10' if log10 else None, device=dev)
        lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
        ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
        engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
        engine.yoperations = ([{'name': 'log10'}] if log10 else []) + [{'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
        engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
        X = torch.as_tensor(rng.uniform(lo, hi, (B, ndim)), device=dev)
        lines.append('MLP emulator: B = %d points, ndim = %d, K = %d, hidden %s, M = %d outputs, silu, y operation %s, float64' % (B, ndim, K, nhidden, M, args.yoperation))
        u, v = (torch.as_tensor((hi - lo) * rng.normal(0., 1., (B, K, ndim)), device=dev) for _ in range(2))
        compare(torch, lines, engine, X, u, v, 1e-4, args.repeats, args.warmup, args.once)
    if args.only != 'mlp':
        powers = np.array([p for total in range(args.order + 1) for p in itertools.product(range(args.order + 1), repeat=ndim) if sum(p) == total], dtype='i4')
        taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
        Xt = torch.as_tensor(rng.uniform(0.4, 0.6, (B, ndim)), device=dev)
        lines.append('Taylor emulator: B = %d points, ndim = %d, K = %d, order %d (%d terms), M = %d outputs, float64' % (B, ndim, K, args.order, len(powers), M))
        u, v = (torch.as_tensor(rng.normal(0., 1., (B, K, ndim)), device=dev) for _ in range(2))
        compare(torch, lines, taylor, Xt, u, v, 1e-4, args.repeats, args.warmup, args.once)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
