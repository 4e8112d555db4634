"""Contracted second derivatives of the emulators (``Emulator.vjp2``: the residual-curvature term of the Hessian of chi2) against the only route to the same
numbers before it: ``Emulator.hessian(device=True)`` -- ``jvp2`` on the ndim (ndim + 1) / 2 unit pairs, mirrored -- followed by ``torch.einsum`` with the
cotangent.

    python tools/bench_vjp2.py [--batch 10000] [--ndim 8] [--outputs 256] [--order 3] [--repeats 20] [--warmup 3] [--only mlp|taylor] [--once] [--out FILE]

B = 10^4 parameter points, ndim = 8, 256 output columns under one key.  MLP: hidden (32, 32, 32) and (64, 64, 64), silu, synthetic weights, without a
y operation and with arcsinh.  Taylor: 8 parameters at order 3 (165 terms), synthetic coefficients.  The cotangent is drawn from N(0, 1), (B, 256).
Timed with HIP events on the current stream, the two routes alternating in one run after the warm-up calls, median and spread of the repeats:

  vjp2            : ``emulator.vjp2(params, cotangents, device=True)``
  hessian, einsum : ``torch.einsum('bc,bijc->bij', cotangent, emulator.hessian(params, device=True)[key])``

Before timing, the two results are compared at the size that is timed: the largest distance relative to the largest entry of the (i, j) block over the
batch (reordered float64 sums: a few 1e-16 x the cancellation of the block).  Condition (exit status 1 if missed): the median of ``vjp2`` is below the median of
the other route in every configuration.  ``--once`` runs each route once after the warm-up and times nothing: the run to put under
``rocprofv3 --kernel-trace --stats`` for the per-kernel times.  Needs neither the reference nor the oracle."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KEY = 'y'


def wrapped(engine, names, M):
    """An ``Emulator`` around a ready engine: one varied output ``KEY`` of M entries"""
    from cosmoprimo_amd.emulators import Emulator
    emulator = Emulator(None, params={name: (0., 1.) for name in names}, device=engine.device)
    emulator.engine = engine
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = [KEY], [(M,)], {}
    return emulator


def compare(torch, lines, emulator, X, cot, repeats, warmup, once):
    """True if vjp2 is the faster route (or nothing was timed)"""
    params = {name: X[:, i] for i, name in enumerate(emulator.params)}
    B, ndim = X.shape
    routes = [('vjp2', lambda: emulator.vjp2(params, {KEY: cot}, device=True)),
              ('hessian, einsum', lambda: torch.einsum('bc,bijc->bij', cot, emulator.hessian(params, device=True)[KEY]))]
    new, old = (fn() for name, fn in routes)
    top = old.abs().amax(dim=0)
    lines.append('  largest distance of vjp2 from the contracted hessian: %.2e of the block\'s largest entry' % float(((new - old).abs().amax(dim=0) / top).max()))
    del new, old
    for _ in range(warmup):
        for name, fn in routes:
            fn()
    torch.cuda.synchronize()
    if once:
        for name, fn in routes:
            fn()
        torch.cuda.synchronize()
        return True
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
        lines.append('  %-16s median %8.3f ms  (min %8.3f, max %8.3f over %d)  %7.2f ns per (point, pair)'
                     % (name, np.median(t), t.min(), t.max(), len(t), 1e6 * np.median(t) / (B * ndim * (ndim + 1) // 2)))
    median = {name: np.median(t) for name, t in times.items()}
    lines.append('  hessian, einsum / vjp2 = %.2f' % (median['hessian, einsum'] / median['vjp2']))
    return median['vjp2'] < median['hessian, einsum']


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=10000)
    parser.add_argument('--ndim', type=int, default=8)
    parser.add_argument('--outputs', type=int, default=256)
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
    B, M, ndim = args.batch, args.outputs, args.ndim
    names = ['p%d' % i for i in range(ndim)]
    cot = torch.as_tensor(rng.normal(0., 1., (B, M)), device=dev)
    lines, faster = [], True
    if args.only != 'taylor':
        for nhidden, yoperation in itertools.product(((32, 32, 32), (64, 64, 64)), (None, 'arcsinh')):
            engine = MLPEmulatorEngine(nhidden=nhidden, yoperation=yoperation, device=dev)
            lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
            ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
            engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
            engine.yoperations = ([{'name': yoperation}] if yoperation else []) + [{'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
            engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
            X = torch.as_tensor(rng.uniform(lo, hi, (B, ndim)), device=dev)
            lines.append('MLP emulator: B = %d points, ndim = %d, hidden %s, %d columns, silu, y operation %s, float64' % (B, ndim, nhidden, M, yoperation or 'none'))
            faster = compare(torch, lines, wrapped(engine, names, M), X, cot, args.repeats, args.warmup, args.once) and faster
    if args.only != 'mlp':
        powers = np.array([p for total in range(args.order + 1) for p in itertools.product(range(args.order + 1), repeat=ndim) if sum(p) == total], dtype='i4')
        taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
        X = torch.as_tensor(rng.uniform(0.4, 0.6, (B, ndim)), device=dev)
        lines.append('Taylor emulator: B = %d points, ndim = %d, order %d (%d terms), %d columns, float64' % (B, ndim, args.order, len(powers), M))
        faster = compare(torch, lines, wrapped(taylor, names, M), X, cot, args.repeats, args.warmup, args.once) and faster
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')
    if not faster:
        sys.exit('vjp2 is not the faster route somewhere')


if __name__ == '__main__':
    main()
