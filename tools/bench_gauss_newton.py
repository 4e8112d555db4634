"""Batched Fisher matrices and Gauss-Newton normal equations of the emulators (``gauss_newton``) against the only route there was before them: the full
Jacobian and the value on the device, then their contraction with ``torch.einsum``.

    python tools/bench_gauss_newton.py [--batch 10000 64 1] [--ndim 8] [--nhidden 64 64 64] [--outputs 1024] [--order 3] [--repeats 20] [--warmup 3]
                                       [--only mlp|taylor] [--once] [--out FILE]

MLP: ndim = 8, hidden (64, 64, 64), silu, M = 1024 outputs, synthetic weights, y operation log10.  Taylor: 8 parameters at order 3 (165 terms), M = 1024,
synthetic coefficients.  Per batch size, timed with HIP events on the current stream, the routes alternating in one run after warm-up calls, median and
spread of the repeats:

  gauss_newton      : ``engine.gauss_newton(X, weights, data=data)``: (fisher, grad, chi2), no (B, ndim, M) array
  jacobian + einsum : ``value, J = engine.jacobian(X, return_value=True)``, then ``wJ = w[:, None, :] * J``, ``einsum('bic,bjc->bij', wJ, J)``,
                      ``einsum('bic,bc->bi', wJ, data - value)`` and ``(w * (data - value)**2).sum(1)``: what a user of ``jacobian`` writes
  fisher only       : ``engine.gauss_newton(X, weights)`` against ``jacobian`` and the first einsum

Weights and data are per point, (B, M).  No ratio is required: the script reports.  ``--once`` runs each route once after the warm-up and times nothing:
the run to put under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times.  Needs neither the reference nor the oracle."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def composed(torch, engine, X, w, data):
    value, J = engine.jacobian(X, return_value=True)
    wJ = w[:, None, :] * J
    resid = data - value
    return torch.einsum('bic,bjc->bij', wJ, J), torch.einsum('bic,bc->bi', wJ, resid), (w * resid * resid).sum(dim=1)


def composed_fisher(torch, engine, X, w):
    J = engine.jacobian(X)
    return torch.einsum('bic,bjc->bij', w[:, None, :] * J, J)


def compare(torch, lines, engine, X, M, repeats, warmup, once, rng):
    B, ndim = (int(n) for n in X.shape)
    w = torch.as_tensor(10.**rng.uniform(-2., 1., (B, M)), device=X.device)
    data = engine.predict(X) * torch.as_tensor(1. + 0.05 * rng.standard_normal((B, M)), device=X.device)
    routes = [('gauss_newton', lambda: engine.gauss_newton(X, w, data=data)), ('jacobian + einsum', lambda: composed(torch, engine, X, w, data)),
              ('fisher only', lambda: engine.gauss_newton(X, w)), ('jacobian + einsum (F)', lambda: composed_fisher(torch, engine, X, w))]
    ours, theirs = routes[0][1](), routes[1][1]()
    distance = [float(((a - b).abs().reshape(B, -1).max(dim=0).values / b.abs().reshape(B, -1).max(dim=0).values).max()) for a, b in zip(ours, theirs)]
    lines.append('B = %d: largest distance of the two routes, per block over the batch: fisher %.2e, grad %.2e, chi2 %.2e of the block\'s largest entry' % ((B,) + tuple(distance)))
    del ours, theirs
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
        lines.append('  %-22s median %8.3f ms  (min %8.3f, max %8.3f over %d)' % (name, np.median(t), t.min(), t.max(), len(t)))
    median = {name: np.median(t) for name, t in times.items()}
    lines.append('  jacobian + einsum / gauss_newton = %.2f, fisher only: %.2f; the Jacobian the call avoids: %.1f MB'
                 % (median['jacobian + einsum'] / median['gauss_newton'], median['jacobian + einsum (F)'] / median['fisher only'], 8e-6 * B * ndim * M))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, nargs='+', default=[10000, 64, 1])
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
    M, ndim, nhidden = args.outputs, args.ndim, tuple(args.nhidden)
    lines = []
    if args.only != 'taylor':
        engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
        lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
        ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
        engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
        engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
        engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
        lines.append('MLP emulator: ndim = %d, hidden %s, M = %d outputs, silu, y operation log10, float64' % (ndim, nhidden, M))
        for B in args.batch:
            compare(torch, lines, engine, torch.as_tensor(rng.uniform(lo, hi, (B, ndim)), device=dev), M, args.repeats, args.warmup, args.once, rng)
    if args.only != 'mlp':
        powers = np.array([p for total in range(args.order + 1) for p in itertools.product(range(args.order + 1), repeat=ndim) if sum(p) == total], dtype='i4')
        taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
        lines.append('Taylor emulator: ndim = %d, order %d (%d terms), M = %d outputs, float64' % (ndim, args.order, len(powers), M))
        for B in args.batch:
            compare(torch, lines, taylor, torch.as_tensor(rng.uniform(0.4, 0.6, (B, ndim)), device=dev), M, args.repeats, args.warmup, args.once, rng)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
