"""Batched parameter derivatives of the emulators (``jacobian``) against what a user had before them: central differences of ``predict``.

    python tools/bench_jacobian.py [--batch 10000] [--ndim 6] [--nhidden 32 32 32] [--outputs 2560] [--repeats 20] [--warmup 3] [--out profiles/jacobian.txt]

MLP: B = 10^4 parameter points, ndim = 6, hidden (32, 32, 32), M = 2560 outputs, synthetic weights, y operation log10 (``--nhidden 64 64 64``: the
widest layers, 72 KB of LDS in the tangent kernel).  Taylor: the shape of the README's example, 2 parameters at order 3 (10 terms) and
M = 422 x 30 outputs, synthetic coefficients.  Timed with HIP events on the current stream after warm-up calls, median and spread of the repeats:

  jacobian          : ``engine.jacobian(X, return_value=True)`` (MLP: forward kernel + tangent kernel; Taylor: predict + the derivative front end)
  2 ndim predicts   : the alternative before this call, central differences: ``engine.predict`` at x +- h e_i (the subtraction and division not counted)
  ndim + 1 predicts : the store-bound expectation -- the Jacobian and the value are ndim + 1 times the bytes of one prediction

and the achieved store bandwidth 8 B (ndim + 1) M / t against 8 TB/s (HBM3E of one MI355X).  Needs neither the reference nor the oracle."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

HBM = 8e12


def compare(torch, lines, engine, X, repeats, warmup):
    from bench_mlp import time_call
    B, ndim = (int(n) for n in X.shape)
    value, J = engine.jacobian(X, return_value=True)
    M = int(value.shape[1])
    h = 1e-4 * X.abs().mean(dim=0)
    shifted = [X + sign * h[i] * torch.nn.functional.one_hot(torch.tensor(i), ndim).to(X) for i in range(ndim) for sign in (1., -1.)]
    fd = torch.stack([(engine.predict(shifted[2 * i]) - engine.predict(shifted[2 * i + 1])) / (shifted[2 * i][:, i] - shifted[2 * i + 1][:, i])[:, None] for i in range(ndim)], dim=1)
    top = J.abs().amax(dim=0)
    lines.append('largest distance of the Jacobian from central differences with h = 1e-4 x: %.2e of a (parameter, column) block' % float(((J - fd).abs().amax(dim=0) / top).max()))
    del fd
    nbytes = 8. * B * (ndim + 1) * M
    results = {}
    for name, fn in [('jacobian (value and derivatives)', lambda: engine.jacobian(X, return_value=True)),
                     ('%d predicts (central differences)' % (2 * ndim), lambda: [engine.predict(x) for x in shifted]),
                     ('%d predicts (ndim + 1)' % (ndim + 1), lambda: [engine.predict(x) for x in shifted[:ndim + 1]])]:
        t = time_call(torch, fn, repeats, warmup)
        results[name] = np.median(t)
        lines.append('%-36s median %8.3f ms  (min %8.3f, max %8.3f over %d)' % (name, np.median(t), t.min(), t.max(), len(t)))
    jac, central, expected = results.values()
    lines.append('jacobian / central differences = %.3f, jacobian / (ndim + 1) predicts = %.3f; stores 8 B (ndim + 1) M = %.1f MB at %.2f TB/s (%.0f %% of %.0f TB/s)'
                 % (jac / central, jac / expected, nbytes / 1e6, nbytes / jac / 1e9, 100. * nbytes / jac * 1e3 / HBM, HBM / 1e12))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=10000)
    parser.add_argument('--ndim', type=int, default=6)
    parser.add_argument('--nhidden', type=int, nargs='+', default=[32, 32, 32])
    parser.add_argument('--outputs', type=int, default=2560)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine, TaylorEmulatorEngine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    B, M, ndim, nhidden = args.batch, args.outputs, args.ndim, tuple(args.nhidden)
    engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
    lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
    ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
    engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
    engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
    engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
    X = torch.as_tensor(rng.uniform(lo, hi, (B, ndim)), device=dev)
    lines = ['MLP emulator: B = %d points, ndim = %d, hidden %s, M = %d outputs, silu, y operation log10, float64' % (B, ndim, nhidden, M)]
    compare(torch, lines, engine, X, args.repeats, args.warmup)
    tdim, order, TM = 2, 3, 422 * 30
    powers = np.array([p for total in range(order + 1) for p in itertools.product(range(order + 1), repeat=tdim) if sum(p) == total], dtype='i4')
    taylor = TaylorEmulatorEngine.from_state({'center': np.array([0.3, 0.7]), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), TM))}, device=dev)
    Xt = torch.as_tensor(np.column_stack([rng.uniform(0.28, 0.32, B), rng.uniform(0.65, 0.75, B)]), device=dev)
    lines.append('Taylor emulator: B = %d points, ndim = %d, order %d (%d terms), M = %d outputs, float64' % (B, tdim, order, len(powers), TM))
    compare(torch, lines, taylor, Xt, args.repeats, args.warmup)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
