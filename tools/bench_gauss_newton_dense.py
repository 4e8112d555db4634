"""``Emulator.gauss_newton(..., precision=)`` -- Fisher matrices and normal equations under a dense precision matrix (``cp_gauss_newton_dense``) -- against the
diagonal call at the same shape and against what a user could write for a dense P before it: ``Emulator.jacobian(device=True)`` and ``torch.einsum``.

    python tools/bench_gauss_newton_dense.py [--batch 10000] [--ndim 8] [--nhidden 64 64 64] [--outputs 256] [--repeats 20] [--warmup 3] [--out FILE]

An MLP emulator with synthetic weights (ndim = 8, hidden (64, 64, 64), silu, y operation log10) whose one output key 'y' holds N = 256 values;
P[c, d] = 0.6^|c - d| sqrt(w_c w_d), w = 10^U(-2, 1); data = prediction x (1 + 0.05 xi).  Timed with HIP events on the current stream, the routes alternating
in one run after warm-up calls, median and spread of the repeats:

  gauss_newton(precision=P)   : the new call, device=True: the engine's jacobian into the (B, ndim, N) buffer, cp_gauss_newton_dense
  the contraction alone       : ``gauss_newton_dense(J, value, P, data)`` on a Jacobian that is there already
  gauss_newton (diagonal)     : the diagonal call with weights diag(P), one row shared by all points, device=True: no Jacobian in memory
  jacobian + einsum           : ``values, J = emulator.jacobian(params, device=True, return_value=True)``, ``JP = einsum('bic,cd->bid', J, P)``,
                                ``einsum('bid,bjd->bij', JP, J)``, ``einsum('bid,bd->bi', JP, r)``, ``einsum('bc,cd,bd->b', r, P, r)``
  einsum alone                : those four on a Jacobian that is there already

No ratio is required: the script reports.  Needs neither the reference nor the oracle."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def contracted(torch, J, value, P, data):
    JP, resid = torch.einsum('bic,cd->bid', J, P), data - value
    return torch.einsum('bid,bjd->bij', JP, J), torch.einsum('bid,bd->bi', JP, resid), torch.einsum('bc,cd,bd->b', resid, P, resid)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, nargs='+', default=[10000])
    parser.add_argument('--ndim', type=int, default=8)
    parser.add_argument('--nhidden', type=int, nargs='+', default=[64, 64, 64])
    parser.add_argument('--outputs', type=int, default=256)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.emulators import Emulator, MLPEmulatorEngine
    from cosmoprimo_amd.emulators.tools import gauss_newton_dense
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    N, ndim, nhidden = args.outputs, args.ndim, tuple(args.nhidden)
    engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
    lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
    ylo, yhi = rng.uniform(-2., 0., N), rng.uniform(1., 3., N)
    engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
    engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
    engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, N, seed=1), ndim, N
    names = ['p%d' % i for i in range(ndim)]
    emulator = Emulator(None, params={name: (lo[i], hi[i]) for i, name in enumerate(names)}, engine=engine)
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['y'], [(N,)], {}
    w = 10.**rng.uniform(-2., 1., N)
    c = np.arange(N)
    P = torch.as_tensor(0.6**np.abs(c[:, None] - c[None, :]) * np.sqrt(w[:, None] * w[None, :]), device=dev)
    wrow = torch.as_tensor(w, device=dev)
    lines = ['MLP emulator: ndim = %d, hidden %s, N = %d outputs under one key, silu, y operation log10, float64; P dense (N, N), shared by all points' % (ndim, nhidden, N)]
    for B in args.batch:
        X = rng.uniform(lo, hi, (B, ndim))
        params = {name: torch.as_tensor(X[:, i], device=dev) for i, name in enumerate(names)}
        data = {'y': emulator.predict(params, device=True)['y'] * torch.as_tensor(1. + 0.05 * rng.standard_normal((B, N)), device=dev)}
        values, J = emulator.jacobian(params, device=True, return_value=True)
        J0, value0 = J['y'].contiguous(), values['y'].contiguous()

        def composed():
            values, J = emulator.jacobian(params, device=True, return_value=True)
            return contracted(torch, J['y'], values['y'], P, data['y'])

        routes = [('gauss_newton(precision=P)', lambda: emulator.gauss_newton(params, ['y'], data=data, precision=P, device=True)),
                  ('the contraction alone', lambda: gauss_newton_dense(J0, value0, P, data['y'])),
                  ('gauss_newton (diagonal)', lambda: emulator.gauss_newton(params, {'y': wrow}, data=data, device=True)),
                  ('jacobian + einsum', composed),
                  ('einsum alone', lambda: contracted(torch, J0, value0, P, data['y']))]
        ours, theirs = routes[0][1](), routes[3][1]()
        ours = (ours[0], torch.stack([ours[1][name] for name in names], dim=1), ours[2])
        distance = [float(((a - b).abs().reshape(B, -1).max(dim=0).values / b.abs().reshape(B, -1).max(dim=0).values).max()) for a, b in zip(ours, theirs)]
        lines.append('B = %d: largest distance of the new call from jacobian + einsum, per block over the batch: fisher %.2e, grad %.2e, chi2 %.2e of the block\'s largest entry'
                     % ((B,) + tuple(distance)))
        del ours, theirs
        for _ in range(args.warmup):
            for name, fn in routes:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, fn in routes}
        for _ in range(args.repeats):
            for name, fn in routes:      # alternating
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                fn()
                stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop))
        for name, t in times.items():
            t = np.array(t)
            lines.append('  %-26s median %8.3f ms  (min %8.3f, max %8.3f over %d)' % (name, np.median(t), t.min(), t.max(), len(t)))
        median = {name: np.median(t) for name, t in times.items()}
        lines.append('  jacobian + einsum / gauss_newton(precision=P) = %.2f; einsum alone / the contraction alone = %.2f; gauss_newton(precision=P) / diagonal = %.2f'
                     % (median['jacobian + einsum'] / median['gauss_newton(precision=P)'], median['einsum alone'] / median['the contraction alone'],
                        median['gauss_newton(precision=P)'] / median['gauss_newton (diagonal)']))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
