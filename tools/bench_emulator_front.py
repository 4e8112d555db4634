"""Host time per call of the emulator engines' entry points, where they are launch-bound (B = 1) and where they are not (B = 10^4).

    python tools/bench_emulator_front.py [--repeats 20] [--out FILE]

The engines of tools/bench_vjp.py (MLP: ndim = 8, hidden (64, 64, 64), silu, M = 1024, y operation log10; Taylor: 8 parameters at order 3, 165 terms,
M = 1024): ``predict``, ``predict(columns=(768, 1024))`` -- the call ``Emulator.predict(keys=...)`` makes --, ``jacobian`` and ``vjp`` at B = 1 and
B = 10^4.  Then ``Emulator.predict(keys='background', device=True)`` over the engine of tools/bench_mlp.py (ndim = 7, hidden (32, 32, 32),
M = 422 x 30 + 256: 'fourier.pk.delta_m.delta_m' and 256 columns of 'background.table').  n calls are made back to back after a synchronisation
(n = 50 at B = 1, 5 at B = 10^4) and two times are taken, each divided by n:

  host    : until the last call has returned -- nothing inside waits for the device, so this is what the host spends on a call (Python, the checks of
            the C entry point, the launches)
  through : until the device has finished them -- the larger of host and device time per call

Median, min and max of the repeats.  Run it on two builds, twice each in separate processes for a build's own spread.  Needs neither the reference nor
the oracle."""
import argparse
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_mlp(rng, ndim, nhidden, M, dev):
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
    lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
    ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
    engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
    engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
    engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
    return engine, lo, hi


def per_call(torch, fn, n, repeats):
    for _ in range(3):
        fn()
    host, through = [], []
    for _ in range(repeats):
        torch.cuda.synchronize()
        start = time.perf_counter()
        for _ in range(n):
            fn()
        returned = time.perf_counter()
        torch.cuda.synchronize()
        host.append((returned - start) / n * 1e6)
        through.append((time.perf_counter() - start) / n * 1e6)
    return np.array(host), np.array(through)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.emulators import Emulator, TaylorEmulatorEngine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    ndim, M = 8, 1024
    mlp, lo, hi = synthetic_mlp(rng, ndim, (64, 64, 64), M, dev)
    powers = np.array([p for total in range(4) for p in itertools.product(range(4), repeat=ndim) if sum(p) == total], dtype='i4')
    taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
    cases = []
    for B in (1, 10000):
        cot = torch.as_tensor(rng.normal(0., 1., (B, M)), device=dev)
        for name, engine, X in (('mlp', mlp, rng.uniform(lo, hi, (B, ndim))), ('taylor', taylor, rng.uniform(0.4, 0.6, (B, ndim)))):
            X = torch.as_tensor(X, device=dev)
            cases += [('%s.predict' % name, B, lambda e=engine, X=X: e.predict(X)), ('%s.predict(columns)' % name, B, lambda e=engine, X=X: e.predict(X, columns=(768, 1024))),
                      ('%s.jacobian' % name, B, lambda e=engine, X=X: e.jacobian(X)),
                      ('%s.vjp' % name, B, lambda e=engine, X=X, c=cot: e.vjp(X, c))]
    emulator = Emulator(None, params={'p%d' % i: (0., 1.) for i in range(7)}, device=dev)
    emulator.engine, lo7, hi7 = synthetic_mlp(rng, 7, (32, 32, 32), 422 * 30 + 256, dev)
    emulator.varied_keys, emulator.varied_shapes = ['fourier.pk.delta_m.delta_m', 'background.table'], [(422, 30), (256,)]
    for B in (1, 10000):
        params = {name: torch.as_tensor(rng.uniform(lo7[i], hi7[i], B), device=dev) for i, name in enumerate(emulator.params)}
        cases.append(("Emulator.predict(keys='background')", B, lambda p=params: emulator.predict(p, device=True, keys='background')))
    lines = ['%-36s %6s  %26s  %26s   (microseconds per call: median (min .. max))' % ('call', 'B', 'host', 'through')]
    for name, B, fn in cases:
        host, through = per_call(torch, fn, 50 if B == 1 else 5, args.repeats)
        lines.append('%-36s %6d  %s  %s' % ((name, B) + tuple('%8.1f (%6.1f .. %6.1f)' % (np.median(t), t.min(), t.max()) for t in (host, through))))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
