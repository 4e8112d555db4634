"""Host time per call of the methods of ``Emulator`` at B = 1, where a call is its Python: the protocol of tools/bench_emulator_front.py (n calls back to back
after a synchronisation; host: until the last has returned, through: until the device has finished them; median, min and max of 20 repeats of 50 calls).

    python tools/bench_emulator_methods.py [FILE]

The emulator of that tool's last rows (MLP, ndim = 7, hidden (32, 32, 32), M = 422 x 30 + 256), the key 'background.table' (256 columns, one run), ``device=True``,
device tensors for weights, data and cotangents, the 256 x 256 identity for the dense precision.  ``least_squares`` (10 iterations), its geodesic form and ``hmc``
(2 trajectories of 6 steps: 13 evaluations) are divided by their count of evaluations, 5 calls per repeat.  Run it on two builds, twice each in separate processes
for a build's own spread (profiles/emulator_front_refactor.txt).  Needs neither the reference nor the oracle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench_emulator_front import per_call, synthetic_mlp      # noqa: E402


def main():
    import torch
    from cosmoprimo_amd.emulators import Emulator
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    emulator = Emulator(None, params={'p%d' % i: (0., 3.) for i in range(7)}, device=dev)
    emulator.engine, lo7, hi7 = synthetic_mlp(rng, 7, (32, 32, 32), 422 * 30 + 256, dev)
    emulator.varied_keys, emulator.varied_shapes = ['fourier.pk.delta_m.delta_m', 'background.table'], [(422, 30), (256,)]
    names = list(emulator.params)
    B = 1
    p = {name: torch.as_tensor(rng.uniform(lo7[i], hi7[i], B), device=dev) for i, name in enumerate(names)}
    t = {name: torch.as_tensor(rng.normal(0., 1., B), device=dev) for name in names}
    key = 'background.table'
    cot = {key: torch.as_tensor(rng.normal(0., 1., (B, 256)), device=dev)}
    value = emulator.predict(p, device=True, keys=key)[key]
    w = {key: torch.ones_like(value) / (1e-2 * value.abs().mean())**2}
    d = {key: value * (1. + 1e-2 * torch.as_tensor(rng.normal(0., 1., (B, 256)), device=dev))}
    P = torch.eye(256, dtype=torch.float64, device=dev)
    cases = [('predict', lambda: emulator.predict(p, device=True, keys='background')),
             ('jacobian', lambda: emulator.jacobian(p, device=True, keys='background')),
             ('jvp', lambda: emulator.jvp(p, t, device=True, keys='background')),
             ('jvp2', lambda: emulator.jvp2(p, t, device=True, keys='background')),
             ('vjp', lambda: emulator.vjp(p, cot, device=True)),
             ('vjp2', lambda: emulator.vjp2(p, cot, device=True)),
             ('gauss_newton', lambda: emulator.gauss_newton(p, w, data=d, device=True)),
             ('gauss_newton dense', lambda: emulator.gauss_newton(p, [key], data=d, device=True, precision=P)),
             ('chi2_hessian', lambda: emulator.chi2_hessian(p, w, d, device=True)),
             ('least_squares / 10 iterations', lambda: emulator.least_squares(p, w, d, niterations=10, device=True)),
             ('least_squares geodesic / 10', lambda: emulator.least_squares(p, w, d, niterations=10, device=True, geodesic=True)),
             ('hmc / 13 evaluations', lambda: emulator.hmc(p, w, d, nsamples=2, nwarmup=0, nleapfrog=6, device=True))]
    lines = ['%-32s %26s  %26s   (microseconds per call at B = 1: median (min .. max))' % ('Emulator method', 'host', 'through')]
    for name, fn in cases:
        n = 50 if '/' not in name else 5
        host, through = per_call(torch, fn, n, 20)
        div = 10 if '/ 10' in name else 13 if '/ 13' in name else 1
        lines.append('%-32s %s  %s' % ((name,) + tuple('%8.1f (%6.1f .. %6.1f)' % (np.median(x) / div, x.min() / div, x.max() / div) for x in (host, through))))
    text = '\n'.join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
