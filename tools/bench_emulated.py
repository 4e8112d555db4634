"""An emulated background of a batch of cosmologies: the prediction on the section's columns against the full prediction followed by slicing.

    python tools/bench_emulated.py [--batch 10000] [--repeats 10] [--warmup 2] [--out profiles/emulated_times.txt]

Set-up: the default calculator of ``DESI()`` emulated on Omega_m in (0.28, 0.34) and h in (0.64, 0.72), Taylor (order 2) and MLP (32, 32, 32; a few
epochs: its accuracy does not enter), each saved and read back through ``EmulatedEngine.read``.  Timed: from the parameters on the device to
``get_background().comoving_radial_distance(z)`` at 10 redshifts for B cosmologies -- a new ``Cosmology`` per repeat, wall clock between two
synchronisations, median and spread --

  range : as ``EmulatedEngine`` does it, ``Emulator.predict(params, keys='background', device=True)`` (cp_*_predict_columns on the section's columns)
  full  : the same engine with the section taken out of ``Emulator.predict(params, device=True)``, every column computed and stored

and the bytes each allocates at its peak (``torch.cuda.max_memory_allocated`` over the call, above what was held before it)."""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {'Omega_m': (0.28, 0.34), 'h': (0.64, 0.72)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=10000)
    parser.add_argument('--repeats', type=int, default=10)
    parser.add_argument('--warmup', type=int, default=2)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.fiducial import DESI
    from cosmoprimo_amd.emulators import Emulator, EmulatedEngine, get_calculator
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    B = args.batch
    params = {name: torch.as_tensor(rng.uniform(lo + 0.01, hi - 0.01, B), device=dev) for name, (lo, hi) in LIMITS.items()}
    z = np.linspace(0.1, 2., 10)
    taylor = Emulator(get_calculator(DESI()), params=LIMITS, engine='taylor', order=2, device=dev)
    taylor.set_samples()
    taylor.fit()
    mlp = Emulator(None, params=LIMITS, engine='mlp', nhidden=(32, 32, 32), device=dev)
    mlp.set_samples(samples=taylor.samples)
    mlp.fit(epochs=5)
    M = sum(int(np.prod(shape, dtype='i8')) for shape in taylor.varied_shapes)
    lines = ['EmulatedEngine, get_background().comoving_radial_distance(z) at %d redshifts for B = %d cosmologies; default calculator of DESI() on Omega_m, h: M = %d columns,'
             % (z.size, B, M), 'of which the background section holds %d; the full (B, M) table is %.1f MB' %
             (sum(int(np.prod(shape, dtype='i8')) for key, shape in zip(taylor.varied_keys, taylor.varied_shapes) if key.startswith('background.')), 8e-6 * B * M)]
    with tempfile.TemporaryDirectory() as base:
        for name, emulator in (('taylor', taylor), ('mlp', mlp)):
            fn = os.path.join(base, name + '.npy')
            emulator.save(fn)
            Range = EmulatedEngine.read(fn)

            class Full(EmulatedEngine.read(fn)):

                __module__ = EmulatedEngine.__module__      # where the engine looks for its sections

                def _predict(self, section):
                    prefix = section + '.'
                    predict = self._emulator.predict(self._emulator_params, device=True)
                    return {key[len(prefix):]: value for key, value in predict.items() if key.startswith(prefix)}

            results = {}
            for route, Engine in (('range', Range), ('full', Full)):
                def call():
                    return DESI(engine=Engine, **params).get_background().comoving_radial_distance(z)

                for _ in range(args.warmup):
                    results[route] = call()
                times, peaks = [], []
                for _ in range(args.repeats):
                    torch.cuda.synchronize(dev)
                    torch.cuda.reset_peak_memory_stats(dev)
                    before = torch.cuda.memory_allocated(dev)
                    start = time.perf_counter()
                    call()
                    torch.cuda.synchronize(dev)
                    times.append((time.perf_counter() - start) * 1e3)
                    peaks.append(torch.cuda.max_memory_allocated(dev) - before)
                t = np.array(times)
                lines.append('%-6s %-5s median %9.3f ms  (min %9.3f, max %9.3f over %d)  peak allocation %12d bytes (%.1f MB)' %
                             (name, route, np.median(t), t.min(), t.max(), len(t), max(peaks), 1e-6 * max(peaks)))
            lines.append('%-6s the two routes agree bit for bit: %s' % (name, bool(np.array_equal(results['range'], results['full'], equal_nan=True))))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
