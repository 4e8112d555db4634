"""Batched prediction of the Taylor emulator, the fused kernel against the two-step route that existed before it.

    python tools/bench_taylor.py [--batch 10000] [--ndim 7] [--order 4] [--outputs 12660] [--repeats 20] [--warmup 3] [--out profiles/taylor_predict.txt]

The workload is a sampler's: B = 10^4 parameter points, 7 parameters at order 4 (T = 330 terms), M = 12 660 outputs ('fourier.pk.delta_m.delta_m', 422 x 30),
synthetic coefficients.  Timed with HIP events on the current stream after warm-up calls, median and spread (min, max) of the repeats:

  fused    : ``TaylorEmulatorEngine.predict`` (cp_taylor_predict: the monomials formed in LDS inside the GEMM)
  two-step : the monomials (B, T) by torch ops into memory, then ``LinearOperator.dense(derivatives.T)`` applied to them (linop_mfma_kernel)

The fraction of the matrix peak counts 2 B T M flops against 78.6 TFLOP/s (float64 matrix cores of one MI355X).  The two results are compared entry by entry.
Needs neither the reference nor the oracle."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12


def time_call(torch, fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return np.array(times)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=10000)
    parser.add_argument('--ndim', type=int, default=7)
    parser.add_argument('--order', type=int, default=4)
    parser.add_argument('--outputs', type=int, default=12660)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    from cosmoprimo_amd.spline import LinearOperator
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    powers = np.array([np.bincount(c, minlength=args.ndim) for total in range(args.order + 1)
                       for c in itertools.combinations_with_replacement(range(args.ndim), total)], dtype='i4').reshape(-1, args.ndim)
    T, M, B = len(powers), args.outputs, args.batch
    derivatives = rng.standard_normal((T, M))
    center = rng.uniform(0.5, 1.5, args.ndim)
    engine = TaylorEmulatorEngine.from_state({'center': center, 'powers': powers, 'derivatives': derivatives}, device=dev)
    X = torch.as_tensor(center + rng.uniform(-0.1, 0.1, (B, args.ndim)), device=dev)
    dense = LinearOperator.dense(np.ascontiguousarray(derivatives.T), device=dev)
    tpowers, tcenter = torch.as_tensor(powers, device=dev), torch.as_tensor(center, device=dev)

    def two_step():
        d = (X - tcenter)[:, None, :]
        mono = torch.where(tpowers > 0, d**tpowers, 1.).prod(dim=-1)
        return dense(mono)

    fused, ref = engine.predict(X), two_step()
    err = float((fused - ref).abs().max() / ref.abs().max())
    lines = ['Taylor emulator, batched prediction: B = %d points, ndim = %d, order %d (T = %d terms), M = %d outputs, float64' % (B, args.ndim, args.order, T, M),
             'largest difference between the two routes / largest value: %.2e' % err]
    flops = 2. * B * T * M
    results = {}
    for name, fn in [('fused (cp_taylor_predict)', lambda: engine.predict(X)), ('two-step (torch monomials + LinearOperator.dense)', two_step)]:
        t = time_call(torch, fn, args.repeats, args.warmup)
        results[name] = np.median(t)
        lines.append('%-52s median %8.3f ms  (min %8.3f, max %8.3f over %d)  %5.1f %% of the %.1f TFLOP/s float64 matrix peak' %
                     (name, np.median(t), t.min(), t.max(), len(t), 100. * flops / (np.median(t) * 1e-3) / PEAK, PEAK / 1e12))
    fused_ms, two_ms = results.values()
    lines.append('fused / two-step = %.3f' % (fused_ms / two_ms))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
