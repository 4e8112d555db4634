"""Batched prediction and one training epoch of the MLP emulator, the fused kernel against the unfused route.

    python tools/bench_mlp.py [--batch 10000] [--ndim 7] [--nhidden 32 32 32] [--outputs 12916] [--samples 10000] [--repeats 20] [--warmup 3] [--out profiles/mlp.txt]

The workload is a sampler's: B = 10^4 parameter points, M = 422 x 30 + 256 outputs ('fourier.pk.delta_m.delta_m' and the background, concatenated),
synthetic weights, y operation log10.  Timed with HIP events on the current stream after warm-up calls, median and spread (min, max) of the repeats:

  fused   : ``MLPEmulatorEngine.predict`` (cp_mlp_predict: x operation, hidden layers in LDS, output layer on the matrix cores, y operations in the epilogue)
  unfused : the same arithmetic as torch operations, each of which reads and writes memory (the hidden layers, then ``LinearOperator.dense`` of the
            output kernel, then bias, scale and 10^v as elementwise passes over (B, M))

against the floor of writing the result once, 8 B M bytes at 8 TB/s (HBM3E of one MI355X).  Then one training epoch as ``MLPEmulatorEngine.fit`` runs
it on ``--samples`` points: batches of 10 % (cp_mlp_loss_grad + cp_mlp_adam per step), and the validation loss.  Needs neither the reference nor the oracle."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM = 8e12


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
    parser.add_argument('--nhidden', type=int, nargs='+', default=[32, 32, 32])
    parser.add_argument('--outputs', type=int, default=422 * 30 + 256)
    parser.add_argument('--samples', type=int, default=10000)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    import time
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    from cosmoprimo_amd.emulators.tools.mlp import unpack_parameters
    from cosmoprimo_amd.spline import LinearOperator
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    B, M, ndim, nhidden = args.batch, args.outputs, args.ndim, tuple(args.nhidden)
    engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
    packed = engine.initial_parameters(ndim, M, seed=1)
    lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
    ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
    engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
    engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
    engine.parameters, engine.ndim, engine.M = packed, ndim, M
    X = torch.as_tensor(rng.uniform(lo, hi, (B, ndim)), device=dev)
    layers = [{name: torch.as_tensor(np.ascontiguousarray(value), device=dev) for name, value in layer.items() if name in ('kernel', 'bias')}
              for layer in unpack_parameters(packed, ndim, nhidden, M)]
    dense = LinearOperator.dense(np.ascontiguousarray(layers[-1]['kernel'].cpu().numpy().T), device=dev)
    tlo, tscale, tylo, tyscale = (torch.as_tensor(a, device=dev) for a in (lo, hi - lo, ylo, yhi - ylo))

    def unfused():
        h = (X - tlo) / tscale
        for layer in layers[:-1]:
            h = h @ layer['kernel'] + layer['bias']
            h = h / (1 + torch.exp(-h))
        return 10**((dense(h.contiguous()) + layers[-1]['bias']) * tyscale + tylo)

    fused, ref = engine.predict(X), unfused()
    err = float(((fused - ref).abs() / ref.abs()).max())
    lines = ['MLP emulator, batched prediction: B = %d points, ndim = %d, hidden %s, M = %d outputs, silu, y operation log10, float64' % (B, ndim, nhidden, M),
             'largest relative difference between the two routes: %.2e' % err]
    floor = 8. * B * M / HBM * 1e3
    results = {}
    for name, fn in [('fused (cp_mlp_predict)', lambda: engine.predict(X)), ('unfused (torch layers + LinearOperator.dense + elementwise)', unfused)]:
        t = time_call(torch, fn, args.repeats, args.warmup)
        results[name] = np.median(t)
        lines.append('%-60s median %8.3f ms  (min %8.3f, max %8.3f over %d)  %5.2f x the %.3f ms of writing 8 B M bytes at %.0f TB/s' %
                     (name, np.median(t), t.min(), t.max(), len(t), np.median(t) / floor, floor, HBM / 1e12))
    fused_ms, unfused_ms = results.values()
    lines.append('fused / unfused = %.3f' % (fused_ms / unfused_ms))
    # one training epoch
    n = args.samples
    Xs, Ys = rng.uniform(lo, hi, (n, ndim)), 10**rng.uniform(ylo, yhi, (n, M))
    trainer = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
    trainer.fit(Xs, Ys, {}, batch_frac=(0.1,), epochs=1, learning_rate=1e-3)      # warm-up: uploads, first launches
    torch.cuda.synchronize()
    epochs = 3
    start = time.perf_counter()
    trainer.fit(Xs, Ys, {}, batch_frac=(0.1,), epochs=epochs, learning_rate=1e-3, patience=epochs)
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - start
    start = time.perf_counter()
    trainer.fit(Xs, Ys, {}, batch_frac=(0.1,), epochs=0, learning_rate=1e-3)
    torch.cuda.synchronize()
    setup = time.perf_counter() - start
    steps = len(trainer.history) and (n - int(n * 0.1 + 0.5)) // trainer.history[0]['batch_size']
    lines.append('training: %d samples, batches of %d (%d steps per epoch + the validation loss): %.1f ms per epoch (wall clock, %d epochs; scaling, upload and split %.1f ms apart)'
                 % (n, trainer.history[0]['batch_size'], steps, (elapsed - setup) / epochs * 1e3, epochs, setup * 1e3))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')


if __name__ == '__main__':
    main()
