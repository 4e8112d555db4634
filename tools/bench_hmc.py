"""Batched Hamiltonian Monte Carlo chains on the device (``Emulator.hmc``: one ``gauss_newton`` call and one launch of ``cp_hmc_step`` per leapfrog step) beside
the floor this design cannot go under: the same count of ``gauss_newton`` calls alone.

    python tools/bench_hmc.py [--batch 10000] [--ndim 2 8] [--nhidden 64 64 64] [--outputs 1024] [--order 3] [--nleapfrog 6] [--trajectories 10] [--repeats 20]
                              [--warmup 3] [--only mlp|taylor] [--once] [--out FILE]

The two engines of tools/bench_least_squares.py (MLP: hidden (64, 64, 64), M = 1024, y operation log10; Taylor: order 3, M = 1024) at each ``--ndim``.  B chains
at once: the data is the prediction at B points with 1 % of noise, the weights are per point, the chains start at those points.  Three routes, timed with HIP
events on the current stream, alternating in one run after the warm-up calls:
  hmc           ``Emulator.hmc(nsamples=trajectories, nwarmup=0, device=True)``: 1 + trajectories x nleapfrog evaluations, as many ``hmc_step`` launches;
  gauss_newton  1 + trajectories x nleapfrog calls of what ``hmc`` evaluates (``Emulator.gauss_newton(device=True)`` and the stacking of its gradient), at a fixed point;
  hmc_step      1 + trajectories x nleapfrog calls of ``hmc_step`` alone on a state of the run, trajectories closed and opened as ``hmc`` does.
Reported per trajectory (the median over ``--repeats``, divided by ``--trajectories``), with the share of ``hmc_step`` in ``hmc`` and the mean acceptance.
``--once`` runs each route once after the warm-up and times nothing: the run to put under ``rocprofv3 --kernel-trace --stats``.  Nothing enters the exit
status but a failure."""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emulator_of(engine, lo, hi, M):
    from cosmoprimo_amd.emulators import Emulator
    emulator = Emulator(None, params={'p%d' % i: (float(a), float(b)) for i, (a, b) in enumerate(zip(lo, hi))}, engine=engine)
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['y'], [(M,)], {}
    return emulator


def compare(torch, lines, emulator, truth, M, args, rng):
    from cosmoprimo_amd.emulators.tools import hmc_factor, hmc_state, hmc_step
    B, ndim = (int(n) for n in truth.shape)
    names = list(emulator.params)
    dev = truth.device
    lo, hi = (torch.as_tensor(np.array([emulator.params[name][side] for name in names]), device=dev) for side in (0, 1))
    value = emulator.predict({name: truth[:, i] for i, name in enumerate(names)}, device=True)['y']
    sigma = 1e-2 * value.abs().mean()
    data = {'y': value + sigma * torch.as_tensor(rng.standard_normal((B, M)), device=dev)}
    weights = {'y': torch.ones_like(value) / sigma**2}
    start = {name: truth[:, i] for i, name in enumerate(names)}
    ncalls = 1 + args.trajectories * args.nleapfrog

    def evaluate(x):
        fisher, gradient, chi2 = emulator.gauss_newton({name: x[:, i] for i, name in enumerate(names)}, weights, data=data, device=True)
        return fisher, torch.stack([gradient[name] for name in names], dim=1), chi2

    fisher, gradient, chi2 = evaluate(truth)
    base = hmc_state(truth, gradient, chi2)
    factor = hmc_factor(fisher, base['status'])
    trial = {'x': truth, 'gradient': gradient, 'chi2': chi2}

    def steps():
        state = {name: tensor.clone() for name, tensor in base.items()}
        hmc_step(state, trial, factor, lo, hi, 0.25, t_open=0)
        for t in range(args.trajectories):
            for leap in range(args.nleapfrog - 1):
                hmc_step(state, trial, factor, lo, hi, 0.25)
            hmc_step(state, trial, factor, lo, hi, 0.25, t_close=t, t_open=t + 1 if t + 1 < args.trajectories else None)

    def floor():
        for call in range(ncalls):
            evaluate(truth)

    routes = [('hmc', lambda: emulator.hmc(start, weights, data, nsamples=args.trajectories, nwarmup=0, nleapfrog=args.nleapfrog, device=True)),
              ('gauss_newton', floor), ('hmc_step', steps)]
    info = routes[0][1]()[2]
    lines.append('B = %d, ndim = %d: %d trajectories of %d steps; mean acceptance %.3f, %d trajectories left the box, status counts %s'
                 % (B, ndim, args.trajectories, args.nleapfrog, float(info['acceptance'].mean()), int(info['nout'].sum()),
                    np.bincount(info['status'].cpu().numpy(), minlength=4).tolist()))
    for _ in range(args.warmup):
        for name, fn in routes:
            fn()
    torch.cuda.synchronize()
    if args.once:
        for name, fn in routes:
            fn()
        torch.cuda.synchronize()
        return
    times = {name: [] for name, fn in routes}
    for _ in range(args.repeats):
        for name, fn in routes:      # alternating
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            fn()
            end.record()
            end.synchronize()
            times[name].append(begin.elapsed_time(end))
    medians = {}
    for name, t in times.items():
        t = np.array(t) / args.trajectories
        medians[name] = np.median(t)
        lines.append('  %-13s median %8.3f ms a trajectory  (min %8.3f, max %8.3f over %d runs of %d calls)' % (name, np.median(t), t.min(), t.max(), len(t), ncalls))
    lines.append('  hmc / gauss_newton = %.3f; hmc_step alone is %.1f %% of hmc; hmc - gauss_newton - hmc_step = %.3f ms a trajectory'
                 % (medians['hmc'] / medians['gauss_newton'], 100. * medians['hmc_step'] / medians['hmc'], medians['hmc'] - medians['gauss_newton'] - medians['hmc_step']))


def run(args):
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine, TaylorEmulatorEngine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    M, nhidden = args.outputs, tuple(args.nhidden)
    lines = []
    for ndim in args.ndim:
        if args.only != 'taylor':
            engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
            lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
            ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
            engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
            engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
            engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
            lines.append('MLP emulator: ndim = %d, hidden %s, M = %d outputs, silu, y operation log10, float64' % (ndim, nhidden, M))
            for B in args.batch:
                truth = torch.as_tensor(rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (B, ndim)), device=dev)
                compare(torch, lines, emulator_of(engine, lo, hi, M), truth, M, args, rng)
        if args.only != 'mlp':
            powers = np.array([p for total in range(args.order + 1) for p in itertools.product(range(args.order + 1), repeat=ndim) if sum(p) == total], dtype='i4')
            taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
            lines.append('Taylor emulator: ndim = %d, order %d (%d terms), M = %d outputs, float64' % (ndim, args.order, len(powers), M))
            for B in args.batch:
                truth = torch.as_tensor(rng.uniform(0.42, 0.58, (B, ndim)), device=dev)
                compare(torch, lines, emulator_of(taylor, np.full(ndim, 0.4), np.full(ndim, 0.6), M), truth, M, args, rng)
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text + '\n')
    return 0


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, nargs='+', default=[10000])
    parser.add_argument('--ndim', type=int, nargs='+', default=[2, 8])
    parser.add_argument('--nhidden', type=int, nargs='+', default=[64, 64, 64])
    parser.add_argument('--outputs', type=int, default=1024)
    parser.add_argument('--order', type=int, default=3)
    parser.add_argument('--nleapfrog', type=int, default=6)
    parser.add_argument('--trajectories', type=int, default=10)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--only', choices=['mlp', 'taylor'], default=None)
    parser.add_argument('--once', action='store_true')
    parser.add_argument('--out', default=None)
    sys.exit(run(parser.parse_args()))


if __name__ == '__main__':
    main()
