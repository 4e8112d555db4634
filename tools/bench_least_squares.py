"""Batched Levenberg-Marquardt fits on the device (``Emulator.least_squares``: ``gauss_newton`` and one launch of ``cp_lm_step`` per iteration) against the
same rules written with what there was before them: ``Emulator.gauss_newton(device=True)`` and torch (``where``, ``clamp``, ``torch.linalg.cholesky_ex``,
``torch.cholesky_solve``: the forms that do not wait for the device), a dozen library launches per iteration.

    python tools/bench_least_squares.py [--batch 10000 64 1] [--ndim 8] [--nhidden 64 64 64] [--outputs 1024] [--order 3] [--iterations 20] [--repeats 20]
                                        [--warmup 3] [--processes 5] [--only mlp|taylor] [--once] [--geodesic] [--out FILE]

The two configurations of tools/bench_gauss_newton.py (MLP: ndim = 8, hidden (64, 64, 64), M = 1024, y operation log10; Taylor: 8 parameters at order 3,
M = 1024).  Per batch size B fits at once: the data is the prediction at B points with 1 % of noise, the weights are per point, the starts lie up to 2 % of
the ranges away, 20 iterations.  Timed with HIP events on the current stream, the two routes alternating in one run after the warm-up calls, in
``--processes`` fresh processes one after the other.  Before timing, one step of each route from the same state is held to the longdouble truth of
tests/lm_reference.py by its level rule, and the routes' final chi2 are compared.  Condition (exit status 1 if missed): at the first batch size the median of
``least_squares`` is below the median of the torch route in every process.  ``--once`` runs each route once after the warm-up and times nothing: the run to
put under ``rocprofv3 --kernel-trace --stats``.  Needs neither the reference nor the oracle.

``--geodesic``: after the two routes (timed exactly as without the option), ``least_squares(geodesic=True)`` and ``least_squares`` are timed alternating in a
loop of their own; one ``lm_accelerate`` from a recorded state is held to the longdouble truth of tests/lm_accel_reference.py (the fits whose gate lies
within a factor 1.25 of equality are left out: there the decision may fall either way); and for the noisy data and for noise-free data the count of
``gauss_newton`` evaluations (iterations) each route needs until every fit has ``status == 1`` is found by bisection (at most ``--most``) and reported,
with the count of corrections taken.  Nothing of this enters the exit status."""
import argparse
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

CONTROLS = dict(lambda_up=10., lambda_down=0.1, lambda_min=1e-12, lambda_max=1e12, ftol=1e-8)


def torch_step(torch, state, trial, lo, hi, lambda_up, lambda_down, lambda_min, lambda_max, ftol):
    """The rules of ``lm_step`` in torch, without a read-back: returns (new state, next)."""
    x, F, g, chi, lam, status, nacc = (state[name] for name in ('x', 'fisher', 'gradient', 'chi2', 'lambda', 'status', 'naccepted'))
    xt, Ft, gt, chit = (trial[name] for name in ('x', 'fisher', 'gradient', 'chi2'))
    frozen = status != 0
    accept = ~frozen & torch.isfinite(chit) & (chit <= chi)
    converged = accept & torch.isfinite(chi) & (chi - chit <= ftol * chi)
    lam = torch.where(accept & (nacc > 0), torch.clamp(lam * lambda_down, min=lambda_min), lam)
    reject = ~frozen & ~accept
    failed = reject & torch.isinf(chi)
    raised = lam * lambda_up
    stalled = reject & ~failed & (raised > lambda_max)
    lam = torch.where(reject & ~failed, torch.clamp(raised, max=lambda_max), lam)
    status = torch.where(converged, 1, torch.where(failed, 3, torch.where(stalled, 2, status))).to(torch.int32)
    nacc = nacc + accept.to(torch.int32)
    x, g, chi = torch.where(accept[:, None], xt, x), torch.where(accept[:, None], gt, g), torch.where(accept, chit, chi)
    F = torch.where(accept[:, None, None], Ft, F)
    held = (status == 0)[:, None] & (((x >= hi) & (g > 0)) | ((x <= lo) & (g < 0)))
    free = ~held
    A = F + lam[:, None, None] * torch.diag_embed(torch.diagonal(F, dim1=1, dim2=2))
    A = torch.where(free[:, :, None] & free[:, None, :], A, torch.eye(A.shape[1], dtype=A.dtype, device=A.device))
    L, info = torch.linalg.cholesky_ex(A)
    status = torch.where((status == 0) & (info > 0), 3, status).to(torch.int32)
    delta = torch.cholesky_solve(torch.where(held, 0., g)[..., None], L)[..., 0]
    nxt = torch.where((status == 0)[:, None] & free, torch.clamp(x + delta, min=lo, max=hi), x)
    return {'x': x, 'fisher': F, 'gradient': g, 'chi2': chi, 'lambda': lam, 'status': status, 'naccepted': nacc}, nxt


def torch_least_squares(torch, emulator, start, weights, data, lo, hi, niterations, record=None):
    from cosmoprimo_amd.emulators.tools import lm_state
    names = list(emulator.params)
    x = torch.clamp(torch.stack([start[name] for name in names], dim=1), min=lo, max=hi)
    state = lm_state(x)
    for iteration in range(niterations):
        fisher, gradient, chi2 = emulator.gauss_newton({name: x[:, i] for i, name in enumerate(names)}, weights, data=data, device=True)
        trial = {'x': x, 'fisher': fisher, 'gradient': torch.stack([gradient[name] for name in names], dim=1), 'chi2': chi2}
        if record is not None and iteration == record[0]:
            record[1].update(state={name: value.clone() for name, value in state.items()}, trial=trial)
        state, x = torch_step(torch, state, trial, lo, hi, **CONTROLS)
    return state


def check_one_step(torch, lines, recorded, lo, hi):
    """One step of both routes from the state and the trial ``recorded`` against the longdouble truth, a block a fit, 16 levels (tests/lm_reference.py)."""
    import lm_reference as lr
    from cosmoprimo_amd.emulators.tools import lm_step
    state, trial = recorded['state'], recorded['trial']
    theirs = torch_step(torch, state, trial, lo, hi, **CONTROLS)[1].cpu().numpy()
    mine = {name: value.clone() for name, value in state.items()}
    ours = lm_step(mine, trial, lo, hi, **CONTROLS).cpu().numpy()
    host = lambda d: {name: value.cpu().numpy() for name, value in d.items()}      # noqa: E731
    args = (host(state), host(trial), lo.cpu().numpy(), hi.cpu().numpy())
    (new64, next64, held64), (newld, nextld, heldld) = lr.step(*args, dtype='f8', **lr.CONTROLS), lr.step(*args, dtype=np.longdouble, **lr.CONTROLS)
    assert np.array_equal(new64['status'], mine['status'].cpu().numpy()) and np.array_equal(new64['status'], newld['status'])
    lr.assert_within(ours, nextld, next64, 'lm_step')
    lr.assert_within(theirs, nextld, next64, 'torch')
    lines.append('  one step of each route from the same state: both within 16 levels of the longdouble truth; lm_step has the bits of the float64 restatement: %s'
                 % (ours.tobytes() == next64.tobytes()))


def check_one_acceleration(torch, lines, emulator, recorded, weights, lo, hi):
    """One lm_accelerate from the state and the trial ``recorded`` against the longdouble truth, a block a fit, 16 levels (tests/lm_accel_reference.py)."""
    import lm_accel_reference as la
    import lm_reference as lr
    from cosmoprimo_amd.emulators.tools import lm_accelerate, lm_step
    names = list(emulator.params)
    state = {name: value.clone() for name, value in recorded['state'].items()}
    nxt, v = lm_step(state, recorded['trial'], lo, hi, return_velocity=True, **CONTROLS)
    at = {name: state['x'][:, i] for i, name in enumerate(names)}
    q = emulator.jvp2(at, {name: v[:, i] for i, name in enumerate(names)}, device=True)
    h = emulator.vjp(at, {key: weights[key] * q[key] for key in weights}, device=True)
    h = torch.stack([h[name] for name in names], dim=1)
    count = torch.zeros(len(v), dtype=torch.int32, device=v.device)
    ours = lm_accelerate(state, v, h, lo, hi, naccelerated=count).cpu().numpy()
    host = lambda d: {name: value.cpu().numpy() for name, value in d.items()}      # noqa: E731
    args = (host(state), v.cpu().numpy(), h.cpu().numpy(), lo.cpu().numpy(), hi.cpu().numpy())
    (next64, taken64), (nextld, takenld) = la.accelerate(*args, dtype='f8'), la.accelerate(*args, dtype=np.longdouble)
    ratio = la.gate_ratio(*args, dtype='f8')
    clear = ~((ratio > 0.8) & (ratio < 1.25))
    taken = count.cpu().numpy() == 1
    assert np.array_equal(taken[clear], taken64[clear]) and np.array_equal(taken64[clear], takenld[clear])
    same = clear | ((taken == taken64) & (taken64 == takenld))
    lr.assert_within(ours[same], nextld[same], next64[same], 'lm_accelerate')
    lines.append('  one lm_accelerate from a recorded state: within 16 levels of the longdouble truth; %d of %d fits take the correction (%d within 1.25 of the gate); the bits '
                 'of the float64 restatement: %s' % (taken.sum(), len(taken), (~clear).sum(), ours.tobytes() == next64.tobytes()))


def evaluations(emulator, start, weights, data, geodesic, most):
    """(the least count of iterations after which every fit has status 1, or None if ``most`` do not suffice; status counts and corrections there)"""
    def run(n):
        info = emulator.least_squares(start, weights, data, niterations=n, device=True, geodesic=geodesic, **CONTROLS)[2]
        status = info['status'].cpu().numpy()
        return bool((status == 1).all()), np.bincount(status, minlength=4).tolist(), (info['naccelerated'].cpu().numpy() if geodesic else None)

    last = run(most)
    if not last[0]:
        return None, last[1], last[2]
    below, above = 0, most
    while above - below > 1:
        middle = (below + above) // 2
        now = run(middle)
        if now[0]:
            above, last = middle, now
        else:
            below = middle
    return above, last[1], last[2]


def compare_geodesic(torch, lines, emulator, start, weights, data, clean, recorded, lo, hi, args):
    check_one_acceleration(torch, lines, emulator, recorded, weights, lo, hi)
    if args.once:
        emulator.least_squares(start, weights, data, niterations=args.iterations, device=True, geodesic=True, **CONTROLS)
        torch.cuda.synchronize()
        return
    for what, d in (('noisy', data), ('noise-free', clean)):
        for geodesic in (False, True):
            count, status, taken = evaluations(emulator, start, weights, d, geodesic, args.most)
            lines.append('  %-10s data, %-8s: every fit has status 1 after %s evaluations (status counts there %s%s)' % (
                what, 'geodesic' if geodesic else 'plain', count if count is not None else 'more than %d' % args.most, status,
                '; corrections taken per fit %d .. %d, mean %.2f' % (taken.min(), taken.max(), taken.mean()) if taken is not None else ''))
    routes = [('least_squares', lambda: emulator.least_squares(start, weights, data, niterations=args.iterations, device=True, **CONTROLS)),
              ('least_squares, geodesic', lambda: emulator.least_squares(start, weights, data, niterations=args.iterations, device=True, geodesic=True, **CONTROLS))]
    for _ in range(args.warmup):
        for name, fn in routes:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, fn in routes}
    for _ in range(args.repeats):
        for name, fn in routes:      # alternating
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            fn()
            end.record()
            end.synchronize()
            times[name].append(begin.elapsed_time(end))
    for name, t in times.items():
        t = np.array(t)
        lines.append('  %-24s median %8.3f ms  (min %8.3f, max %8.3f over %d), %.3f ms an iteration' % (name, np.median(t), t.min(), t.max(), len(t), np.median(t) / args.iterations))
    lines.append('  the correction costs %.3f ms an iteration' % ((np.median(times['least_squares, geodesic']) - np.median(times['least_squares'])) / args.iterations))


def compare(torch, lines, emulator, truth, M, args, rng):
    B, ndim = (int(n) for n in truth.shape)
    names = list(emulator.params)
    dev = truth.device
    lo, hi = (torch.as_tensor(np.array([emulator.params[name][side] for name in names]), device=dev) for side in (0, 1))
    value = emulator.predict({name: truth[:, i] for i, name in enumerate(names)}, device=True)['y']
    sigma = 1e-2 * value.abs().mean()
    data = {'y': value + sigma * torch.as_tensor(rng.standard_normal((B, M)), device=dev)}
    weights = {'y': torch.ones_like(value) / sigma**2}
    start = {name: truth[:, i] + 0.02 * (hi[i] - lo[i]) * torch.as_tensor(rng.uniform(-1., 1., B), device=dev) for i, name in enumerate(names)}
    routes = [('least_squares', lambda: emulator.least_squares(start, weights, data, niterations=args.iterations, device=True, **CONTROLS)),
              ('gauss_newton + torch', lambda: torch_least_squares(torch, emulator, start, weights, data, lo, hi, args.iterations))]
    recorded = {}
    theirs = torch_least_squares(torch, emulator, start, weights, data, lo, hi, args.iterations, record=(2, recorded))
    best, chi2, info = routes[0][1]()
    first = emulator.gauss_newton({name: torch.clamp(start[name], min=lo[i], max=hi[i]) for i, name in enumerate(names)}, weights, data=data, device=True)[2]
    lines.append('B = %d: chi2 / M from %.3g to %.3g (least_squares; status counts %s), largest relative distance of the two routes\' chi2 %.2e'
                 % (B, float(first.mean()) / M, float(chi2.mean()) / M, np.bincount(info['status'].cpu().numpy(), minlength=4).tolist(),
                    float(((chi2 - theirs['chi2']).abs() / chi2).max())))
    check_one_step(torch, lines, recorded, lo, hi)
    for _ in range(args.warmup):
        for name, fn in routes:
            fn()
    torch.cuda.synchronize()
    if args.once:
        for name, fn in routes:
            fn()
        torch.cuda.synchronize()
        if args.geodesic:
            compare_geodesic(torch, lines, emulator, start, weights, data, {'y': value}, recorded, lo, hi, args)
        return None
    times = {name: [] for name, fn in routes}
    for _ in range(args.repeats):
        for name, fn in routes:      # alternating
            begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            begin.record()
            fn()
            end.record()
            end.synchronize()
            times[name].append(begin.elapsed_time(end))
    for name, t in times.items():
        t = np.array(t)
        lines.append('  %-22s median %8.3f ms  (min %8.3f, max %8.3f over %d)' % (name, np.median(t), t.min(), t.max(), len(t)))
    ratio = np.median(times['gauss_newton + torch']) / np.median(times['least_squares'])
    lines.append('  gauss_newton + torch / least_squares = %.2f' % ratio)
    if args.geodesic:
        compare_geodesic(torch, lines, emulator, start, weights, data, {'y': value}, recorded, lo, hi, args)
    return ratio


def emulator_of(engine, lo, hi, M):
    from cosmoprimo_amd.emulators import Emulator
    emulator = Emulator(None, params={'p%d' % i: (float(a), float(b)) for i, (a, b) in enumerate(zip(lo, hi))}, engine=engine)
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['y'], [(M,)], {}
    return emulator


def run(args):
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine, TaylorEmulatorEngine
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(0)
    M, ndim, nhidden = args.outputs, args.ndim, tuple(args.nhidden)
    lines, ratios = [], []
    if args.only != 'taylor':
        engine = MLPEmulatorEngine(nhidden=nhidden, yoperation='log10', device=dev)
        lo, hi = rng.uniform(0., 1., ndim), rng.uniform(2., 3., ndim)
        ylo, yhi = rng.uniform(-2., 0., M), rng.uniform(1., 3., M)
        engine.xoperations = [{'name': 'scale', 'offset': lo, 'scale': hi - lo}]
        engine.yoperations = [{'name': 'log10'}, {'name': 'scale', 'offset': ylo, 'scale': yhi - ylo}]
        engine.parameters, engine.ndim, engine.M = engine.initial_parameters(ndim, M, seed=1), ndim, M
        lines.append('MLP emulator: ndim = %d, hidden %s, M = %d outputs, silu, y operation log10, float64, %d iterations' % (ndim, nhidden, M, args.iterations))
        for B in args.batch:
            truth = torch.as_tensor(rng.uniform(lo + 0.1 * (hi - lo), hi - 0.1 * (hi - lo), (B, ndim)), device=dev)
            ratios.append(compare(torch, lines, emulator_of(engine, lo, hi, M), truth, M, args, rng))
    if args.only != 'mlp':
        powers = np.array([p for total in range(args.order + 1) for p in itertools.product(range(args.order + 1), repeat=ndim) if sum(p) == total], dtype='i4')
        taylor = TaylorEmulatorEngine.from_state({'center': np.full(ndim, 0.5), 'powers': powers, 'derivatives': rng.normal(0., 1., (len(powers), M))}, device=dev)
        lines.append('Taylor emulator: ndim = %d, order %d (%d terms), M = %d outputs, float64, %d iterations' % (ndim, args.order, len(powers), M, args.iterations))
        for B in args.batch:
            truth = torch.as_tensor(rng.uniform(0.42, 0.58, (B, ndim)), device=dev)
            ratios.append(compare(torch, lines, emulator_of(taylor, np.full(ndim, 0.4), np.full(ndim, 0.6), M), truth, M, args, rng))
    print('\n'.join(lines))
    first = [ratio for ratio in ratios[::len(args.batch)] if ratio is not None]      # the first batch size of each engine
    return 0 if all(ratio > 1. for ratio in first) else 1


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, nargs='+', default=[10000, 64, 1])
    parser.add_argument('--ndim', type=int, default=8)
    parser.add_argument('--nhidden', type=int, nargs='+', default=[64, 64, 64])
    parser.add_argument('--outputs', type=int, default=1024)
    parser.add_argument('--order', type=int, default=3)
    parser.add_argument('--iterations', type=int, default=20)
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    parser.add_argument('--processes', type=int, default=5)
    parser.add_argument('--only', choices=['mlp', 'taylor'], default=None)
    parser.add_argument('--once', action='store_true')
    parser.add_argument('--geodesic', action='store_true')
    parser.add_argument('--most', type=int, default=200, help='the iterations at which --geodesic gives up counting evaluations')
    parser.add_argument('--out', default=None)
    parser.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = parser.parse_args()
    if args.child or args.once:
        sys.exit(run(args))
    forwarded = [arg for arg in sys.argv[1:]]
    if args.out:
        at = forwarded.index('--out')
        del forwarded[at:at + 2]
    texts, status = [], 0
    for process in range(args.processes):      # fresh processes, one after the other
        done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'] + forwarded, capture_output=True, text=True)
        texts.append('process %d of %d (exit status %d)\n%s' % (process + 1, args.processes, done.returncode, done.stdout))
        if done.returncode:
            texts[-1] += done.stderr[-2000:]
            status = 1
            if done.returncode != 1:      # not the condition: something broke, nothing more is started
                break
    text = '\n'.join(texts) + ('\nevery process: the median of least_squares is below the median of the torch route at B = %d\n' % args.batch[0] if not status else
                               '\nthe condition is missed, or a process failed\n')
    print(text)
    if args.out:
        with open(args.out, 'w') as file:
            file.write(text)
    sys.exit(status)


if __name__ == '__main__':
    main()
