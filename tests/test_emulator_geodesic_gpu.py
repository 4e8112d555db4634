"""GPU: ``Emulator.least_squares(..., geodesic=True)`` on the emulators and the ``problem()`` of tests/test_emulator_least_squares_gpu.py (a Taylor emulator of
order 3 and the golden MLP on the toy calculator; 64 Levenberg-Marquardt fits at once).  The result is the stated composition of ``gauss_newton``,
``lm_step(return_velocity=True)``, ``jvp2``, the cotangent, ``vjp`` and ``lm_accelerate``, bit for bit, with diagonal weights over two runs of columns and with
a dense precision whose rows the front permutes; a zero weight (a zero on the diagonal of the precision) over a NaN datum leaves everything finite;
noise-free data comes down the project's four decades with no ``status == 3`` and every parameter inside its box; scalar parameters give scalar results; a
bad ``alpha`` raises; the call records into a HIP graph (17 fits); and ``geodesic=False`` is the call without the argument, bit for bit.

The start offsets are those of ``problem()``: 5 % of the ranges.  On the CPU, with the float64 restatements of tests/ (tests/lm_accel_reference.py on
tests/jacobian_reference.py and tests/jvp2_reference.py for the golden MLP, and on the toy function itself for its Taylor emulator), every one of the 64
fits takes the correction at least twice at that offset, with and without noise: nothing had to be widened, and ``naccelerated >= 1`` is asserted of all."""
import numpy as np
import pytest

import mlp_reference as mr
from test_emulator_dense_precision_gpu import correlated
from test_emulator_gauss_newton_gpu import KEYS, NAMES, emulators  # noqa: F401
from test_emulator_least_squares_gpu import B, HI, LO, clipped, problem

pytestmark = pytest.mark.gpu
TWO_RUNS = ['head', 'tail', 'product']      # [0, 3) and [5, 8): two maximal runs of columns
LISTED = ['tail', 'head']      # against the order of the columns: two runs, and a precision the front has to permute
INFO = ['covariance', 'fisher', 'gradient', 'lambda', 'naccelerated', 'naccepted', 'status']


def dense_problem(emulator, noise=1.):
    """(start, precision (5, 5) in the listed order, data) on the outputs LISTED"""
    start, weights, data = problem(emulator, noise=noise)
    w = np.concatenate([weights[key][0].ravel() for key in LISTED])
    return start, correlated(w), {key: data[key] for key in LISTED}


def flatten(result):
    best, chi2, info = result
    return [best[name] for name in NAMES] + [chi2] + [info[name] for name in sorted(info) if name != 'gradient'] + [info['gradient'][name] for name in NAMES]


def compose(emulator, start, weights, data, N, alpha, precision=None):
    """The stated composition, through the public methods: ``(state, naccelerated)``."""
    import torch
    from cosmoprimo_amd.emulators.tools import lm_accelerate, lm_state, lm_step
    dev = torch.device('cuda', 0)
    lo, hi = torch.as_tensor(LO, device=dev), torch.as_tensor(HI, device=dev)
    x = torch.clamp(torch.as_tensor(np.stack([start[name] for name in NAMES], axis=1), device=dev), min=lo, max=hi)
    state, count = lm_state(x, lambda0=1e-3), torch.zeros(len(x), dtype=torch.int32, device=dev)
    by_name = lambda X: {name: X[:, i] for i, name in enumerate(NAMES)}      # noqa: E731
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    if precision is not None:
        planned = [key for key in KEYS if key in weights]      # the order of the column plan: head, then tail
        sizes = {key: int(np.prod(np.shape(data[key])[1:], dtype='i8')) for key in weights}
        offset = dict(zip(weights, np.cumsum([0] + [sizes[key] for key in weights])))
        order = np.concatenate([offset[key] + np.arange(sizes[key]) for key in planned])
        permuted = torch.as_tensor(np.ascontiguousarray(precision[np.ix_(order, order)]), device=dev)
        dropped = permuted.diagonal() == 0
    for iteration in range(N):
        fisher, gradient, c = emulator.gauss_newton(by_name(x), weights, data=data, device=True, precision=precision)
        x, v = lm_step(state, {'x': x, 'fisher': fisher, 'gradient': torch.stack([gradient[name] for name in NAMES], dim=1), 'chi2': c}, lo, hi, return_velocity=True)
        at = by_name(state['x'])
        q = emulator.jvp2(at, by_name(v), device=True, keys=list(weights))
        if precision is None:
            w = {key: torch.as_tensor(weights[key], device=dev) for key in weights}
            cotangent = {key: torch.where(w[key] == 0, zero, w[key] * q[key]) for key in weights}
        else:
            flat = torch.cat([q[key].reshape(len(x), -1) for key in planned], dim=1)
            flat = torch.where(dropped, zero, torch.matmul(torch.where(dropped, zero, flat), permuted))
            edges = np.cumsum([0] + [sizes[key] for key in planned])
            cotangent = {key: flat[:, edges[k]:edges[k + 1]].reshape(q[key].shape) for k, key in enumerate(planned)}
        h = emulator.vjp(at, cotangent, device=True)
        x = lm_accelerate(state, v, torch.stack([h[name] for name in NAMES], dim=1), lo, hi, alpha=alpha, naccelerated=count)
    return state, count


@pytest.mark.parametrize('dense', [False, True], ids=['diagonal', 'dense'])
@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_composition(emulators, which, dense):      # noqa: F811
    import torch
    emulator = emulators[which]
    N, alpha = 4, 0.5
    if dense:
        start, precision, data = dense_problem(emulator)
        weights = LISTED
    else:
        start, weights, data = problem(emulator, noise=1.)
        weights, data, precision = {key: weights[key] for key in TWO_RUNS}, {key: data[key] for key in TWO_RUNS}, None
    best, chi2, info = emulator.least_squares(start, weights, data, niterations=N, device=True, precision=precision, geodesic=True, alpha=alpha)
    assert sorted(info) == INFO and info['naccelerated'].dtype == torch.int32 and tuple(info['naccelerated'].shape) == (B,) and info['naccelerated'].is_cuda
    state, count = compose(emulator, start, weights, data, N, alpha, precision=precision)
    assert torch.equal(state['x'], torch.stack([best[name] for name in NAMES], dim=1)) and torch.equal(state['chi2'], chi2) and torch.equal(state['fisher'], info['fisher'])
    assert torch.equal(state['gradient'], torch.stack([info['gradient'][name] for name in NAMES], dim=1))
    assert all(torch.equal(state[name], info[name]) for name in ('status', 'naccepted', 'lambda')) and torch.equal(count, info['naccelerated'])
    assert int(count.sum()) >= 1 and int(count.max()) <= N and int(state['naccepted'].min()) >= 1
    # the correction changes the path: the plain fits differ after as many iterations
    plain = emulator.least_squares(start, weights, data, niterations=N, device=True, precision=precision)
    assert not torch.equal(plain[1], chi2)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_geodesic_false_is_the_call_without_it(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    without, off = emulator.least_squares(start, weights, data, niterations=6), emulator.least_squares(start, weights, data, niterations=6, geodesic=False, alpha=0.3)
    assert sorted(off[2]) == [name for name in INFO if name != 'naccelerated']
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(flatten(without), flatten(off)))
    start, precision, data = dense_problem(emulator)
    without, off = (emulator.least_squares(start, LISTED, data, niterations=6, precision=precision, **tail) for tail in ({}, {'geodesic': False}))
    assert all(np.array_equal(a, b) for a, b in zip(flatten(without), flatten(off)))


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_noise_free_data(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator)
    before = emulator.gauss_newton(clipped(start), weights, data=data)[2]
    best, chi2, info = emulator.least_squares(start, weights, data, geodesic=True)
    plain = emulator.least_squares(start, weights, data)
    print('%s: chi2 from %.3g .. %.3g to %.3g .. %.3g (plain: %.3g .. %.3g), status %s (plain: %s), corrections taken %d .. %d of %d .. %d acceptances' % (
        which, before.min(), before.max(), chi2.min(), chi2.max(), plain[1].min(), plain[1].max(), np.bincount(info['status'], minlength=4),
        np.bincount(plain[2]['status'], minlength=4), info['naccelerated'].min(), info['naccelerated'].max(), info['naccepted'].min(), info['naccepted'].max()))
    assert isinstance(chi2, np.ndarray) and chi2.shape == (B,) and list(best) == NAMES and all(value.shape == (B,) for value in best.values())
    assert sorted(info) == INFO and info['naccelerated'].shape == (B,) and info['naccelerated'].dtype == np.int32
    assert (before > 0).all() and (chi2 <= 1e-4 * before).all() and (chi2 <= before).all()
    assert (info['naccepted'] >= 2).all() and (info['status'] != 3).all()
    assert (info['naccelerated'] >= 1).all() and (info['naccelerated'] <= 20).all()
    assert all((best[name] >= mr.TOY_LIMITS[name][0]).all() and (best[name] <= mr.TOY_LIMITS[name][1]).all() for name in NAMES)
    # the bits gauss_newton returns at the best point
    fisher, gradient, again = emulator.gauss_newton(best, weights, data=data)
    assert np.array_equal(again, chi2) and np.array_equal(fisher, info['fisher']) and all(np.array_equal(gradient[name], info['gradient'][name]) for name in NAMES)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_a_masked_nan_and_the_box(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1., outside=True)      # the odd fits end on a bound of c
    weights, data = {key: value.copy() for key, value in weights.items()}, {key: value.copy() for key, value in data.items()}
    weights['head'][:, 1], data['head'][:, 1] = 0., np.nan
    weights['product'][::3], data['product'][::3] = 0., np.nan
    best, chi2, info = emulator.least_squares(start, weights, data, niterations=30, geodesic=True)
    assert all(np.isfinite(value).all() for value in flatten((best, chi2, info)))
    assert all((best[name] >= mr.TOY_LIMITS[name][0]).all() and (best[name] <= mr.TOY_LIMITS[name][1]).all() for name in NAMES)
    c, g = best['c'][1::2], info['gradient']['c'][1::2]
    low, high = mr.TOY_LIMITS['c']
    on_bound = (c == high) | (c == low)
    print('%s: %d of %d odd fits end exactly on a bound of c' % (which, on_bound.sum(), on_bound.size))
    assert (((c == high) & (g > 0.)) | ((c == low) & (g < 0.)))[on_bound].all()
    # the dense route: a zero on the diagonal of the precision over a NaN datum
    start, precision, data = dense_problem(emulator)
    precision, data = precision.copy(), {key: value.copy() for key, value in data.items()}
    precision[1, 1] = 0.      # the second entry of 'tail'
    data['tail'][:, 1] = np.nan
    best, chi2, info = emulator.least_squares(start, LISTED, data, precision=precision, geodesic=True)
    assert all(np.isfinite(value).all() for value in flatten((best, chi2, info))) and (info['naccelerated'] <= 20).all()
    assert all((best[name] >= mr.TOY_LIMITS[name][0]).all() and (best[name] <= mr.TOY_LIMITS[name][1]).all() for name in NAMES)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_scalar_parameters_and_errors(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    at = lambda d: {key: value[5] for key, value in d.items()}      # noqa: E731
    point = {name: float(start[name][5]) for name in NAMES}
    best, chi2, info = emulator.least_squares(point, at(weights), at(data), geodesic=True)
    assert all(value.shape == () for value in best.values()) and chi2.shape == () and info['fisher'].shape == (3, 3) and info['covariance'].shape == (3, 3)
    assert info['status'].shape == () and info['naccepted'].shape == () and info['lambda'].shape == () and all(g.shape == () for g in info['gradient'].values())
    assert info['naccelerated'].shape == () and 0 <= info['naccelerated'] <= 20 and np.isfinite(chi2) and info['status'] != 3
    for alpha in (0., -0.75, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            emulator.least_squares(start, weights, data, geodesic=True, alpha=alpha)
    with pytest.raises(KeyError):
        emulator.least_squares(start, dict(weights, heads=1.), data, geodesic=True)
    with pytest.raises(ValueError):
        emulator.least_squares(start, weights, None, geodesic=True)


@pytest.mark.parametrize('dense', [False, True], ids=['diagonal', 'dense'])
@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_no_host_synchronisation(emulators, which, dense):      # noqa: F811
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    if dense:
        start, precision, data = dense_problem(emulator)
        weights, precision = LISTED, torch.as_tensor(precision, device=dev)
    else:
        start, weights, data = problem(emulator, noise=1.)
        weights, precision = {key: torch.as_tensor(value[:17], device=dev) for key, value in weights.items()}, None
    static = {name: torch.as_tensor(value[:17], device=dev) for name, value in start.items()}
    fresh = {name: torch.as_tensor(np.clip(value[17:34], *mr.TOY_LIMITS[name]), device=dev) for name, value in start.items()}
    data = {key: torch.as_tensor(value[:17], device=dev) for key, value in data.items()}

    def fn():
        best, chi2, info = emulator.least_squares({name: v[:] for name, v in static.items()}, weights, data, niterations=6, device=True, precision=precision, geodesic=True)
        assert chi2.is_cuda and tuple(info['covariance'].shape) == (17, 3, 3) and info['naccelerated'].is_cuda
        return torch.cat([torch.stack([best[name] for name in NAMES], dim=1), chi2[:, None], info['lambda'][:, None], info['status'][:, None].to(torch.float64),
                          info['naccepted'][:, None].to(torch.float64), info['naccelerated'][:, None].to(torch.float64), info['fisher'].reshape(17, 9),
                          info['covariance'].reshape(17, 9)], dim=1)

    capture_and_compare(torch, fn, static, fresh)
