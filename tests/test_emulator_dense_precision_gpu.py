"""GPU: ``Emulator.gauss_newton(..., precision=)`` and ``Emulator.least_squares(..., precision=)`` on the emulators of
tests/test_emulator_gauss_newton_gpu.py (a Taylor emulator of order 3 fitted there, the golden MLP of tests/golden/mlp.npz; the toy's curve cut into 'head'
(3 values), 'middle' (2), 'tail' (2) beside the scalar 'product').

The keys ['tail', 'head'] are listed against the order of the columns ('head' is [0, 3), 'tail' [5, 7)): two runs, and a 5 x 5 precision whose rows and
columns the front has to permute.  fisher, gradient and chi2 against the contraction, in longdouble on the host, of what ``Emulator.jacobian`` and
``Emulator.predict`` return IN THE LISTED ORDER, by the rule of tests/jacobian_reference.py (tests/gauss_newton_dense_reference.py ``contract``; the case is
held to the cap of 32 floors like every other); ``precision=np.diag(w)`` against the diagonal call by the same rule; scalar parameters;
``return_value=True`` against ``predict``; the refusals; ``device=True`` recorded into a HIP graph (no read-back); and 64 Levenberg-Marquardt fits at once on
noise-free data under an 8 x 8 precision over all four keys, listed backwards: every fit ends converged (status 1), chi2 comes down by the four decades the
diagonal test (tests/test_emulator_least_squares_gpu.py) asks for -- its tolerance on a recovered fit; how far the parameters end from those that generated the
data is printed --, and ``info['covariance']`` is the inverse of the returned Fisher matrix by that test's rule (tests/lm_reference.py)."""
import numpy as np
import pytest

import gauss_newton_dense_reference as gd
import gauss_newton_reference as gr
import jacobian_reference as jr
import lm_reference as lr
import mlp_reference as mr
from test_emulator_gauss_newton_gpu import KEYS, NAMES, batch, emulators, flat  # noqa: F401

pytestmark = pytest.mark.gpu
LISTED = ['tail', 'head']


def correlated(w):
    """P[c, d] = 0.6^|c - d| sqrt(w_c w_d): positive definite, every entry positive"""
    c = np.arange(len(w))
    return 0.6**np.abs(c[:, None] - c[None, :]) * np.sqrt(w[:, None] * w[None, :])


def operands(emulator, params, keys, seed=3):
    """(precision (N, N) in the listed order, data by key): w = 10^U(-2, 1), data = prediction x (1 + 0.05 xi)"""
    rng = np.random.default_rng(seed)
    value = emulator.predict(params, keys=keys)
    N = sum(int(np.prod(value[key].shape[1:], dtype='i8')) for key in keys)
    return correlated(10.**rng.uniform(-2., 1., N)), {key: value[key] * (1. + 0.05 * rng.standard_normal(value[key].shape)) for key in keys}


def stacked(gradient):
    return np.stack([gradient[name] for name in NAMES], axis=1)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_against_the_contracted_jacobian(emulators, which):      # noqa: F811
    emulator = emulators[which]
    B = 65
    params = batch(B, seed=4)
    precision, data = operands(emulator, params, LISTED)
    calls = []
    engine, real = emulator.engine, emulator.engine.jacobian
    engine.jacobian = lambda X, **kwargs: calls.append((kwargs['columns'], tuple(kwargs['out'][1].shape), kwargs['out'][1].stride(1))) or real(X, **kwargs)
    try:
        fisher, gradient, chi2 = emulator.gauss_newton(params, LISTED, data=data, precision=precision)
        only = emulator.gauss_newton(params, LISTED, precision=precision)
    finally:
        del engine.jacobian
    assert calls == [((0, 3), (B, 3, 3), 5), ((5, 7), (B, 3, 2), 5)] * 2      # one engine call per run, straight into its slice of the (B, 3, 5) Jacobian
    assert isinstance(fisher, np.ndarray) and fisher.shape == (B, 3, 3) and chi2.shape == (B,) and list(gradient) == NAMES and all(g.shape == (B,) for g in gradient.values())
    assert np.array_equal(only, fisher) and np.array_equal(fisher, fisher.transpose(0, 2, 1))
    J, value = emulator.jacobian(params, keys=LISTED), emulator.predict(params, keys=LISTED)
    J, value, d = flat(J, LISTED, (B, 3)), flat(value, LISTED, (B,)), flat(data, LISTED, (B,))      # the listed order: tail, then head
    truth, restated = gd.contract(J, value, precision, d, jr.LD), gd.contract(J, value, precision, d, 'f8')
    level = gr.worst_level(truth, restated)
    print('%s: level %.3g floors' % (which, level))
    assert level <= gd.CAP
    gd.assert_within((fisher, stacked(gradient), chi2), truth, restated, '%s emulator' % which)
    # the same data vector listed in the order of the columns, the precision permuted by hand: the same bits (the front's permutation is exact)
    swap = np.array([2, 3, 4, 0, 1])
    f2, g2, c2 = emulator.gauss_newton(params, ['head', 'tail'], data=data, precision=precision[np.ix_(swap, swap)])
    assert np.array_equal(f2, fisher) and np.array_equal(c2, chi2) and np.array_equal(stacked(g2), stacked(gradient))
    # a device tensor for the precision, data that broadcasts
    import torch
    f3, g3, c3 = emulator.gauss_newton(params, LISTED, data={'tail': data['tail'], 'head': data['head'][0]}, precision=torch.as_tensor(precision, device='cuda:0'))
    f4, g4, c4 = emulator.gauss_newton(params, LISTED, data={'tail': data['tail'], 'head': np.tile(data['head'][0], (B, 1))}, precision=precision)
    assert np.array_equal(f3, fisher) and np.array_equal(c3, c4) and np.array_equal(stacked(g3), stacked(g4))
    # a zero on the diagonal drops the entry, whatever the data hold there
    masked, poisoned = precision.copy(), {key: value.copy() for key, value in data.items()}
    masked[1, 1] = 0.      # the second entry of 'tail'
    poisoned['tail'][:, 1] = np.nan
    f5, g5, c5 = emulator.gauss_newton(params, LISTED, data=poisoned, precision=masked)
    keep = np.array([0, 2, 3, 4])
    want = gd.contract(J[:, :, keep], value[:, keep], precision[np.ix_(keep, keep)], d[:, keep], jr.LD), gd.contract(J[:, :, keep], value[:, keep], precision[np.ix_(keep, keep)], d[:, keep], 'f8')
    gd.assert_within((f5, stacked(g5), c5), *want, '%s emulator, masked' % which)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_diagonal_precision_is_the_diagonal_call(emulators, which):      # noqa: F811
    emulator = emulators[which]
    B = 33
    params = batch(B)
    rng = np.random.default_rng(5)
    w = 10.**rng.uniform(-2., 1., 5)
    value = emulator.predict(params, keys=LISTED)
    data = {key: value[key] * (1. + 0.05 * rng.standard_normal(value[key].shape)) for key in LISTED}
    dense = emulator.gauss_newton(params, LISTED, data=data, precision=np.diag(w))
    diagonal = emulator.gauss_newton(params, {'tail': w[:2], 'head': w[2:]}, data=data)
    J, value, d = flat(emulator.jacobian(params, keys=LISTED), LISTED, (B, 3)), flat(value, LISTED, (B,)), flat(data, LISTED, (B,))
    truth, restated = gr.contract(J, value, w, d, jr.LD), gr.contract(J, value, w, d, 'f8')
    for name, result in (('dense', dense), ('diagonal', diagonal)):
        gr.assert_within((result[0], stacked(result[1]), result[2]), truth, restated, '%s emulator, %s' % (which, name))


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_scalar_parameters_and_return_value(emulators, which):      # noqa: F811
    emulator = emulators[which]
    params = batch(33)
    precision, data = operands(emulator, params, LISTED)
    fisher, gradient, chi2 = emulator.gauss_newton(params, LISTED, data=data, precision=precision)
    point = {name: float(params[name][5]) for name in NAMES}
    at = {key: value[5] for key, value in data.items()}
    f1, g1, c1 = emulator.gauss_newton(point, LISTED, data=at, precision=precision)
    assert f1.shape == (3, 3) and c1.shape == () and all(g.shape == () for g in g1.values())
    assert np.array_equal(f1, fisher[5]) and c1 == chi2[5] and all(g1[name] == gradient[name][5] for name in NAMES)
    assert emulator.gauss_newton(point, LISTED, precision=precision).shape == (3, 3)
    for keys in (LISTED, ['product'], ['product', 'tail', 'middle', 'head']):
        P, d = operands(emulator, params, keys)
        want = emulator.predict(params, keys=keys)
        values, f, g, c = emulator.gauss_newton(params, keys, data=d, precision=P, return_value=True)
        assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want), keys
        values, f = emulator.gauss_newton(params, keys, precision=P, return_value=True)
        assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want) and f.shape == (33, 3, 3)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_refusals(emulators, which):      # noqa: F811
    emulator = emulators[which]
    params = batch(9)
    precision, data = operands(emulator, params, LISTED)
    for method, tail in ((emulator.gauss_newton, {}), (emulator.least_squares, {'niterations': 1})):
        with pytest.raises(TypeError):      # a dictionary of weights beside a precision
            method(params, {'tail': 1., 'head': 1.}, data, precision=precision, **tail)
        with pytest.raises(KeyError):       # a fixed key
            method(params, ['tail', 'x'], data, precision=precision, **tail)
        with pytest.raises(KeyError):       # an unknown key
            method(params, ['tail', 'heads'], data, precision=precision, **tail)
        with pytest.raises(ValueError):     # the shape of the precision
            method(params, LISTED, data, precision=precision[:4, :4], **tail)
        with pytest.raises(ValueError):
            method(params, LISTED, data, precision=precision[0], **tail)
        with pytest.raises(ValueError):     # a key listed twice
            method(params, ['tail', 'head', 'tail'], data, precision=np.eye(7), **tail)
        with pytest.raises(KeyError):       # data for a key the precision does not cover
            method(params, ['tail'], data, precision=precision[:2, :2], **tail)
        with pytest.raises(ValueError):     # no data for a listed key
            method(params, LISTED, {'tail': data['tail']}, precision=precision, **tail)
    with pytest.raises(ValueError):
        emulator.least_squares(params, LISTED, None, precision=precision)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_results_without_read_back(emulators, which):      # noqa: F811
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}
    precision, data = operands(emulator, batch(17, seed=2), LISTED)
    data = {key: torch.as_tensor(value, device=dev) for key, value in data.items()}
    on_device = torch.as_tensor(precision, device=dev)

    def fn():
        values, fisher, gradient, chi2 = emulator.gauss_newton({name: v[:] for name, v in static.items()}, LISTED, data=data, device=True, return_value=True,
                                                               precision=precision)      # a host array: uploaded once, served from the cache while recording
        assert fisher.is_cuda and tuple(fisher.shape) == (17, 3, 3) and tuple(chi2.shape) == (17,) and gradient['b'].is_cuda and values['tail'].is_cuda
        only = emulator.gauss_newton({name: v[:] for name, v in static.items()}, LISTED, device=True, precision=on_device)
        best, least, info = emulator.least_squares({name: v[:] for name, v in static.items()}, LISTED, data, niterations=3, device=True, precision=on_device)
        return torch.cat([fisher.reshape(17, 9), torch.stack([gradient[name] for name in NAMES], dim=1), chi2[:, None], values['head'], only.reshape(17, 9),
                          torch.stack([best[name] for name in NAMES], dim=1), least[:, None], info['covariance'].reshape(17, 9)], dim=1)

    capture_and_compare(torch, fn, static, fresh)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_least_squares_on_noise_free_data(emulators, which):      # noqa: F811
    emulator = emulators[which]
    B, keys = 64, ['product', 'tail', 'middle', 'head']
    truth = batch(B, seed=7)
    start = {name: np.clip(truth[name] + 0.05 * (mr.TOY_LIMITS[name][1] - mr.TOY_LIMITS[name][0]) * np.random.default_rng(8).uniform(-1., 1., B), *mr.TOY_LIMITS[name])
             for name in NAMES}
    data = emulator.predict(truth, keys=keys)
    sigma = np.concatenate([np.full(int(np.prod(data[key].shape[1:], dtype='i8')), 1e-2 * np.abs(data[key]).mean()) for key in keys])
    precision = correlated(1. / sigma**2)
    before = emulator.gauss_newton(start, keys, data=data, precision=precision)[2]
    best, chi2, info = emulator.least_squares(start, keys, data, niterations=60, precision=precision)
    moved = max(np.abs(best[name] - truth[name]).max() / (mr.TOY_LIMITS[name][1] - mr.TOY_LIMITS[name][0]) for name in NAMES)
    print('%s: chi2 from %.3g .. %.3g to %.3g .. %.3g, status %s, at least %d acceptances, parameters within %.3g of their ranges' % (
        which, before.min(), before.max(), chi2.min(), chi2.max(), np.bincount(info['status'], minlength=4), info['naccepted'].min(), moved))
    assert chi2.shape == (B,) and list(best) == NAMES and info['fisher'].shape == info['covariance'].shape == (B, 3, 3)
    assert (info['status'] == 1).all()
    assert (before > 0).all() and (chi2 <= 1e-4 * before).all()      # the four decades of the diagonal test
    # ... which are two decades in the residual: a start within 5 % of a range ends within 0.05 % of it where the fit is linear; ten times that is allowed
    assert moved <= 5e-3
    # the bits gauss_newton returns at the best point
    fisher, gradient, again = emulator.gauss_newton(best, keys, data=data, precision=precision)
    assert np.array_equal(again, chi2) and np.array_equal(fisher, info['fisher']) and all(np.array_equal(gradient[name], info['gradient'][name]) for name in NAMES)
    # the covariance: the inverse of the returned Fisher matrix, by the rule of the diagonal test
    (inv64, info64), (invld, infold) = lr.spd_inverse(fisher, 'f8'), lr.spd_inverse(fisher, jr.LD)
    assert not info64.any() and np.array_equal(info['covariance'], info['covariance'].transpose(0, 2, 1))
    lr.assert_within(info['covariance'], invld, inv64, '%s: covariance' % which)
    # ... and numpy's inverse, to the error a float64 inversion may make: 100 roundings times the condition number
    inverse = np.linalg.inv(fisher)
    allowed = 100. * np.finfo('f8').eps * np.linalg.cond(fisher)[:, None, None] * np.abs(inverse).max(axis=(1, 2), keepdims=True)
    assert (np.abs(info['covariance'] - inverse) <= allowed).all()
