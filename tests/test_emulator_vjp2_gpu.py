"""GPU: ``Emulator.vjp2`` and ``Emulator.chi2_hessian`` on the emulators of tests/test_emulator_gauss_newton_gpu.py (the toy calculator cut into the keys 'head'
[0, 3), 'middle' [3, 5), 'tail' [5, 7), 'product' and the fixed 'x': a Taylor emulator of order 3 fitted here, an MLP from a golden configuration).

Truth: what ``Emulator.hessian(device=True)`` returns, contracted with the cotangents on the host in longdouble; the level is that of the same contraction
in float64, floored at 1.1e-16, a block one (i, j) over the batch, 16 levels allowed (tests/jacobian_reference.py).  The cotangents are the signed
q = w (data - value).  Cotangents on 'head' and 'tail' are two runs of columns.  ``chi2_hessian``: gradient and chi2 bit for bit those of ``gauss_newton``,
hessian bit for bit ``fisher - vjp2(q)`` of the public calls, a zero weight over a NaN datum, a dense precision against the truth and a diagonal one against
the weights' form."""
import numpy as np
import pytest

import gauss_newton_dense_reference as gd
import gauss_newton_reference as gr
import jacobian_reference as jr
from test_emulator_dense_precision_gpu import correlated
from test_emulator_gauss_newton_gpu import NAMES, batch, emulators, flat, operands  # noqa: F401

pytestmark = pytest.mark.gpu
TWO_RUNS = ['head', 'tail']
LD = jr.LD


def cotangents(weights, data, value):
    return {key: weights[key] * (data[key] - value[key]) for key in weights}


def contracted(emulator, params, q, keys, B, dtype):
    """sum over the entries of ``keys`` of q x hessian, (B, 3, 3) in ``dtype``"""
    H = emulator.hessian(params, device=True, keys=keys)
    H = np.concatenate([H[key].cpu().numpy().reshape(B, 3, 3, -1) for key in keys], axis=-1)
    return np.einsum('bc,bijc->bij', flat(q, keys, (B,)).astype(dtype), H.astype(dtype))


def within(device, truth, restated, what):
    B = len(truth)
    jr.assert_within(np.asarray(device).reshape(B, -1), truth.reshape(B, -1), restated.reshape(B, -1), what)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_against_the_contracted_hessian(emulators, which):      # noqa: F811
    emulator = emulators[which]
    B = 65
    params = batch(B, seed=4)
    weights, data = operands(emulator, params, TWO_RUNS)
    q = cotangents(weights, data, emulator.predict(params, keys=TWO_RUNS))
    calls = []
    engine, real = emulator.engine, emulator.engine.vjp2
    engine.vjp2 = lambda X, cot, **kwargs: calls.append(kwargs['columns']) or real(X, cot, **kwargs)
    try:
        C = emulator.vjp2(params, q)
        only = emulator.vjp2(params, dict(q, x=1.))      # a fixed key contributes nothing
    finally:
        del engine.vjp2
    assert calls == [(0, 3), (5, 7)] * 2      # one engine call per run
    assert isinstance(C, np.ndarray) and C.shape == (B, 3, 3) and np.array_equal(C, only) and np.array_equal(C, C.transpose(0, 2, 1))
    within(C, contracted(emulator, params, q, TWO_RUNS, B, LD), contracted(emulator, params, q, TWO_RUNS, B, 'f8'), '%s emulator' % which)
    # the runs' matrices are added in run order
    parts = [emulator.vjp2(params, {key: q[key]}) for key in TWO_RUNS]
    assert np.array_equal(C, parts[0] + parts[1])
    # a cotangent that broadcasts, every key at once
    every = {'head': q['head'][0], 'middle': 0.5, 'tail': q['tail'], 'product': q['head'][:, 0]}
    tiled = {'head': np.tile(q['head'][0], (B, 1)), 'middle': np.full((B, 2), 0.5), 'tail': q['tail'], 'product': q['head'][:, 0]}
    assert np.array_equal(emulator.vjp2(params, every), emulator.vjp2(params, tiled))
    keys = list(every)
    within(emulator.vjp2(params, tiled), contracted(emulator, params, tiled, keys, B, LD), contracted(emulator, params, tiled, keys, B, 'f8'), '%s emulator, every key' % which)
    zeros = emulator.vjp2(params, {})
    assert zeros.shape == (B, 3, 3) and not zeros.any()
    with pytest.raises(KeyError):
        emulator.vjp2(params, {'heads': 1.})


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_scalar_parameters_device_and_return_value(emulators, which):      # noqa: F811
    import torch
    emulator = emulators[which]
    params = batch(33)
    weights, data = operands(emulator, params, TWO_RUNS)
    q = cotangents(weights, data, emulator.predict(params, keys=TWO_RUNS))
    C = emulator.vjp2(params, q)
    point = {name: float(params[name][5]) for name in NAMES}
    c1 = emulator.vjp2(point, {key: value[5] for key, value in q.items()})
    assert c1.shape == (3, 3) and np.array_equal(c1, C[5])
    assert emulator.vjp2(point, {}).shape == (3, 3)
    values, again = emulator.vjp2(params, dict(q, x=1.), return_value=True)
    want = emulator.predict(params, keys=TWO_RUNS + ['x'])
    assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want) and np.array_equal(again, C)
    dev = torch.device('cuda', 0)
    on = emulator.vjp2({name: torch.as_tensor(v, device=dev) for name, v in params.items()}, {key: torch.as_tensor(v, device=dev) for key, v in q.items()}, device=True)
    assert isinstance(on, torch.Tensor) and on.device == emulator.engine._dev['device'] and np.array_equal(on.cpu().numpy(), C)
    values, on = emulator.vjp2(params, q, device=True, return_value=True)
    assert on.is_cuda and all(values[key].is_cuda for key in TWO_RUNS)
    assert emulator.vjp2(point, {key: value[5] for key, value in q.items()}, device=True).shape == (3, 3)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_chi2_hessian(emulators, which):      # noqa: F811
    import torch
    emulator = emulators[which]
    B = 33
    params = batch(B)
    weights, data = operands(emulator, params, TWO_RUNS)
    fisher, gradient, chi2 = emulator.gauss_newton(params, weights, data=data)
    hessian, g, c = emulator.chi2_hessian(params, weights, data)
    assert isinstance(hessian, np.ndarray) and hessian.shape == (B, 3, 3) and list(g) == NAMES
    assert np.array_equal(c, chi2) and all(np.array_equal(g[name], gradient[name]) for name in NAMES)
    q = cotangents(weights, data, emulator.predict(params, keys=TWO_RUNS))
    assert np.array_equal(hessian, fisher - emulator.vjp2(params, q)) and np.array_equal(hessian, hessian.transpose(0, 2, 1))
    assert np.abs(hessian - fisher).max() > 1e-6 * np.abs(fisher).max(), 'the residual curvature does not show'
    # scalar parameters, the values, the device
    point = {name: float(params[name][5]) for name in NAMES}
    at = lambda d: {key: value[5] for key, value in d.items()}      # noqa: E731
    h1, g1, c1 = emulator.chi2_hessian(point, at(weights), at(data))
    assert h1.shape == (3, 3) and np.array_equal(h1, hessian[5]) and c1 == chi2[5] and all(g1[name] == gradient[name][5] for name in NAMES)
    values, h2, g2, c2 = emulator.chi2_hessian(params, dict(weights, x=1.), data, return_value=True)
    want = emulator.predict(params, keys=TWO_RUNS + ['x'])
    assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want) and np.array_equal(h2, hessian)
    hd, gd_, cd = emulator.chi2_hessian(params, weights, data, device=True)
    assert hd.is_cuda and cd.is_cuda and gd_[NAMES[0]].is_cuda and np.array_equal(hd.cpu().numpy(), hessian)
    # a zero weight over a NaN datum: finite, and the call without that column
    w0, d0 = {key: value.copy() for key, value in weights.items()}, {key: value.copy() for key, value in data.items()}
    w0['tail'][:, 1], d0['tail'][:, 1] = 0., np.nan
    masked = emulator.chi2_hessian(params, w0, d0)
    d0['tail'][:, 1] = 1.
    plain = emulator.chi2_hessian(params, w0, d0)
    assert np.isfinite(masked[0]).all() and np.array_equal(masked[0], plain[0]) and np.array_equal(masked[2], plain[2])
    with pytest.raises(KeyError):
        emulator.chi2_hessian(params, {'heads': 1.}, {'heads': 1.})
    with pytest.raises(ValueError):
        emulator.chi2_hessian(params, weights, {'head': 1.})
    # a dense precision, listed against the order of the columns
    listed = ['tail', 'head']
    rng = np.random.default_rng(11)
    w = 10.**rng.uniform(-2., 1., 5)
    precision = correlated(w)
    hp, gp, cp_ = emulator.chi2_hessian(params, listed, data, precision=precision)
    fp, gp2, cp2 = emulator.gauss_newton(params, listed, data=data, precision=precision)
    assert np.array_equal(cp_, cp2) and all(np.array_equal(gp[name], gp2[name]) for name in NAMES)
    J, value, d = flat(emulator.jacobian(params, keys=listed), listed, (B, 3)), flat(emulator.predict(params, keys=listed), listed, (B,)), flat(data, listed, (B,))

    def restated(P, dtype):
        r = d.astype(dtype) - value.astype(dtype)
        qd = r @ P.astype(dtype)
        qd = {'tail': qd[:, :2], 'head': qd[:, 2:]}
        return gd.contract(J, value, P, d, dtype)[0] - contracted(emulator, params, qd, listed, B, dtype)

    within(hp, restated(precision, LD), restated(precision, 'f8'), '%s emulator, dense precision' % which)
    # a diagonal precision against the weights' form: both within the rule of the same truth
    diagonal = np.diag(w)
    by_key = {'tail': np.broadcast_to(w[:2], (B, 2)), 'head': np.broadcast_to(w[2:], (B, 3))}
    truth, level = restated(diagonal, LD), restated(diagonal, 'f8')
    within(emulator.chi2_hessian(params, listed, data, precision=diagonal)[0], truth, level, '%s emulator, diagonal precision' % which)
    within(emulator.chi2_hessian(params, by_key, data)[0], truth, level, '%s emulator, the weights of the diagonal' % which)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_results_without_read_back(emulators, which):      # noqa: F811
    """``device=True`` waits for nothing: both calls are recorded into a HIP graph and replayed on other points (tests/test_no_host_sync_gpu.py)"""
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}
    weights, data = operands(emulator, batch(17, seed=2), TWO_RUNS)
    weights, data = ({key: torch.as_tensor(value, device=dev) for key, value in d.items()} for d in (weights, data))

    def fn():
        params = {name: v[:] for name, v in static.items()}
        values, hessian, gradient, chi2 = emulator.chi2_hessian(params, weights, data, device=True, return_value=True)
        assert hessian.is_cuda and tuple(hessian.shape) == (17, 3, 3) and tuple(chi2.shape) == (17,) and gradient[NAMES[0]].is_cuda and values['tail'].is_cuda
        C = emulator.vjp2(params, {'product': weights['head'][:, 0], 'middle': data['tail']}, device=True)
        return torch.cat([hessian.reshape(17, 9), torch.stack([gradient[name] for name in NAMES], dim=1), chi2[:, None], values['head'], C.reshape(17, 9)], dim=1)

    capture_and_compare(torch, fn, static, fresh)
