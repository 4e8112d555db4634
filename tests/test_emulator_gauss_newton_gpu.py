"""GPU: Emulator.gauss_newton on the toy calculator of tests/mlp_reference.py (3 parameters) with its curve cut into three keys -- 'head' (3 values),
'middle' (2), 'tail' (2) -- beside the scalar 'product' and the fixed 'x': a Taylor emulator of order 3 fitted here, and an MLP loaded from a golden
configuration of tests/golden/mlp.npz (no training) under the same keys.  Weights on 'head' and 'tail' are two runs of columns, [0, 3) and [5, 7).

fisher, gradient and chi2 against the contraction, in longdouble on the host, of what ``Emulator.jacobian`` and ``Emulator.predict`` return, by the rule of
tests/jacobian_reference.py (a block is an (i, j) entry of fisher, an i of the gradient, or chi2, over the batch; the level is that of the same contraction in
float64, floored at 1.1e-16; 16 levels allowed); data = value x (1 + 0.05 xi), weights over three decades.  Then: scalar parameters, ``return_value=True``
against ``predict``, ``device=True`` without a read-back (the call is recorded into a HIP graph, the approach of tests/test_no_host_sync_gpu.py), and a
Levenberg-Marquardt loop on noise-free data for 64 fits at once."""
import numpy as np
import pytest

import gauss_newton_reference as gr
import jacobian_reference as jr
import mlp_reference as mr

pytestmark = pytest.mark.gpu
NAMES = list(mr.TOY_LIMITS)
XGRID = np.linspace(0.1, 1., 7)
KEYS, SHAPES = ['head', 'middle', 'tail', 'product'], [(3,), (2,), (2,), ()]


def calculator(**params):
    out = mr.toy(*[params[name] for name in NAMES])
    return {'head': out[..., :3], 'middle': out[..., 3:5], 'tail': out[..., 5:7], 'product': out[..., 7], 'x': XGRID}


@pytest.fixture(scope='module')
def emulators(golden):
    from cosmoprimo_amd.emulators import Emulator, MLPEmulatorEngine
    taylor = Emulator(calculator, params=mr.TOY_LIMITS, engine='taylor', order=3, device='cuda:0')
    taylor.set_samples()
    taylor.fit()
    assert taylor.varied_keys == KEYS and list(taylor.fixed) == ['x']
    mlp = Emulator(None, params=mr.TOY_LIMITS, device='cuda:0')
    mlp.engine = MLPEmulatorEngine.from_state(mr.engine_state(mr.golden_config(golden('mlp'), 0)), device='cuda:0')
    assert mlp.engine.M == 8
    mlp.varied_keys, mlp.varied_shapes, mlp.fixed = list(KEYS), list(SHAPES), {'x': XGRID}
    return {'taylor': taylor, 'mlp': mlp}


def batch(B=33, seed=1):
    rng = np.random.default_rng(seed)
    return {name: rng.uniform(*mr.TOY_LIMITS[name], B) for name in NAMES}


def operands(emulator, params, keys, seed=3):
    """(weights, data) by key for the outputs ``keys``: weights 10^U(-2, 1) per entry, data = prediction x (1 + 0.05 xi)"""
    rng = np.random.default_rng(seed)
    value = emulator.predict(params, keys=keys)
    return ({key: 10.**rng.uniform(-2., 1., value[key].shape) for key in keys}, {key: value[key] * (1. + 0.05 * rng.standard_normal(value[key].shape)) for key in keys})


def flat(d, keys, lead):
    return np.concatenate([np.asarray(d[key]).reshape(lead + (-1,)) for key in keys], axis=-1)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_against_the_contracted_jacobian(emulators, which):
    emulator = emulators[which]
    params, keys = batch(65, seed=4), ['head', 'tail']
    weights, data = operands(emulator, params, keys)
    calls = []
    engine, real = emulator.engine, emulator.engine.gauss_newton
    engine.gauss_newton = lambda X, w, **kwargs: calls.append(kwargs['columns']) or real(X, w, **kwargs)
    try:
        fisher, gradient, chi2 = emulator.gauss_newton(params, weights, data=data)
        only = emulator.gauss_newton(params, dict(weights, x=1.))      # a fixed key contributes nothing
    finally:
        del engine.gauss_newton
    assert calls == [(0, 3), (5, 7)] * 2      # one engine call per run
    assert isinstance(fisher, np.ndarray) and fisher.shape == (65, 3, 3) and chi2.shape == (65,) and list(gradient) == NAMES and all(g.shape == (65,) for g in gradient.values())
    assert np.array_equal(only, fisher) and np.array_equal(fisher, fisher.transpose(0, 2, 1))
    J, value = emulator.jacobian(params, keys=keys), emulator.predict(params, keys=keys)
    J, value, w, d = flat(J, keys, (65, 3)), flat(value, keys, (65,)), flat(weights, keys, (65,)), flat(data, keys, (65,))
    truth, restated = gr.contract(J, value, w, d, jr.LD), gr.contract(J, value, w, d, 'f8')
    gr.assert_within((fisher, np.stack([gradient[name] for name in NAMES], axis=1), chi2), truth, restated, '%s emulator' % which)
    # broadcast operands: one row of weights for all points, a scalar weight, data of a single point
    shared = {'head': weights['head'][0], 'tail': 2.}
    f2, g2, c2 = emulator.gauss_newton(params, shared, data={'head': data['head'][0], 'tail': data['tail']})
    f3, g3, c3 = emulator.gauss_newton(params, {'head': np.tile(weights['head'][0], (65, 1)), 'tail': np.full((65, 2), 2.)},
                                       data={'head': np.tile(data['head'][0], (65, 1)), 'tail': data['tail']})
    assert np.array_equal(f2, f3) and np.array_equal(c2, c3) and all(np.array_equal(g2[name], g3[name]) for name in NAMES)
    with pytest.raises(KeyError):
        emulator.gauss_newton(params, {'heads': 1.})
    with pytest.raises(KeyError):
        emulator.gauss_newton(params, {'head': 1.}, data={'head': 1., 'tail': 1.})
    with pytest.raises(ValueError):
        emulator.gauss_newton(params, weights, data={'head': 1.})
    zeros = emulator.gauss_newton(params, {}, data={})
    assert not zeros[0].any() and zeros[0].shape == (65, 3, 3) and not zeros[2].any() and not any(g.any() for g in zeros[1].values())


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_scalar_parameters_and_return_value(emulators, which):
    emulator = emulators[which]
    params, keys = batch(33), ['head', 'tail']
    weights, data = operands(emulator, params, keys)
    fisher, gradient, chi2 = emulator.gauss_newton(params, weights, data=data)
    point = {name: float(params[name][5]) for name in NAMES}
    at = lambda d: {key: value[5] for key, value in d.items()}      # noqa: E731
    f1, g1, c1 = emulator.gauss_newton(point, at(weights), data=at(data))
    assert f1.shape == (3, 3) and c1.shape == () and all(g.shape == () for g in g1.values())
    assert np.array_equal(f1, fisher[5]) and c1 == chi2[5] and all(g1[name] == gradient[name][5] for name in NAMES)
    assert emulator.gauss_newton(point, at(weights)).shape == (3, 3)
    for wkeys in (['head', 'tail'], ['tail', 'x', 'head'], ['product']):
        w, d = operands(emulator, params, [key for key in wkeys if key != 'x'])
        if 'x' in wkeys:
            w['x'] = 1.
        want = emulator.predict(params, keys=list(w))
        values, f, g, c = emulator.gauss_newton(params, w, data=d, return_value=True)
        assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want), wkeys
        values, f = emulator.gauss_newton(params, w, return_value=True)
        assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want) and f.shape == (33, 3, 3)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_results_without_read_back(emulators, which):
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}
    weights, data = operands(emulator, batch(17, seed=2), ['head', 'tail'])
    weights, data = ({key: torch.as_tensor(value, device=dev) for key, value in d.items()} for d in (weights, data))

    def fn():
        values, fisher, gradient, chi2 = emulator.gauss_newton({name: v[:] for name, v in static.items()}, weights, data=data, device=True, return_value=True)
        assert fisher.is_cuda and tuple(fisher.shape) == (17, 3, 3) and tuple(chi2.shape) == (17,) and gradient['b'].is_cuda and values['tail'].is_cuda
        only = emulator.gauss_newton({name: v[:] for name, v in static.items()}, {'product': weights['head'][:, 0]}, device=True)
        return torch.cat([fisher.reshape(17, 9), torch.stack([gradient[name] for name in NAMES], dim=1), chi2[:, None], values['head'], only.reshape(17, 9)], dim=1)

    capture_and_compare(torch, fn, static, fresh)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_levenberg_marquardt_recovers_noise_free_data(emulators, which):
    """64 fits at once: data is the emulator's own prediction at 64 points, the starts are those points moved by up to 5 % of each parameter's range, and ten
    steps (F + lambda diag F) delta = g with lambda = 1e-3 bring chi2 down by at least four decades in every fit (a functional check of the triple's signs
    and layout, not a tolerance on the parameters: the steps are those of an undamped Gauss-Newton iteration near its quadratic convergence)."""
    import torch
    emulator = emulators[which]
    B, keys = 64, list(KEYS)
    truth = batch(B, seed=7)
    data = emulator.predict(truth, keys=keys, device=True)
    rng = np.random.default_rng(8)
    theta = {name: torch.as_tensor(truth[name] + 0.05 * (mr.TOY_LIMITS[name][1] - mr.TOY_LIMITS[name][0]) * rng.uniform(-1., 1., B), device='cuda:0') for name in NAMES}
    weights = {key: 1. / (1e-2 * data[key].abs().mean())**2 * torch.ones_like(data[key]) for key in keys}
    history = []
    for step in range(10):
        fisher, gradient, chi2 = emulator.gauss_newton(theta, weights, data=data, device=True)
        history.append(chi2)
        g = torch.stack([gradient[name] for name in NAMES], dim=1)
        delta = torch.linalg.solve(fisher + 1e-3 * torch.diag_embed(torch.diagonal(fisher, dim1=1, dim2=2)), g)
        theta = {name: theta[name] + delta[:, i] for i, name in enumerate(NAMES)}
    history.append(emulator.gauss_newton(theta, weights, data=data, device=True)[2])
    history = torch.stack(history).cpu().numpy()      # (11, B)
    print('%s: chi2 from %.3g .. %.3g to %.3g .. %.3g' % (which, history[0].min(), history[0].max(), history[-1].min(), history[-1].max()))
    assert (history[0] > 0).all() and (history[-1] <= 1e-4 * history[0]).all()
    assert (history[1] < history[0]).all()      # the first step goes downhill in every fit
