"""GPU: Emulator.jacobian on the toy calculator of tests/mlp_reference.py (3 parameters; 'curve' of 7 values and the scalar 'product' vary, 'x' is fixed):
a Taylor emulator of order 3 fitted here, and an MLP loaded from a golden configuration of tests/golden/mlp.npz (no training).  Shapes and key sets for
scalar and array parameters, ``keys=`` against the full call, ``device=True`` without a read-back (the call is recorded into a HIP graph, the approach
of tests/test_no_host_sync_gpu.py), ``return_value=True`` against ``predict``, and the Taylor Jacobian against the toy function's analytic derivative."""
import numpy as np
import pytest

import jacobian_reference as jr
import mlp_reference as mr

pytestmark = pytest.mark.gpu
NAMES = list(mr.TOY_LIMITS)
XGRID = np.linspace(0.1, 1., 7)
MEASURED_DISTANCE = 5e-3


def calculator(**params):
    out = mr.toy(*[params[name] for name in NAMES])
    return {'curve': out[..., :7], 'product': out[..., 7], 'x': XGRID}


def toy_derivative(a, b, c):
    """(B, 3, 8) analytic derivative of ``mr.toy`` in longdouble."""
    a, b, c = (np.asarray(v).astype(jr.LD)[:, None] for v in (a, b, c))
    x = XGRID.astype(jr.LD)
    e = np.exp(a * x)
    one = np.ones_like(a)
    return np.stack([np.concatenate([x * e * np.sin(b * x), b * c], axis=1), np.concatenate([x * e * np.cos(b * x), a * c], axis=1),
                     np.concatenate([3 * c**2 * x * one, a * b], axis=1)], axis=1)


@pytest.fixture(scope='module')
def emulators(golden):
    from cosmoprimo_amd.emulators import Emulator, MLPEmulatorEngine
    taylor = Emulator(calculator, params=mr.TOY_LIMITS, engine='taylor', order=3, device='cuda:0')
    taylor.set_samples()
    taylor.fit()
    assert taylor.varied_keys == ['curve', 'product'] and list(taylor.fixed) == ['x']
    mlp = Emulator(None, params=mr.TOY_LIMITS, device='cuda:0')
    mlp.engine = MLPEmulatorEngine.from_state(mr.engine_state(mr.golden_config(golden('mlp'), 0)), device='cuda:0')
    assert mlp.engine.M == 8
    mlp.varied_keys, mlp.varied_shapes, mlp.fixed = ['curve', 'product'], [(7,), ()], {'x': XGRID}
    return {'taylor': taylor, 'mlp': mlp}


def batch(B=33, seed=1):
    rng = np.random.default_rng(seed)
    return {name: rng.uniform(*mr.TOY_LIMITS[name], B) for name in NAMES}


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_shapes_keys_and_values(emulators, which):
    import torch
    emulator = emulators[which]
    params = batch()
    X = np.column_stack([params[name] for name in NAMES])
    J = emulator.jacobian(params)
    assert list(J) == ['curve', 'product'] and J['curve'].shape == (33, 3, 7) and J['product'].shape == (33, 3)      # no fixed output: its derivative is zero
    assert all(isinstance(value, np.ndarray) for value in J.values())
    full = emulator.engine.jacobian(X).cpu().numpy()
    assert np.array_equal(J['curve'], full[:, :, :7]) and np.array_equal(J['product'], full[:, :, 7])      # the ndim axis in the order of Emulator.params
    point = {name: float(params[name][5]) for name in NAMES}
    Jp = emulator.jacobian(point)
    assert Jp['curve'].shape == (3, 7) and Jp['product'].shape == (3,)
    assert np.array_equal(Jp['curve'], J['curve'][5]) and np.array_equal(Jp['product'], J['product'][5])
    mixed = emulator.jacobian(dict(params, b=2.))      # scalars and arrays together, one of them a device tensor
    assert mixed['curve'].shape == (33, 3, 7)
    mixed_dev = emulator.jacobian(dict(params, a=torch.as_tensor(params['a'], device='cuda:0'), b=2.))
    assert np.array_equal(mixed_dev['curve'], mixed['curve'])
    # keys=: one run of columns per call, the same bits
    for keys, names in (('product', ['product']), (['curve'], ['curve']), (['product', 'curve'], ['curve', 'product']), (['x'], [])):
        got = emulator.jacobian(params, keys=keys)
        assert list(got) == names and all(np.array_equal(got[key], J[key]) for key in names), keys
    with pytest.raises(KeyError):
        emulator.jacobian(params, keys='curves')
    with pytest.raises(ValueError):
        emulator.jacobian({'a': 1., 'b': 2.})
    # return_value=True: predict's dictionary first
    for keys in (None, 'product', ['x', 'curve']):
        values, got = emulator.jacobian(params, keys=keys, return_value=True)
        want = emulator.predict(params, keys=keys)
        assert list(sorted(values)) == list(sorted(want)) and all(np.array_equal(values[key], want[key]) for key in want), keys
        assert all(np.array_equal(got[key], J[key]) for key in got) and set(got) == set(want) - {'x'}
    values, got = emulator.jacobian(point, return_value=True)
    assert values['curve'].shape == (7,) and np.array_equal(values['curve'], emulator.predict(point)['curve']) and got['product'].shape == (3,)


def test_keys_call_the_engine_once_per_run(emulators):
    """``keys=`` plans the columns with ``column_runs``: one engine call per maximal run, on that range only."""
    emulator = emulators['taylor']
    engine, calls = emulator.engine, []

    class Spy(object):
        name = engine.name
        _dev = engine._dev
        device = engine.device

        def jacobian(self, X, columns=None, return_value=False):
            calls.append(columns)
            return engine.jacobian(X, columns=columns, return_value=return_value)

    emulator.engine = Spy()
    try:
        emulator.jacobian(batch(), keys='product')
        emulator.jacobian(batch(), keys=['curve', 'product'])
        emulator.jacobian(batch())
    finally:
        emulator.engine = engine
    assert calls == [(7, 8), (0, 8), None]


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_views_without_read_back(emulators, which):
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}

    def fn():
        J = emulator.jacobian({name: v[:] for name, v in static.items()}, device=True)
        assert J['curve'].shape == (17, 3, 7) and J['product'].shape == (17, 3) and J['curve'].is_cuda
        assert J['curve'].data_ptr() + 7 * 8 == J['product'].data_ptr()      # views of one (B, ndim, 8) buffer
        values, J2 = emulator.jacobian({name: v[:] for name, v in static.items()}, device=True, keys='product', return_value=True)
        assert values['product'].shape == (17,) and values['product'].is_cuda and J2['product'].shape == (17, 3)
        return torch.cat([J['curve'].reshape(17, -1), J['product'], J2['product'], values['product'][:, None]], dim=1)

    capture_and_compare(torch, fn, static, fresh)


def test_taylor_against_the_analytic_derivative(emulators):
    """The order-3 Taylor emulator's Jacobian against the toy function's analytic derivative.  The yardstick is the distance of the longdouble derivative of
    the fitted polynomial (the truth of what the device computes) from the analytic derivative, per (parameter, column) block relative to the block's
    largest entry: measured 4.48e-3 at most over the blocks (truncation of the expansion and of its finite differences over the toy limits), held to
    MEASURED_DISTANCE = 5e-3.  The device is
    allowed that distance plus the rule of tests/jacobian_reference.py, and the distance itself must stay what was measured."""
    engine = emulators['taylor'].engine
    params = batch(65, seed=4)
    X = np.column_stack([params[name] for name in NAMES])
    analytic = toy_derivative(*[params[name] for name in NAMES])
    args = (engine.center, engine.powers, engine.derivatives, X)
    J_ld, J_64 = jr.taylor_jacobian(*args, dtype=jr.LD), jr.taylor_jacobian(*args, dtype='f8')
    top, level = jr.levels(J_ld, J_64)
    distance = np.abs(J_ld - analytic).max(axis=0)
    print('polynomial derivative against the analytic one: at most %.3g of a block' % float((distance / top).max()))
    assert float((distance / top).max()) <= MEASURED_DISTANCE
    J = emulators['taylor'].jacobian(params)
    got = np.concatenate([J['curve'], J['product'][:, :, None]], axis=2)
    assert (np.abs(got - analytic).max(axis=0) <= distance + jr.ALLOW * level * top).all()
    jr.assert_within(got, J_ld, J_64, 'taylor emulator')

