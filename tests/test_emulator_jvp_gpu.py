"""GPU: Emulator.jvp on the toy calculator of tests/mlp_reference.py (3 parameters; 'curve' of 7 values and the scalar 'product' vary, 'x' is fixed), with
the emulators of tests/test_emulator_jacobian_gpu.py: a Taylor emulator of order 3 fitted here, and an MLP loaded from a golden configuration (no
training).  Shapes and key order for scalar, array, 2-D (K directions) and mixed host / device tangents, ``keys=`` as a section prefix and as names with
one engine call per run, ``return_value=True`` against ``predict``, ``device=True`` as views of one buffer without a read-back (the call is recorded into
a HIP graph, the approach of tests/test_no_host_sync_gpu.py), and equality within the rule of tests/jvp_reference.py with the tangents contracted with
``Emulator.jacobian``."""
import numpy as np
import pytest

import jacobian_reference as jr
import jvp_reference as pr
import mlp_reference as mr
from test_emulator_jacobian_gpu import NAMES, batch, emulators      # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def directions(B, K=None, seed=5):
    """{name: (B,) or (B, K)} of the order of each parameter's range"""
    rng = np.random.default_rng(seed)
    return {name: (mr.TOY_LIMITS[name][1] - mr.TOY_LIMITS[name][0]) * rng.normal(0., 1., (B,) if K is None else (B, K)) for name in NAMES}


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_shapes_keys_and_values(emulators, which):
    import torch
    emulator = emulators[which]
    params = batch()
    X = np.column_stack([params[name] for name in NAMES])
    tan = directions(33)
    out = emulator.jvp(params, tan)
    assert list(out) == ['curve', 'product'] and out['curve'].shape == (33, 7) and out['product'].shape == (33,)      # no fixed output: its derivative is zero
    assert all(isinstance(value, np.ndarray) for value in out.values())
    full = emulator.engine.jvp(X, np.column_stack([tan[name] for name in NAMES])).cpu().numpy()      # the components in the order of Emulator.params
    assert np.array_equal(out['curve'], full[:, :7]) and np.array_equal(out['product'], full[:, 7])
    tanK = directions(33, K=4)
    outK = emulator.jvp(params, tanK)
    assert list(outK) == ['curve', 'product'] and outK['curve'].shape == (33, 4, 7) and outK['product'].shape == (33, 4)
    fullK = emulator.engine.jvp(X, np.stack([tanK[name] for name in NAMES], axis=-1)).cpu().numpy()
    assert np.array_equal(outK['curve'], fullK[:, :, :7]) and np.array_equal(outK['product'], fullK[:, :, 7])
    one = emulator.jvp(params, {name: tanK[name][:, 2] for name in NAMES})      # a direction of the K alone: the same bits
    assert np.array_equal(one['curve'], outK['curve'][:, 2]) and np.array_equal(one['product'], outK['product'][:, 2])
    point = {name: float(params[name][5]) for name in NAMES}
    outp = emulator.jvp(point, {name: float(tan[name][5]) for name in NAMES})
    assert outp['curve'].shape == (7,) and outp['product'].shape == ()
    assert np.array_equal(outp['curve'], out['curve'][5]) and np.array_equal(outp['product'], out['product'][5])
    outp = emulator.jvp(point, {name: tanK[name][5:6] for name in NAMES})
    assert outp['curve'].shape == (4, 7) and np.array_equal(outp['curve'], outK['curve'][5])
    # a missing name is a zero component, a scalar broadcasts, (1, K) broadcasts over the points; host and device tangents together
    mixed = emulator.jvp(params, {'a': tanK['a'], 'c': 0.5})
    want = emulator.engine.jvp(X, np.stack([tanK['a'], np.zeros((33, 4)), np.full((33, 4), 0.5)], axis=-1)).cpu().numpy()
    assert np.array_equal(mixed['curve'], want[:, :, :7]) and np.array_equal(mixed['product'], want[:, :, 7])
    mixed_dev = emulator.jvp(params, {'a': torch.as_tensor(tanK['a'], device='cuda:0'), 'c': 0.5})
    assert np.array_equal(mixed_dev['curve'], mixed['curve'])
    row = emulator.jvp(dict(params, a=torch.as_tensor(params['a'], device='cuda:0')), {'a': tanK['a'][:1], 'b': tan['b']})
    want = emulator.engine.jvp(X, np.stack([np.broadcast_to(tanK['a'][:1], (33, 4)), np.broadcast_to(tan['b'][:, None], (33, 4)), np.zeros((33, 4))], axis=-1)).cpu().numpy()
    assert np.array_equal(row['product'], want[:, :, 7])
    zeros = emulator.jvp(params, {})
    assert zeros['curve'].shape == (33, 7) and not zeros['curve'].any() and not zeros['product'].any()
    with pytest.raises(KeyError):
        emulator.jvp(params, {'d': 1.})
    with pytest.raises(ValueError):
        emulator.jvp(params, {'a': np.ones((33, 2)), 'b': np.ones((33, 3))})
    with pytest.raises(ValueError):
        emulator.jvp({'a': 1., 'b': 2.}, tan)
    # keys=: one run of columns per call, the same bits
    for keys, names in (('product', ['product']), (['curve'], ['curve']), (['product', 'curve'], ['curve', 'product']), (['x'], [])):
        got = emulator.jvp(params, tanK, keys=keys)
        assert list(got) == names and all(np.array_equal(got[key], outK[key]) for key in names), keys
    with pytest.raises(KeyError):
        emulator.jvp(params, tan, keys='curves')
    # return_value=True: predict's dictionary first
    for keys in (None, 'product', ['x', 'curve']):
        values, got = emulator.jvp(params, tanK, keys=keys, return_value=True)
        want = emulator.predict(params, keys=keys)
        assert list(sorted(values)) == list(sorted(want)) and all(np.array_equal(values[key], want[key]) for key in want), keys
        assert all(np.array_equal(got[key], outK[key]) for key in got) and set(got) == set(want) - {'x'}
    values, got = emulator.jvp(point, {'b': 1.}, return_value=True)
    assert values['curve'].shape == (7,) and np.array_equal(values['curve'], emulator.predict(point)['curve']) and got['product'].shape == ()


def test_keys_call_the_engine_once_per_run(emulators):
    """``keys=`` plans the columns with ``column_runs``: one engine call per maximal run, on that range only; a section prefix takes its keys."""
    from cosmoprimo_amd.emulators import Emulator
    emulator = emulators['taylor']
    engine, calls = emulator.engine, []

    class Spy(object):
        name = engine.name
        _dev = engine._dev
        device = engine.device

        def jvp(self, X, tangents, columns=None, return_value=False):
            calls.append(columns)
            return engine.jvp(X, tangents, columns=columns, return_value=return_value)

    emulator.engine = Spy()
    try:
        emulator.jvp(batch(), directions(33), keys='product')
        emulator.jvp(batch(), directions(33, K=2), keys=['curve', 'product'])
        emulator.jvp(batch(), directions(33))
    finally:
        emulator.engine = engine
    assert calls == [(7, 8), (0, 8), None]
    sections = Emulator.__new__(Emulator)      # the same engine under the keys of two sections with an output between them
    sections.params, sections.engine, sections.fixed = emulator.params, Spy(), {}
    sections.varied_keys, sections.varied_shapes = ['fourier.a', 'background.b', 'fourier.c', 'fourier.d'], [(2,), (3,), (2,), ()]
    del calls[:]
    out = sections.jvp(batch(), directions(33, K=2), keys='fourier')
    assert calls == [(0, 2), (5, 8)] and list(out) == ['fourier.a', 'fourier.c', 'fourier.d'] and out['fourier.c'].shape == (33, 2, 2) and out['fourier.d'].shape == (33, 2)
    full = emulator.jvp(batch(), directions(33, K=2))
    assert np.array_equal(out['fourier.c'], full['curve'][:, :, 5:7]) and np.array_equal(out['fourier.d'], full['product'])


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_views_without_read_back(emulators, which):
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}
    tan = {name: torch.as_tensor(v, device=dev) for name, v in directions(17, K=3).items()}

    def fn():
        out = emulator.jvp({name: v[:] for name, v in static.items()}, tan, device=True)
        assert out['curve'].shape == (17, 3, 7) and out['product'].shape == (17, 3) and out['curve'].is_cuda
        assert out['curve'].data_ptr() + 7 * 8 == out['product'].data_ptr()      # views of one (B, K, 8) buffer
        values, out2 = emulator.jvp({name: v[:] for name, v in static.items()}, {'a': tan['a'][:, 0]}, device=True, keys='product', return_value=True)
        assert values['product'].shape == (17,) and values['product'].is_cuda and out2['product'].shape == (17,)
        return torch.cat([out['curve'].reshape(17, -1), out['product'], out2['product'][:, None], values['product'][:, None]], dim=1)

    capture_and_compare(torch, fn, static, fresh)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_against_the_contracted_jacobian(emulators, golden, which):
    """Emulator.jvp against the tangents contracted with Emulator.jacobian: both lie within the rule of their own truth -- the longdouble passes of
    tests/jacobian_reference.py on the engine's state, contracted in longdouble for the jvp --, so each is checked against it, and their distance is within
    the sum of the two allowances (the Jacobian's, 16 x its level per (parameter, column) block, carried through the contraction)."""
    emulator = emulators[which]
    engine = emulator.engine
    params, tanK = batch(65, seed=4), directions(65, K=4, seed=6)
    X, tan = np.column_stack([params[name] for name in NAMES]), np.stack([tanK[name] for name in NAMES], axis=-1)
    if which == 'taylor':
        args = (engine.center, engine.powers, engine.derivatives, X)
        J_ld, J_64 = jr.taylor_jacobian(*args, dtype=jr.LD), jr.taylor_jacobian(*args, dtype='f8')
    else:
        cfg = mr.golden_config(golden('mlp'), 0)
        args = (cfg['packed'], cfg['dims'], cfg['activations'], X, cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])
        J_ld, J_64 = jr.mlp_jacobian(*args, dtype=jr.LD)[1], jr.mlp_jacobian(*args, dtype='f8')[1]
    out_ld, out_64 = pr.jvp(J_ld, tan, jr.LD), pr.jvp(J_64, tan, 'f8')
    out = emulator.jvp(params, tanK)
    got = np.concatenate([out['curve'], out['product'][:, :, None]], axis=2)
    jr.assert_within(got, out_ld, out_64, '%s emulator' % which)
    J = emulator.jacobian(params)
    J = np.concatenate([J['curve'], J['product'][:, :, None]], axis=2)
    contracted = np.einsum('bki,bic->bkc', tan, J)
    top, level = jr.levels(out_ld, out_64)
    jtop, jlevel = jr.levels(J_ld, J_64)
    allowed = jr.ALLOW * level * top + np.einsum('bki,ic->bkc', np.abs(tan), jr.ALLOW * jlevel * jtop).max(axis=0) + 3 * 2.**-53 * pr.jvp(np.abs(J), np.abs(tan), 'f8').max(axis=0)
    assert (np.abs(got - contracted).max(axis=0) <= allowed).all()
