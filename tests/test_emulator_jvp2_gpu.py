"""GPU: Emulator.jvp2 and Emulator.hessian on the toy calculator of tests/mlp_reference.py (3 parameters; 'curve' of 7 values and the scalar 'product' vary,
'x' is fixed), with the emulators of tests/test_emulator_jacobian_gpu.py: a Taylor emulator of order 3 fitted here, and an MLP loaded from a golden
configuration (no training).  Shapes and key order for scalar, array and 2-D (K pairs) tangents, ``keys=`` with one engine call per run,
``return_value`` against ``predict`` and ``return_first`` against ``jvp``, bit for bit; ``Emulator.jvp2`` bit-equal to the engine call on the same X;
``hessian`` bit-equal to ``jvp2`` on unit pairs and symmetric bit for bit; ``device=True`` as views without a read-back (the call is recorded into a HIP
graph, the approach of tests/test_no_host_sync_gpu.py)."""
import numpy as np
import pytest

from test_emulator_jacobian_gpu import NAMES, batch, emulators      # noqa: F401 (the fixture)
from test_emulator_jvp_gpu import directions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_shapes_keys_and_values(emulators, which):
    import torch
    emulator = emulators[which]
    params = batch()
    X = np.column_stack([params[name] for name in NAMES])
    stack = lambda tan: np.stack([tan[name] for name in NAMES], axis=-1)      # noqa: E731 (the components in the order of Emulator.params)
    tan, tan2 = directions(33), directions(33, seed=8)
    out = emulator.jvp2(params, tan, tan2)
    assert list(out) == ['curve', 'product'] and out['curve'].shape == (33, 7) and out['product'].shape == (33,)      # no fixed output: its derivatives are zero
    assert all(isinstance(value, np.ndarray) for value in out.values())
    full = emulator.engine.jvp2(X, stack(tan), stack(tan2)).cpu().numpy()
    assert np.array_equal(out['curve'], full[:, :7]) and np.array_equal(out['product'], full[:, 7])
    swapped = emulator.jvp2(params, tan2, tan)
    assert all(np.array_equal(swapped[key], out[key]) for key in out)
    tanK, tanK2 = directions(33, K=4), directions(33, K=4, seed=8)
    outK = emulator.jvp2(params, tanK, tanK2)
    assert list(outK) == ['curve', 'product'] and outK['curve'].shape == (33, 4, 7) and outK['product'].shape == (33, 4)
    fullK = emulator.engine.jvp2(X, stack(tanK), stack(tanK2)).cpu().numpy()
    assert np.array_equal(outK['curve'], fullK[:, :, :7]) and np.array_equal(outK['product'], fullK[:, :, 7])
    sameK = emulator.jvp2(params, tanK)      # the second directional derivative
    fullsame = emulator.engine.jvp2(X, stack(tanK)).cpu().numpy()
    assert np.array_equal(sameK['curve'], fullsame[:, :, :7]) and np.array_equal(sameK['product'], fullsame[:, :, 7])
    assert np.array_equal(emulator.jvp2(params, tanK, tanK)['curve'], sameK['curve'])
    one = emulator.jvp2(params, {name: tanK[name][:, 2] for name in NAMES}, {name: tanK2[name][:, 2] for name in NAMES})      # a pair of the K alone: the same bits
    assert np.array_equal(one['curve'], outK['curve'][:, 2]) and np.array_equal(one['product'], outK['product'][:, 2])
    point = {name: float(params[name][5]) for name in NAMES}
    outp = emulator.jvp2(point, {name: float(tan[name][5]) for name in NAMES}, {name: float(tan2[name][5]) for name in NAMES})
    assert outp['curve'].shape == (7,) and outp['product'].shape == ()
    assert np.array_equal(outp['curve'], out['curve'][5]) and np.array_equal(outp['product'], out['product'][5])
    outp = emulator.jvp2(point, {name: tanK[name][5:6] for name in NAMES})
    assert outp['curve'].shape == (4, 7) and np.array_equal(outp['curve'], sameK['curve'][5])
    # a missing name is a zero component, a scalar broadcasts; host and device tangents together
    mixed = emulator.jvp2(params, {'a': tanK['a'], 'c': 0.5}, {'b': tanK2['b']})
    want = emulator.engine.jvp2(X, np.stack([tanK['a'], np.zeros((33, 4)), np.full((33, 4), 0.5)], axis=-1),
                                np.stack([np.zeros((33, 4)), tanK2['b'], np.zeros((33, 4))], axis=-1)).cpu().numpy()
    assert np.array_equal(mixed['curve'], want[:, :, :7]) and np.array_equal(mixed['product'], want[:, :, 7])
    mixed_dev = emulator.jvp2(params, {'a': torch.as_tensor(tanK['a'], device='cuda:0'), 'c': 0.5}, {'b': tanK2['b']})
    assert np.array_equal(mixed_dev['curve'], mixed['curve'])
    zeros = emulator.jvp2(params, tan, {})
    assert zeros['curve'].shape == (33, 7) and not zeros['curve'].any() and not zeros['product'].any()
    for bad in (({'d': 1.}, None), (tan, {'d': 1.})):      # unknown names raise as in jvp, in either set
        with pytest.raises(KeyError):
            emulator.jvp2(params, *bad)
    with pytest.raises(ValueError):
        emulator.jvp2(params, {'a': np.ones((33, 2))}, {'b': np.ones((33, 3))})
    with pytest.raises(ValueError):
        emulator.jvp2({'a': 1., 'b': 2.}, tan)
    # keys=: one run of columns per call, the same bits
    for keys, names in (('product', ['product']), (['curve'], ['curve']), (['product', 'curve'], ['curve', 'product']), (['x'], [])):
        got = emulator.jvp2(params, tanK, tanK2, keys=keys)
        assert list(got) == names and all(np.array_equal(got[key], outK[key]) for key in names), keys
    with pytest.raises(KeyError):
        emulator.jvp2(params, tan, keys='curves')
    # return_value=True: predict's dictionary first; return_first=True: jvp's dictionaries next
    for keys in (None, 'product', ['x', 'curve']):
        values, first_u, first_v, got = emulator.jvp2(params, tanK, tanK2, keys=keys, return_value=True, return_first=True)
        want = emulator.predict(params, keys=keys)
        assert list(sorted(values)) == list(sorted(want)) and all(np.array_equal(values[key], want[key]) for key in want), keys
        assert all(np.array_equal(got[key], outK[key]) for key in got) and set(got) == set(want) - {'x'}
        for first, t in ((first_u, tanK), (first_v, tanK2)):
            want_first = emulator.jvp(params, t, keys=keys)
            assert list(first) == list(want_first) and all(np.array_equal(first[key], want_first[key]) for key in first), keys
    first_u, got = emulator.jvp2(point, {'b': 1.}, return_first=True)
    assert got['product'].shape == () and np.array_equal(first_u['curve'], emulator.jvp(point, {'b': 1.})['curve'])
    values, got = emulator.jvp2(point, {'b': 1.}, return_value=True)
    assert values['curve'].shape == (7,) and np.array_equal(values['curve'], emulator.predict(point)['curve'])


def test_keys_call_the_engine_once_per_run(emulators):
    """``keys=`` plans the columns with ``column_runs``: one engine call per maximal run, on that range only."""
    emulator = emulators['taylor']
    engine, calls = emulator.engine, []

    class Spy(object):
        name = engine.name
        _dev = engine._dev
        device = engine.device

        def jvp2(self, X, tangents, tangents2=None, columns=None, return_value=False, return_first=False):
            calls.append(columns)
            return engine.jvp2(X, tangents, tangents2, columns=columns, return_value=return_value, return_first=return_first)

    emulator.engine = Spy()
    try:
        emulator.jvp2(batch(), directions(33), keys='product')
        emulator.jvp2(batch(), directions(33, K=2), directions(33, K=2, seed=8), keys=['curve', 'product'])
        emulator.jvp2(batch(), directions(33))
        emulator.hessian(batch(), keys='product')
        emulator.hessian(batch())
    finally:
        emulator.engine = engine
    assert calls == [(7, 8), (0, 8), None, (7, 8), None]


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_hessian(emulators, which):
    """``hessian``: one jvp2 call on the unit pairs i <= j, mirrored -- bit-equal to jvp2 on each unit pair and symmetric bit for bit."""
    emulator = emulators[which]
    params = batch()
    H = emulator.hessian(params)
    assert list(H) == ['curve', 'product'] and H['curve'].shape == (33, 3, 3, 7) and H['product'].shape == (33, 3, 3)
    for key, block in H.items():
        assert np.array_equal(block, np.swapaxes(block, 1, 2)), key
    for i, first in enumerate(NAMES):
        for j, second in enumerate(NAMES):
            pair = emulator.jvp2(params, {first: 1.}, {second: 1.})
            assert np.array_equal(pair['curve'], H['curve'][:, i, j]) and np.array_equal(pair['product'], H['product'][:, i, j]), (first, second)
    diagonal = emulator.jvp2(params, {NAMES[1]: 1.})      # v absent: the same bits as the unit pair (1, 1)
    assert np.array_equal(diagonal['curve'], H['curve'][:, 1, 1])
    point = {name: float(params[name][5]) for name in NAMES}
    Hp = emulator.hessian(point)
    assert Hp['curve'].shape == (3, 3, 7) and Hp['product'].shape == (3, 3)
    assert np.array_equal(Hp['curve'], H['curve'][5]) and np.array_equal(Hp['product'], H['product'][5])
    Hk = emulator.hessian(params, keys='product')
    assert list(Hk) == ['product'] and np.array_equal(Hk['product'], H['product'])
    assert emulator.hessian(params, keys=['x']) == {}
    with pytest.raises(KeyError):
        emulator.hessian(params, keys='curves')


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_views_without_read_back(emulators, which):
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}
    tan, tan2 = ({name: torch.as_tensor(v, device=dev) for name, v in directions(17, K=3, seed=seed).items()} for seed in (5, 8))

    def fn():
        out = emulator.jvp2({name: v[:] for name, v in static.items()}, tan, tan2, device=True)
        assert out['curve'].shape == (17, 3, 7) and out['product'].shape == (17, 3) and out['curve'].is_cuda
        assert out['curve'].data_ptr() + 7 * 8 == out['product'].data_ptr()      # views of one (B, K, 8) buffer
        values, first, out2 = emulator.jvp2({name: v[:] for name, v in static.items()}, {'a': tan['a'][:, 0]}, device=True, keys='product', return_value=True, return_first=True)
        assert values['product'].shape == (17,) and values['product'].is_cuda and out2['product'].shape == (17,) and first['product'].shape == (17,)
        return torch.cat([out['curve'].reshape(17, -1), out['product'], out2['product'][:, None], first['product'][:, None], values['product'][:, None]], dim=1)

    capture_and_compare(torch, fn, static, fresh)
