"""GPU: Emulator.vjp on the toy calculator of tests/test_emulator_jacobian_gpu.py (3 parameters; 'curve' of 7 values and the scalar 'product' vary, 'x' is
fixed): a Taylor emulator of order 3 fitted here, and an MLP loaded from a golden configuration (no training).  Shapes and key order for scalar, array
and mixed host / device parameters, the key cases of ``cotangents`` (a fixed key, an unknown key, an empty dictionary), one engine call per run of
columns, ``device=True`` (views of one buffer, recorded into a HIP graph), ``return_value=True`` against ``predict``, and equality within the rule of
tests/vjp_reference.py with the cotangent contracted with ``Emulator.jacobian``."""
import numpy as np
import pytest

import jacobian_reference as jr
import mlp_reference as mr
import vjp_reference as vr
from test_emulator_jacobian_gpu import NAMES, batch, emulators  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def cotangents(B=33, seed=7):
    rng = np.random.default_rng(seed)
    return {'curve': rng.normal(0., 1., (B, 7)), 'product': rng.normal(0., 1., B)}


def engine_case(emulator, which, golden, X, cot):
    """(G_ld, A, level) of the engine under the emulator for the cotangent (B, 8)."""
    if which == 'taylor':
        engine = emulator.engine
        return vr.taylor_case(dict(center=engine.center, powers=engine.powers, derivatives=engine.derivatives, X=X), cot)
    return vr.mlp_case(dict(mr.golden_config(golden('mlp'), 0), X=X), cot)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_shapes_keys_and_values(emulators, golden, which):  # noqa: F811
    import torch
    emulator = emulators[which]
    params, cot = batch(), cotangents()
    X = np.column_stack([params[name] for name in NAMES])
    G = emulator.vjp(params, cot)
    assert list(G) == NAMES and all(isinstance(g, np.ndarray) and g.shape == (33,) for g in G.values())
    got = np.column_stack([G[name] for name in NAMES])
    full = np.concatenate([cot['curve'], cot['product'][:, None]], axis=1)
    assert np.array_equal(got, emulator.engine.vjp(X, full).cpu().numpy())
    # within the rule of the truth, and of the cotangent contracted with Emulator.jacobian (whose own allowance is added)
    G_ld, A, level = engine_case(emulator, which, golden, X, full)
    vr.assert_within(got, G_ld, A, level, which)
    J = emulator.jacobian(params)
    J = np.concatenate([J['curve'], J['product'][:, :, None]], axis=2)
    if which == 'taylor':
        args = (emulator.engine.center, emulator.engine.powers, emulator.engine.derivatives, X)
        J_ld, J_64 = jr.taylor_jacobian(*args, dtype=jr.LD), jr.taylor_jacobian(*args, dtype='f8')
    else:
        cfg = mr.golden_config(golden('mlp'), 0)
        args = (cfg['packed'], cfg['dims'], cfg['activations'], X, cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])
        J_ld, J_64 = jr.mlp_jacobian(*args, dtype=jr.LD)[1], jr.mlp_jacobian(*args, dtype='f8')[1]
    top, block_level = jr.levels(J_ld, J_64)
    einsum = np.einsum('bc,bic->bi', full, J)
    allowed = vr.ALLOW * level * vr.EPS * A + np.abs(full) @ (jr.ALLOW * block_level * top).T + 8 * vr.EPS * A      # (+ the float64 sum over 8 columns itself)
    assert (np.abs(got - einsum) <= np.asarray(allowed, dtype='f8')).all()
    # scalar parameters: scalars, the cotangent of shape ``shape``
    point = {name: float(params[name][5]) for name in NAMES}
    Gp = emulator.vjp(point, {key: value[5] for key, value in cot.items()})
    assert list(Gp) == NAMES and all(np.ndim(Gp[name]) == 0 and Gp[name] == G[name][5] for name in NAMES)
    # scalars and arrays together, one of them a device tensor, a cotangent on the device, one broadcast over the batch
    mixed = emulator.vjp(dict(params, b=2.), cot)
    assert mixed['a'].shape == (33,)
    mixed_dev = emulator.vjp(dict(params, a=torch.as_tensor(params['a'], device='cuda:0'), b=2.), dict(cot, curve=torch.as_tensor(cot['curve'], device='cuda:0')))
    assert all(np.array_equal(mixed_dev[name], mixed[name]) for name in NAMES)
    shared = emulator.vjp(params, {'curve': cot['curve'][0]})
    assert all(np.array_equal(shared[name], emulator.vjp(params, {'curve': np.tile(cot['curve'][0], (33, 1))})[name]) for name in NAMES)
    # the key cases: a fixed key contributes nothing, an unknown one raises, an empty dictionary gives zeros
    alone = emulator.vjp(params, {'product': cot['product']})
    with_fixed = emulator.vjp(params, {'x': np.ones(7), 'product': cot['product']})
    assert all(np.array_equal(with_fixed[name], alone[name]) for name in NAMES)
    only_fixed = emulator.vjp(params, {'x': np.ones(7)})
    empty = emulator.vjp(params, {})
    for zeros in (only_fixed, empty):
        assert list(zeros) == NAMES and all(g.shape == (33,) and not g.any() for g in zeros.values())
    assert all(np.ndim(g) == 0 and g == 0. for g in emulator.vjp(point, {}).values())
    with pytest.raises(KeyError):
        emulator.vjp(params, {'curves': cot['curve']})
    with pytest.raises(KeyError):
        emulator.vjp(params, {'curv': cot['curve']})      # names, not prefixes
    with pytest.raises(ValueError):
        emulator.vjp({'a': 1., 'b': 2.}, cot)
    # a run of columns is the range of the engine: 'product' alone is columns [7, 8)
    assert np.array_equal(np.column_stack([alone[name] for name in NAMES]), emulator.engine.vjp(X, cot['product'][:, None], columns=(7, 8)).cpu().numpy())
    # return_value=True: predict's dictionary for those keys first
    for keys in (['curve', 'product'], ['product'], ['x', 'curve'], []):
        values, got = emulator.vjp(params, {key: (cot[key] if key in cot else np.ones(7)) for key in keys}, return_value=True)
        want = emulator.predict(params, keys=keys)
        assert list(values) == list(want) and all(np.array_equal(values[key], want[key]) for key in want), keys
        again = emulator.vjp(params, {key: cot[key] for key in keys if key in cot})
        assert all(np.array_equal(got[name], again[name]) for name in NAMES)
    values, got = emulator.vjp(point, {'curve': cot['curve'][5]}, return_value=True)
    assert values['curve'].shape == (7,) and np.array_equal(values['curve'], emulator.predict(point)['curve']) and np.ndim(got['a']) == 0


def test_one_engine_call_per_run(emulators):  # noqa: F811
    """The columns are planned with ``column_runs`` over the cotangents' varied keys: one engine call per maximal run, on that range only, added in run order."""
    from cosmoprimo_amd.emulators import Emulator
    emulator = emulators['taylor']
    engine, calls = emulator.engine, []

    class Spy(object):
        name = engine.name
        _dev = engine._dev
        device = engine.device

        def vjp(self, X, cotangent, columns=None, return_value=False):
            calls.append((columns, tuple(cotangent.shape)))
            return engine.vjp(X, cotangent, columns=columns, return_value=return_value)

    params, cot = batch(), cotangents()
    emulator.engine = Spy()
    try:
        emulator.vjp(params, {'product': cot['product']})
        emulator.vjp(params, {'product': cot['product'], 'curve': cot['curve'], 'x': 1.})
        emulator.vjp(params, {'x': 1.})
    finally:
        emulator.engine = engine
    assert calls == [((7, 8), (33, 1)), ((0, 8), (33, 8))]
    # two runs: the same engine under three varied keys, the middle one left out
    split = Emulator.__new__(Emulator)
    split.calculator, split.samples, split.params, split.fixed = None, None, dict(emulator.params), {}
    split.varied_keys, split.varied_shapes = ['head', 'middle', 'tail'], [(3,), (2, 2), ()]
    calls.clear()
    split.engine = Spy()
    rng = np.random.default_rng(9)
    head, tail = rng.normal(0., 1., (33, 3)), rng.normal(0., 1., 33)
    G = split.vjp(params, {'tail': tail, 'head': head})
    assert calls == [((0, 3), (33, 3)), ((7, 8), (33, 1))]
    X = np.column_stack([params[name] for name in NAMES])
    want = engine.vjp(X, head, columns=(0, 3)) + engine.vjp(X, tail[:, None], columns=(7, 8))
    assert np.array_equal(np.column_stack([G[name] for name in NAMES]), want.cpu().numpy())
    values, G2 = split.vjp(params, {'tail': tail, 'head': head}, return_value=True)
    assert list(values) == ['head', 'tail'] and values['head'].shape == (33, 3) and values['tail'].shape == (33,)
    assert np.array_equal(values['tail'], engine.predict(X, columns=(7, 8)).cpu().numpy()[:, 0])


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_device_views_without_read_back(emulators, which):  # noqa: F811
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    static = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=2).items()}
    fresh = {name: torch.as_tensor(v, device=dev) for name, v in batch(17, seed=3).items()}
    for source, seed in ((static, 4), (fresh, 5)):      # the cotangents are inputs of the graph as the parameters are
        source.update({'cot_' + key: torch.as_tensor(v, device=dev) for key, v in cotangents(17, seed=seed).items()})

    def fn():
        params = {name: static[name][:] for name in NAMES}
        G = emulator.vjp(params, {'curve': static['cot_curve'], 'product': static['cot_product']}, device=True)
        assert list(G) == NAMES and all(g.shape == (17,) and g.is_cuda for g in G.values())
        assert all(G[name].data_ptr() == G['a'].data_ptr() + 8 * i and G[name].stride(0) == 3 for i, name in enumerate(NAMES))      # views of one (B, 3) buffer
        values, G2 = emulator.vjp(params, {'product': static['cot_product']}, device=True, return_value=True)
        assert values['product'].shape == (17,) and values['product'].is_cuda and G2['c'].shape == (17,)
        return torch.stack([G[name] for name in NAMES] + [G2[name] for name in NAMES] + [values['product']], dim=1)

    capture_and_compare(torch, fn, static, fresh)
