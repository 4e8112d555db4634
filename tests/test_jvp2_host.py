"""CPU: (a) the level of the tolerance rule, at most 32 floors for every shape the device tests use, with v = u and with the second tangent set, which keeps
the rule meaningful (a case above it was redrawn by its seed, tests/jvp2_reference.py; the cap stays); (b) the longdouble truth of
tests/jvp2_reference.py against central differences of the longdouble first-order Jacobian of tests/jacobian_reference.py along the second direction,
contracted with the first -- a check of the formulas, not of rounding: step and bound are derived from the longdouble epsilon below and printed;
(c) the argument checks of cp_mlp_jvp2 and cp_taylor_jvp2 against tests/golden/jvp2_abi_errors.json (tools/gen_jvp2_abi_errors.py holds the table of
calls and wrote the file): status and message of every refusal, each before any device call (this test runs without a device); (d) the key handling of
Emulator.jvp2 and Emulator.hessian on a stub engine.

Central differences.  With eps the longdouble epsilon and a step of h along v (v of the order of the parameters' scales), [J(x + h v) - J(x - h v)] / 2 h
differs from the derivative by the truncation h^2 / 6 |D^3| and by the rounding eps |J| / h; h = eps^(1/3) balances them at eps^(2/3) (2.3e-13 with the
64-bit significand of x86).  The third derivatives of these small networks and polynomials (weights of variance 1 / n_in, powers up to 15 of |x - c| < 1.5)
are allowed 1000 times the size of the second ones, the block's largest entry: the bound is 1000 eps^(2/3) of that, 2.3e-10.  A wrong formula is off by
the order of the entry itself."""
import json
import os

import numpy as np
import pytest

import jacobian_reference as jr
import jvp_reference as pr
import jvp2_reference as sr
import mlp_reference as mr
from test_emulator_abi_errors_host import call, comes_back_early

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
STEP, BOUND = EPS**(1. / 3.), 1000. * EPS**(2. / 3.)
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jvp2_abi_errors.json')
ENTRIES = ['cp_mlp_jvp2', 'cp_taylor_jvp2']


@pytest.mark.parametrize('options', sr.MLP_CASES + sr.MLP_RANGE_CASES, ids=[sr.case_id(case) for case in sr.MLP_CASES + sr.MLP_RANGE_CASES])
def test_mlp_level(options):
    cfg = sr.mlp_config(**options)
    for mixed in (False, True):
        out_ld, out_64 = sr.mlp_truth(cfg, mixed)
        assert out_ld.dtype == LD and out_ld.shape == cfg['tan'].shape[:2] + (cfg['dims'][-1],)
        top, level = jr.levels(out_ld, out_64)
        print('%s, %s: level at most %.3g floors' % (options, 'mixed' if mixed else 'v = u', float(level.max() / jr.FLOOR)))
        assert float(level.max()) <= 32. * jr.FLOOR
        if options.get('activations') == 'relu':
            assert not out_ld.any()      # piecewise linear
        else:
            assert (top > 0).all()


@pytest.mark.parametrize('options', sr.TAYLOR_CASES, ids=[sr.case_id(case) for case in sr.TAYLOR_CASES])
def test_taylor_level(options):
    cfg = sr.taylor_config(**options)
    for mixed in (False, True):
        out_ld, out_64 = sr.taylor_truth(cfg, mixed)
        assert out_ld.dtype == LD and out_ld.shape == cfg['tan'].shape[:2] + (cfg['derivatives'].shape[1],)
        top, level = jr.levels(out_ld, out_64)
        print('%s, %s: level at most %.3g floors' % (options, 'mixed' if mixed else 'v = u', float(level.max() / jr.FLOOR)))
        assert float(level.max()) <= 32. * jr.FLOOR
        if cfg['powers'].shape[0] == 1:      # the constant alone
            assert not out_ld.any()


def test_the_seeds_are_the_first_below_the_cap():
    """A redrawn case names the first seed at which both runs lie below the cap: the draw before it does not (spot check of the two cheapest redraws)."""
    for config, truth, options in ((sr.mlp_config, sr.mlp_truth, dict(K=7, seed=0)), (sr.taylor_config, sr.taylor_truth, dict(B=63, K=1, seed=0))):
        cfg = config(**options)
        assert max(float(jr.levels(*truth(cfg, mixed))[1].max()) for mixed in (False, True)) > 32. * jr.FLOOR


def central(jacobian, X, u, v):
    """(B, K, M): [J(x + h v) - J(x - h v)] / 2 h contracted with u, in longdouble; the step is STEP along each v[b, k]."""
    X, u, v = (np.asarray(a).astype(LD) for a in (X, u, v))
    out = []
    for k in range(u.shape[1]):
        difference = (jacobian(X + LD(STEP) * v[:, k]) - jacobian(X - LD(STEP) * v[:, k])) / (2 * LD(STEP))      # (B, ndim, M)
        out.append(np.einsum('bi,bic->bc', u[:, k], difference))
    return np.stack(out, axis=1)


def against_central_differences(out_ld, fd, what):
    top = np.abs(out_ld).max(axis=0)
    used = float((np.abs(out_ld - fd).max(axis=0) / top).max())
    print('%s: longdouble eps %.3g, step %.3g, bound %.3g of the block; largest distance from the central differences %.3g' % (what, EPS, STEP, BOUND, used))
    assert used <= BOUND


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
@pytest.mark.parametrize('activation', [a for a in mr.ACTIVATIONS if a != 'relu'])
def test_mlp_truth_against_central_differences(activation, yfunction):
    cfg = sr.mlp_config(B=16, M=8, K=3, activations=activation, yfunction=yfunction, seed=3)
    args = pr.mlp_args(cfg)
    jacobian = lambda Xp: jr.mlp_jacobian(args[0], args[1], args[2], Xp, *args[4:], dtype=LD)[1]      # noqa: E731
    for mixed in (False, True):
        out_ld = sr.mlp_truth(cfg, mixed)[0]
        fd = central(jacobian, cfg['X'], cfg['tan'], cfg['tan2'] if mixed else cfg['tan'])
        against_central_differences(out_ld, fd, '%s, %s, %s' % (activation, yfunction or 'no y function', 'mixed' if mixed else 'v = u'))


def test_relu_truth_is_zero_under_a_y_function_too_where_it_should_be():
    """relu: without y function exactly 0; with one, the second derivative is f''(v) v_u v_v alone, which the central differences confirm."""
    cfg = sr.mlp_config(B=16, M=8, K=3, activations='relu', yfunction='', seed=3)
    assert not sr.mlp_truth(cfg, True)[0].any()
    cfg = sr.mlp_config(B=16, M=8, K=3, activations='relu', yfunction='arcsinh', seed=3)
    args = pr.mlp_args(cfg)
    out_ld = sr.mlp_truth(cfg, True)[0]
    fd = central(lambda Xp: jr.mlp_jacobian(args[0], args[1], args[2], Xp, *args[4:], dtype=LD)[1], cfg['X'], cfg['tan'], cfg['tan2'])
    against_central_differences(out_ld, fd, 'relu, arcsinh, mixed')


def test_taylor_truth_against_central_differences():
    c = sr.taylor_config(B=16, T=65, M=9, K=3)
    jacobian = lambda Xp: jr.taylor_jacobian(c['center'], c['powers'], c['derivatives'], Xp, dtype=LD)      # noqa: E731
    for mixed in (False, True):
        out_ld = sr.taylor_truth(c, mixed)[0]
        fd = central(jacobian, c['X'], c['tan'], c['tan2'] if mixed else c['tan'])
        against_central_differences(out_ld, fd, 'taylor, %s' % ('mixed' if mixed else 'v = u'))


def test_truth_is_symmetric_and_bilinear():
    """The restatement itself: exchanging u and v changes nothing in longdouble beyond rounding, and (u, v) -> out is linear in v."""
    cfg = sr.mlp_config(B=16, M=8, K=3, activations='tanh', yfunction='log10')
    args = pr.mlp_args(cfg)
    a = sr.mlp_jvp2(*args, cfg['tan'], cfg['tan2'], dtype=LD)
    b = sr.mlp_jvp2(*args, cfg['tan2'], cfg['tan'], dtype=LD)
    c = sr.mlp_jvp2(*args, cfg['tan'], 2 * cfg['tan2'].astype(LD) + cfg['tan'].astype(LD), dtype=LD)      # (the combination formed in longdouble)
    d = sr.mlp_jvp2(*args, cfg['tan'], dtype=LD)
    scale = np.abs(a).max() + np.abs(d).max()
    assert np.abs(a - b).max() <= 64 * EPS * scale and np.abs(c - (2 * a + d)).max() <= 64 * EPS * scale


@pytest.fixture(scope='module')
def cases():
    with open(FIXTURE) as file:
        cases = json.load(file)
    assert sorted({case['entry'] for case in cases}) == sorted(ENTRIES)
    late = [case for case in cases if not comes_back_early(case)]
    assert not late, late      # such a call would launch on fake pointers
    return cases


@pytest.mark.parametrize('entry', ENTRIES)
def test_status_and_message_of_every_refusal(cases, entry):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    mine = [case for case in cases if case['entry'] == entry]
    assert len(mine) >= 30
    wrong = []
    for case in mine:
        status, message = call(lib, entry, case['args'])
        if (status, message) != (case['status'], case['message']):
            wrong.append((case['what'], (status, message), (case['status'], case['message'])))
    assert not wrong, wrong


def test_the_checks_are_those_of_jvp_in_its_order(cases):
    """What the issue of the entry points fixes, read off the fixture: K < 1 is CP_EINVAL, more than 2^37 rows or K > 2^31 - 1 CP_EUNSUPPORTED, B = 0 CP_OK, a
    null pointer CP_EINVAL (d_first_* missing under a y function and d_first_v without d_tan_v included); the range answers before the strides, the strides
    before K, K before the caps, the caps before the null pointers."""
    from cosmoprimo_amd import _lib
    for entry in ENTRIES:
        mine = {case['what']: case for case in cases if case['entry'] == entry}
        assert all(mine['K = %d' % K]['status'] == _lib.CP_EINVAL and 'directions' in mine['K = %d' % K]['message'] for K in (0, -1))
        assert mine['K = 2^31']['status'] == _lib.CP_EUNSUPPORTED and mine['B = 2^62']['status'] == _lib.CP_EUNSUPPORTED
        for K in (1, 3, 64):
            assert mine['one past the grid, K = %d' % K]['status'] == _lib.CP_EUNSUPPORTED and '2^37' in mine['one past the grid, K = %d' % K]['message']
            assert mine['the grid full, every pointer null, K = %d' % K]['status'] == _lib.CP_EINVAL and 'null pointer' in mine['the grid full, every pointer null, K = %d' % K]['message']
        assert mine['B = 0, every pointer null']['status'] == _lib.CP_OK
        assert all(case['status'] == _lib.CP_EINVAL and 'null pointer' in case['message'] and entry in case['message'] for what, case in mine.items() if what.startswith('null d_'))
        assert 'columns' in mine['a bad range, a short stride and K = 0']['message'] and 'row stride' in mine['a short stride and K = 0']['message']
        assert 'directions' in mine['K = 0 and one past the grid']['message'] and 'directions' in mine['K = 0 and a null pointer']['message']
    mlp = {case['what']: case for case in cases if case['entry'] == 'cp_mlp_jvp2'}
    for what in ('d_first_v without d_tan_v', 'd_first_v without d_tan_v, y function', 'y function 1 without d_first_u', 'y function 2, d_tan_v without d_first_v',
                 'y function 1 without both', 'y function 2 without both'):
        assert mlp[what]['status'] == _lib.CP_EINVAL and 'null pointer' in mlp[what]['message'], what
    assert 'value' in mlp['ldv and ldf short']['message'] and 'first-order' in mlp['ldf and ldo short']['message']
    assert mlp['ldf one short, no first-order products, no y function: B = 0']['status'] == _lib.CP_OK
    assert 'first-order' in mlp['ldf one short, no first-order products, y function']['message']


class StubEngine(object):
    """What Emulator.jvp2 uses of an engine: the result is the product of the two tangents' sums, in every column."""
    name, device, _dev = 'stub', None, {'device': None}

    def __init__(self):
        self.calls = []

    def jvp2(self, X, tangents, tangents2=None, columns=None, return_value=False, return_first=False):
        self.calls.append((np.asarray(X), np.asarray(tangents), None if tangents2 is None else np.asarray(tangents2), columns))
        M = 8 if columns is None else columns[1] - columns[0]
        wide = lambda a: np.repeat(np.asarray(a)[..., None], M, axis=-1)      # noqa: E731
        u = np.asarray(tangents).sum(axis=-1)
        v = u if tangents2 is None else np.asarray(tangents2).sum(axis=-1)
        toret = ([np.zeros((len(X), M))] if return_value else []) + ([wide(u)] + ([] if tangents2 is None else [wide(v)]) if return_first else []) + [wide(u * v)]
        return tuple(toret) if len(toret) > 1 else toret[0]


def stub_emulator():
    from cosmoprimo_amd.emulators import Emulator
    emulator = Emulator(None, params={'a': (0., 1.), 'b': (0., 1.), 'c': (0., 1.)}, engine=StubEngine())
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['curve', 'product'], [(7,), ()], {'x': np.arange(3.)}
    return emulator


def test_emulator_keys_on_a_stub_engine():
    emulator = stub_emulator()
    engine = emulator.engine
    params = {'a': np.linspace(0., 1., 5), 'b': 0.5, 'c': np.linspace(1., 0., 5)}
    for bad in (({'a': 1., 'd': 1.}, None), ({'a': 1.}, {'d': 1.})):      # a name that is no parameter, in either set
        with pytest.raises(KeyError):
            emulator.jvp2(params, *bad)
    assert not engine.calls
    out = emulator.jvp2(params, {'b': 2.})      # missing names are zero components; no second set: None reaches the engine
    X, T, T2, columns = engine.calls.pop()
    assert columns is None and T2 is None and X.shape == (5, 3) and T.shape == (5, 3) and np.array_equal(T, np.tile([0., 2., 0.], (5, 1)))
    assert list(out) == ['curve', 'product'] and out['curve'].shape == (5, 7) and out['product'].shape == (5,) and (out['product'] == 4.).all()
    out = emulator.jvp2(params, {'a': np.arange(5.), 'b': np.arange(20.).reshape(5, 4)}, {'c': np.ones((1, 4))}, keys='product')
    X, T, T2, columns = engine.calls.pop()
    assert columns == (7, 8) and T.shape == (5, 4, 3) and T2.shape == (5, 4, 3) and list(out) == ['product'] and out['product'].shape == (5, 4)
    assert np.array_equal(T2, np.tile([0., 0., 1.], (5, 4, 1))) and np.array_equal(out['product'], T.sum(axis=-1))
    with pytest.raises(ValueError):      # the two sets do not share K
        emulator.jvp2(params, {'a': np.ones((5, 2))}, {'b': np.ones((5, 3))})
    with pytest.raises(ValueError):
        emulator.jvp2(params, {'a': np.ones((5, 2))}, {'b': 1.})
    point = {'a': 0.1, 'b': 0.2, 'c': 0.3}      # scalar parameters: no leading axis
    out = emulator.jvp2(point, {'a': 1.}, {'b': 3.})
    assert out['curve'].shape == (7,) and out['product'].shape == () and out['product'] == 3.
    values, first_u, first_v, out = emulator.jvp2(params, {'a': 1.}, {'c': 2.}, keys=['x', 'curve'], return_value=True, return_first=True)
    assert list(values) == ['curve', 'x'] and list(out) == ['curve'] and list(first_u) == ['curve'] and engine.calls.pop()[3] == (0, 7)
    assert (first_u['curve'] == 1.).all() and (first_v['curve'] == 2.).all() and (out['curve'] == 2.).all()
    first_u, out = emulator.jvp2(params, {'a': 3.}, return_first=True)
    assert (first_u['product'] == 3.).all() and (out['product'] == 9.).all()
    # hessian: one call on the ndim (ndim + 1) / 2 unit pairs i <= j, mirrored
    del engine.calls[:]
    H = emulator.hessian(params)
    X, T, T2, columns = engine.calls.pop()
    assert not engine.calls and T.shape == (5, 6, 3) and T2.shape == (5, 6, 3) and columns is None
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    assert all(np.array_equal(T[b, p], np.eye(3)[i]) and np.array_equal(T2[b, p], np.eye(3)[j]) for b in range(5) for p, (i, j) in enumerate(pairs))
    assert list(H) == ['curve', 'product'] and H['curve'].shape == (5, 3, 3, 7) and H['product'].shape == (5, 3, 3) and (H['product'] == 1.).all()
    H = emulator.hessian(point, keys='curve')
    assert list(H) == ['curve'] and H['curve'].shape == (3, 3, 7) and engine.calls.pop()[3] == (0, 7)
