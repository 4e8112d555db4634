"""CPU: (a) the truth of tests/jvp_reference.py -- the longdouble tangent contracted with the longdouble forward-mode Jacobian of
tests/jacobian_reference.py -- against central differences of the longdouble prediction along the direction (the step and tolerance of
tests/test_vjp_host.py: 2^-20 of each parameter's scale, 1e-8 of the entry's magnitude, the magnitude being sum_i |tan_i| |J_i|), for every activation and
y function and for Taylor; (b) the level of the tolerance rule, at most 32 for every shape the device tests use, which keeps the rule meaningful (a seed
whose components cancel over a whole block would be redrawn, the cap stays); (c) the argument checks of cp_mlp_jvp and cp_taylor_jvp, which come back
before any device call (this test runs without a device); (d) the key handling of Emulator.jvp on a stub engine."""
import ctypes

import numpy as np
import pytest

import jacobian_reference as jr
import jvp_reference as pr
import mlp_reference as mr
from test_jacobian_host import central_differences

LD = np.longdouble


@pytest.mark.parametrize('options', pr.MLP_CASES, ids=[pr.case_id(case) for case in pr.MLP_CASES])
def test_mlp_level(options):
    cfg = pr.mlp_config(**options)
    out_ld, out_64 = pr.mlp_truth(cfg)
    assert out_ld.dtype == LD and out_ld.shape == cfg['tan'].shape[:2] + (cfg['dims'][-1],)
    top, level = jr.levels(out_ld, out_64)
    print('%s: level at most %.3g' % (options, float(level.max() / jr.FLOOR)))
    assert (top > 0).all() and float(level.max()) <= 32. * jr.FLOOR


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_mlp_level_of_the_other_tests(yfunction):
    """The configurations of the column ranges, the identity tangents, the duality with vjp and the NaN contract of tests/test_mlp_jvp_gpu.py."""
    for options in (dict(yfunction=yfunction, activations='tanh'), dict(yfunction=yfunction, K=3), dict(B=22, K=3, yfunction=yfunction)):
        top, level = jr.levels(*pr.mlp_truth(pr.mlp_config(**options)))
        assert float(level.max()) <= 32. * jr.FLOOR, options


@pytest.mark.parametrize('options', pr.TAYLOR_CASES, ids=[pr.case_id(case) for case in pr.TAYLOR_CASES])
def test_taylor_level(options):
    cfg = pr.taylor_config(**options)
    out_ld, out_64 = pr.taylor_truth(cfg)
    assert out_ld.dtype == LD and out_ld.shape == cfg['tan'].shape[:2] + (cfg['derivatives'].shape[1],)
    top, level = jr.levels(out_ld, out_64)
    print('%s: level at most %.3g' % (options, float(level.max() / jr.FLOOR)))
    assert float(level.max()) <= 32. * jr.FLOOR
    if cfg['powers'].shape[0] == 1:      # the constant alone
        assert not out_ld.any()


def along(f, X, tan, scale):
    """Central differences of f along each direction: (B, K, M), the step 2^-20 of each parameter's scale (that of ``central_differences``, per unit
    tangent: the tangents are of the order of the scales)."""
    fd = central_differences(f, X, scale)      # (B, ndim, M)
    return pr.jvp(fd, tan, LD)


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
@pytest.mark.parametrize('activation', mr.ACTIVATIONS)
def test_mlp_truth_against_central_differences(activation, yfunction):
    cfg = pr.mlp_config(B=16, M=8, K=3, activations=activation, yfunction=yfunction, seed=3)
    args = pr.mlp_args(cfg)
    J = jr.mlp_jacobian(*args, dtype=LD)[1]
    out_ld = pr.jvp(J, cfg['tan'], LD)
    magnitude = pr.jvp(np.abs(J), np.abs(cfg['tan']), LD)
    fd = along(lambda Xp: mr.predict(args[0], args[1], args[2], Xp, *args[4:], dtype=LD), cfg['X'], cfg['tan'], cfg['xscale'])
    used = float((np.abs(out_ld - fd) / magnitude).max())
    print('%s, %s: largest distance from the central differences %.3g of the magnitude' % (activation, yfunction or 'no y function', used))
    assert used <= 1e-8


def test_taylor_truth_against_central_differences():
    c = pr.taylor_config(B=16, T=65, M=9, K=3)
    J = jr.taylor_jacobian(c['center'], c['powers'], c['derivatives'], c['X'], dtype=LD)
    out_ld = pr.jvp(J, c['tan'], LD)
    magnitude = pr.jvp(np.abs(J), np.abs(c['tan']), LD)
    fd = along(lambda Xp: jr.taylor_predict(c['center'], c['powers'], c['derivatives'], Xp, dtype=LD), c['X'], c['tan'], np.ones(3))
    used = float((np.abs(out_ld - fd) / magnitude).max())
    print('taylor: largest distance from the central differences %.3g of the magnitude' % used)
    assert used <= 1e-8


FAKE = ctypes.c_void_p(8)      # a non-null pointer nobody reads: every call here returns before its first device call


def mlp_call(B=4, ndim=3, widths=(5, 17), M=8, col0=0, ncols=8, K=2, ldv=8, ldo=8, pointers=None, yfunction=0):
    from cosmoprimo_amd import _lib
    L = len(widths)
    p = [FAKE] * 9 if pointers is None else pointers      # d_x, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, d_tan, d_value, d_out
    return _lib.load().cp_mlp_jvp(p[0], B, ndim, L, (ctypes.c_int * L)(*widths), (ctypes.c_int * L)(*([0] * L)), M, p[1], p[2], p[3], p[4], p[5], yfunction, col0, ncols,
                                  p[6], K, p[7], ldv, p[8], ldo, 0, None)


def taylor_call(B=4, ndim=3, T=20, max_power=3, M=8, col0=0, ncols=8, K=2, ldo=8, pointers=None):
    from cosmoprimo_amd import _lib
    p = [FAKE] * 6 if pointers is None else pointers      # d_x, d_center, d_powers, d_derivatives, d_tan, d_out
    return _lib.load().cp_taylor_jvp(p[0], B, p[1], p[2], ndim, T, max_power, p[3], M, col0, ncols, p[4], K, p[5], ldo, 0, None)


@pytest.mark.parametrize('call,npointers', [(mlp_call, 9), (taylor_call, 6)], ids=['mlp', 'taylor'])
def test_argument_checks_come_before_any_device_call(call, npointers):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    for k in range(npointers):      # each null pointer
        assert call(pointers=[None if j == k else FAKE for j in range(npointers)]) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert call(ldo=7) == _lib.CP_EINVAL and b'row stride' in lib.cp_last_error()
    for K in (0, -1):
        assert call(K=K) == _lib.CP_EINVAL and b'directions' in lib.cp_last_error()
    for col0, ncols in ((-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)):
        assert call(col0=col0, ncols=ncols, ldo=16) == _lib.CP_EINVAL and b'columns' in lib.cp_last_error()
    assert call(B=-1) == _lib.CP_EINVAL
    assert call(B=0) == _lib.CP_OK and call(B=0, pointers=[None] * npointers) == _lib.CP_OK
    assert call(ndim=33) == _lib.CP_EUNSUPPORTED
    # beyond the 2^31 - 1 row tiles of 64 that the grid holds, a row per point and direction: the cap jacobian puts on B ndim; the largest count below is
    # refused only for its null pointers
    for K in (1, 3, 64):
        most = (2**31 - 1) * 64 // K
        assert call(B=most + 1, K=K) == _lib.CP_EUNSUPPORTED and b'2^37' in lib.cp_last_error()
        assert call(B=most, K=K, pointers=[None] * npointers) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert call(B=2**62) == _lib.CP_EUNSUPPORTED and call(B=1, K=2**31) == _lib.CP_EUNSUPPORTED
    with pytest.raises(NotImplementedError):
        _lib.check(call(B=(2**31 - 1) * 64 // 2 + 1))


def test_argument_checks_of_the_network_and_the_polynomial():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    assert mlp_call(widths=(5, 65)) == _lib.CP_EUNSUPPORTED and b'width 65' in lib.cp_last_error()
    assert mlp_call(widths=(5, 0)) == _lib.CP_EINVAL
    assert mlp_call(widths=(8,) * 9) == _lib.CP_EUNSUPPORTED
    assert mlp_call(yfunction=3) == _lib.CP_EINVAL
    assert mlp_call(ldv=7) == _lib.CP_EINVAL and b'row stride' in lib.cp_last_error() and b'cp_mlp_jvp' in lib.cp_last_error()
    assert taylor_call(max_power=16) == _lib.CP_EUNSUPPORTED and b'cp_taylor_jvp' in lib.cp_last_error()
    assert taylor_call(max_power=-1) == _lib.CP_EINVAL and taylor_call(T=0) == _lib.CP_EINVAL
    # the order of jacobian: the range of columns before the strides, the strides before the caps
    assert mlp_call(ncols=0, ldo=-1, K=0) == _lib.CP_EINVAL and b'columns' in lib.cp_last_error()
    assert taylor_call(ldo=7, ndim=33) == _lib.CP_EINVAL and taylor_call(K=0, ndim=33) == _lib.CP_EUNSUPPORTED


class StubEngine(object):
    """What Emulator.jvp uses of an engine: the result is the tangent it was given, in every column."""
    name, device, _dev = 'stub', None, {'device': None}

    def __init__(self):
        self.calls = []

    def jvp(self, X, tangents, columns=None, return_value=False):
        self.calls.append((np.asarray(X), np.asarray(tangents), columns))
        M = 8 if columns is None else columns[1] - columns[0]
        out = np.repeat(np.asarray(tangents).sum(axis=-1)[..., None], M, axis=-1)
        return (np.zeros((len(X), M)), out) if return_value else out


def stub_emulator():
    from cosmoprimo_amd.emulators import Emulator
    emulator = Emulator(None, params={'a': (0., 1.), 'b': (0., 1.), 'c': (0., 1.)}, engine=StubEngine())
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['curve', 'product'], [(7,), ()], {'x': np.arange(3.)}
    return emulator


def test_emulator_keys_on_a_stub_engine():
    emulator = stub_emulator()
    engine = emulator.engine
    params = {'a': np.linspace(0., 1., 5), 'b': 0.5, 'c': np.linspace(1., 0., 5)}
    with pytest.raises(KeyError):      # a name that is no parameter
        emulator.jvp(params, {'a': 1., 'd': 1.})
    assert not engine.calls
    out = emulator.jvp(params, {'b': 2.})      # missing names are zero components
    X, T, columns = engine.calls.pop()
    assert columns is None and X.shape == (5, 3) and T.shape == (5, 3) and T.dtype == np.float64 and np.array_equal(T, np.tile([0., 2., 0.], (5, 1)))
    assert list(out) == ['curve', 'product'] and out['curve'].shape == (5, 7) and out['product'].shape == (5,) and (out['product'] == 2.).all()
    out = emulator.jvp(params, {})      # an empty dictionary: the zero direction
    X, T, columns = engine.calls.pop()
    assert T.shape == (5, 3) and not T.any() and not out['curve'].any()
    out = emulator.jvp(params, {'a': np.arange(5.), 'c': np.ones((1, 4)), 'b': np.arange(20.).reshape(5, 4)}, keys='product')      # (B,), (1, K) and (B, K)
    X, T, columns = engine.calls.pop()
    assert columns == (7, 8) and T.shape == (5, 4, 3) and list(out) == ['product'] and out['product'].shape == (5, 4)
    assert np.array_equal(T[:, :, 0], np.repeat(np.arange(5.)[:, None], 4, axis=1)) and (T[:, :, 2] == 1.).all() and np.array_equal(T[:, :, 1], np.arange(20.).reshape(5, 4))
    with pytest.raises(ValueError):      # mixed K
        emulator.jvp(params, {'a': np.ones((5, 2)), 'b': np.ones((5, 3))})
    with pytest.raises(ValueError):
        emulator.jvp(params, {'a': np.ones((5, 2, 2))})
    point = {'a': 0.1, 'b': 0.2, 'c': 0.3}      # scalar parameters: no leading axis
    out = emulator.jvp(point, {'a': 1.})
    assert out['curve'].shape == (7,) and out['product'].shape == ()
    out = emulator.jvp(point, {'a': np.ones((1, 4))})
    assert out['curve'].shape == (4, 7) and out['product'].shape == (4,)
    values, out = emulator.jvp(params, {'a': 1.}, keys=['x', 'curve'], return_value=True)
    assert list(values) == ['curve', 'x'] and list(out) == ['curve'] and engine.calls.pop()[2] == (0, 7)
