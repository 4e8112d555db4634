"""CPU: (a) the truth helpers of tests/vjp_reference.py -- the longdouble reverse pass against the cotangent contracted with the longdouble forward-mode
Jacobian of tests/jacobian_reference.py (agreement within 2^-57 A, A the magnitude pass: longdouble rounds 2^11 times finer than float64, so 9 such
roundings lie well inside, and the truth's own uncertainty is nothing against the least allowance 16 x 2^-53 A of the device tests) and against central
differences of the longdouble prediction (step 2^-20 of each parameter's scale, 1e-8 of the entry's magnitude pass: the check of
tests/test_jacobian_host.py); (b) the level of the tolerance rule, at most 32 over the three float64 orders for every shape the device tests use
(measured: at most 9), which keeps the rule meaningful; (c) the argument checks of cp_mlp_vjp and cp_taylor_vjp, which come back before any device
call (this test runs without a device)."""
import ctypes

import numpy as np
import pytest

import jacobian_reference as jr
import mlp_reference as mr
import vjp_reference as vr
from test_jacobian_host import central_differences

LD = np.longdouble
TRUTH = 2.**-57


def mlp_args(cfg):
    return (cfg['packed'], cfg['dims'], cfg['activations'], cfg['X'], cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])


@pytest.mark.parametrize('options', vr.MLP_CASES, ids=[vr.case_id(case) for case in vr.MLP_CASES])
def test_mlp_truth_and_level(options):
    cfg = vr.mlp_config(**options)
    G_ld, A, level = vr.mlp_case(cfg, cfg['cot'])
    assert G_ld.dtype == LD and G_ld.shape == cfg['X'].shape and (A > 0).all()
    forward = np.einsum('bc,bic->bi', cfg['cot'].astype(LD), jr.mlp_jacobian(*mlp_args(cfg), dtype=LD)[1])
    used = float((np.abs(G_ld - forward) / A).max())
    print('%s: reverse against forward mode in longdouble %.3g x 2^-57 A, level %.3g' % (options, used / TRUTH, level))
    assert used <= TRUTH
    assert level <= 32.


@pytest.mark.parametrize('columns', vr.MLP_RANGES)
@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_mlp_level_of_the_column_ranges(yfunction, columns):
    cfg = vr.mlp_config(yfunction=yfunction, activations='tanh')
    G_ld, A, level = vr.mlp_case(cfg, cfg['cot'][:, columns[0]:columns[1]], columns=columns)
    print('%s, columns %s: level %.3g' % (yfunction or 'no y function', columns, level))
    assert level <= 32.


@pytest.mark.parametrize('options', vr.TAYLOR_CASES, ids=[vr.case_id(case) for case in vr.TAYLOR_CASES])
def test_taylor_truth_and_level(options):
    c = vr.taylor_config(**options)
    G_ld, A, level = vr.taylor_case(c, c['cot'])
    assert G_ld.dtype == LD and G_ld.shape == c['X'].shape
    forward = np.einsum('bc,bic->bi', c['cot'].astype(LD), jr.taylor_jacobian(c['center'], c['powers'], c['derivatives'], c['X'], dtype=LD))
    dist = np.abs(G_ld - forward)
    assert (dist <= TRUTH * A).all()
    print('%s: level %.3g' % (options, level))
    assert level <= 32.
    if c['powers'].shape[0] == 1:      # the constant alone
        assert not G_ld.any() and not A.any()


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
@pytest.mark.parametrize('activation', mr.ACTIVATIONS)
def test_mlp_truth_against_central_differences(activation, yfunction):
    cfg = vr.mlp_config(B=16, M=8, activations=activation, yfunction=yfunction, seed=3)
    G_ld, A, level = vr.mlp_case(cfg, cfg['cot'])
    args = mlp_args(cfg)
    fd = central_differences(lambda Xp: mr.predict(args[0], args[1], args[2], Xp, *args[4:], dtype=LD), cfg['X'], cfg['xscale'])
    G_fd = np.einsum('bc,bic->bi', cfg['cot'].astype(LD), fd)
    used = float((np.abs(G_ld - G_fd) / A).max())
    print('%s, %s: largest distance from the central differences %.3g of the magnitude pass' % (activation, yfunction or 'no y function', used))
    assert used <= 1e-8


def test_taylor_truth_against_central_differences():
    c = vr.taylor_config(B=16, T=65, M=9)
    G_ld, A, level = vr.taylor_case(c, c['cot'])
    fd = central_differences(lambda Xp: jr.taylor_predict(c['center'], c['powers'], c['derivatives'], Xp, dtype=LD), c['X'], np.ones(3))
    used = float((np.abs(G_ld - np.einsum('bc,bic->bi', c['cot'].astype(LD), fd)) / A).max())
    print('taylor: largest distance from the central differences %.3g of the magnitude pass' % used)
    assert used <= 1e-8


def test_magnitude_pass_bounds_the_truth():
    cfg = vr.mlp_config(yfunction='arcsinh', activations=['relu', 'identity-silu'])
    G_ld, A, level = vr.mlp_case(cfg, cfg['cot'])
    assert (np.abs(G_ld) <= A).all()
    c = vr.taylor_config()
    G_ld, A, level = vr.taylor_case(c, c['cot'])
    assert (np.abs(G_ld) <= A).all()


FAKE = ctypes.c_void_p(8)      # a non-null pointer nobody reads: every call here returns before its first device call
BIG = 2**40                    # a workspace nobody allocates


def mlp_call(B=4, ndim=3, widths=(5, 17), M=8, col0=0, ncols=8, ldc=8, ldv=8, pointers=None, yfunction=0, work=BIG, value=True):
    from cosmoprimo_amd import _lib
    L = len(widths)
    p = [FAKE] * 9 if pointers is None else pointers      # d_x, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, d_cot, d_grad, d_work
    return _lib.load().cp_mlp_vjp(p[0], B, ndim, L, (ctypes.c_int * L)(*widths), (ctypes.c_int * L)(*([0] * L)), M, p[1], p[2], p[3], p[4], p[5], yfunction, col0, ncols,
                                  p[6], ldc, FAKE if value else None, ldv, p[7], p[8], work, 0, None)


def taylor_call(B=4, ndim=3, T=20, max_power=3, M=8, col0=0, ncols=8, ldc=8, pointers=None, work=BIG):
    from cosmoprimo_amd import _lib
    p = [FAKE] * 7 if pointers is None else pointers      # d_x, d_center, d_powers, d_derivatives_t, d_cot, d_grad, d_work
    return _lib.load().cp_taylor_vjp(p[0], B, p[1], p[2], ndim, T, max_power, p[3], M, col0, ncols, p[4], ldc, p[5], p[6], work, 0, None)


@pytest.mark.parametrize('call,npointers,rows', [(mlp_call, 9, 1), (taylor_call, 7, 3)], ids=['mlp', 'taylor'])
def test_argument_checks_come_before_any_device_call(call, npointers, rows):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    for k in range(npointers):      # each null pointer
        assert call(pointers=[None if j == k else FAKE for j in range(npointers)]) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert call(ldc=7) == _lib.CP_EINVAL and b'row stride' in lib.cp_last_error()
    for col0, ncols in ((-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)):
        assert call(col0=col0, ncols=ncols, ldc=16) == _lib.CP_EINVAL and b'columns' in lib.cp_last_error()
    assert call(B=-1) == _lib.CP_EINVAL
    assert call(B=0) == _lib.CP_OK and call(B=0, pointers=[None] * npointers, work=0) == _lib.CP_OK
    assert call(ndim=33) == _lib.CP_EUNSUPPORTED
    # beyond the 2^31 - 1 row tiles of 64 that the grid holds (MLP: a row per point; Taylor: per point and parameter); the largest count below is refused
    # only for its null pointers
    most = (2**31 - 1) * 64 // rows
    assert call(B=most + 1) == _lib.CP_EUNSUPPORTED and b'2^37' in lib.cp_last_error()
    assert call(B=2**62) == _lib.CP_EUNSUPPORTED
    assert call(B=most, pointers=[None] * npointers) == _lib.CP_EINVAL
    with pytest.raises(NotImplementedError):
        _lib.check(call(B=most + 1))


def test_a_short_workspace_is_refused_before_any_launch():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    widths = (ctypes.c_int * 2)(5, 17)
    need = lib.cp_mlp_vjp_workspace_doubles(4, 3, 2, widths, 8, 8)
    assert need == 4 * (5 + 17) + 4 * 8 + 4 * 17      # the pre-activations, the weighted cotangent, one slice of partial products
    assert mlp_call(work=need - 1) == _lib.CP_EINVAL and b'workspace' in lib.cp_last_error()
    assert lib.cp_mlp_vjp_workspace_doubles(4, 3, 2, widths, 8, 2) == 4 * (5 + 17) + 4 * 2 + 4 * 17
    assert lib.cp_mlp_vjp_workspace_doubles(0, 3, 2, widths, 8, 8) == 0
    for bad in ((-1, 3, 8, 8), (4, 33, 8, 8), (4, 3, 8, 0), (4, 3, 8, 9)):
        assert lib.cp_mlp_vjp_workspace_doubles(bad[0], bad[1], 2, widths, bad[2], bad[3]) < 0
    assert lib.cp_taylor_vjp_workspace_doubles(4, 20) == 80 and lib.cp_taylor_vjp_workspace_doubles(-1, 20) == -_lib.CP_EINVAL
    assert lib.cp_taylor_vjp_workspace_doubles(4, 0) == -_lib.CP_EINVAL
    assert taylor_call(work=79) == _lib.CP_EINVAL and b'workspace' in lib.cp_last_error()


def test_argument_checks_of_the_network_and_the_polynomial():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    assert mlp_call(widths=(5, 65)) == _lib.CP_EUNSUPPORTED and b'width 65' in lib.cp_last_error()
    assert mlp_call(widths=(5, 0)) == _lib.CP_EINVAL
    assert mlp_call(widths=(8,) * 9) == _lib.CP_EUNSUPPORTED
    assert mlp_call(yfunction=3) == _lib.CP_EINVAL
    assert mlp_call(ldv=7) == _lib.CP_EINVAL and b'row stride' in lib.cp_last_error()
    assert mlp_call(ldv=7, value=False, B=0) == _lib.CP_OK      # no value wanted: its stride is not read
    assert taylor_call(max_power=16) == _lib.CP_EUNSUPPORTED
    assert taylor_call(max_power=-1) == _lib.CP_EINVAL and taylor_call(T=0) == _lib.CP_EINVAL
