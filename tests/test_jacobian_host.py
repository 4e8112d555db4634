"""CPU: (a) the truth helpers of tests/jacobian_reference.py against central differences of the predictions in longdouble; (b) the argument checks of
cp_mlp_jacobian and cp_taylor_jacobian, which come back before any device call (this test runs without a device).

(a) The differences are taken of ``mlp_reference.predict`` (of the polynomial for Taylor) in longdouble with the step h = 2^-20 of each parameter's scale.
Truncation is h^2 ~ 1e-12 times a third derivative of order one, rounding 1e-19 / h ~ 1e-13: agreement to 1e-8 of the largest entry of each
(parameter, column) block leaves four orders of margin, and a helper that misses it is wrong."""
import ctypes

import numpy as np
import pytest

import jacobian_reference as jr
import mlp_reference as mr
from mlp_device import draw_network

LD = np.longdouble
STEP = LD(2)**-20


def central_differences(f, X, scale):
    """(B, ndim, M) from f: (B, ndim) longdouble -> (B, M) longdouble."""
    X = np.asarray(X).astype(LD)
    out = []
    for i in range(X.shape[1]):
        h = STEP * LD(scale[i])
        up, down = X.copy(), X.copy()
        up[:, i] += h
        down[:, i] -= h
        out.append((f(up) - f(down)) / (up[:, i] - down[:, i])[:, None])
    return np.stack(out, axis=1)


def assert_blocks(J, fd, what):
    top = np.abs(J).max(axis=0)
    dist = np.abs(J - fd).max(axis=0)
    assert (top > 0).all(), what
    print('%s: largest distance from the central differences %.3g of the block' % (what, float((dist / top).max())))
    assert (dist <= 1e-8 * top).all(), what


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
@pytest.mark.parametrize('activation', mr.ACTIVATIONS)
def test_mlp_helper_against_central_differences(activation, yfunction):
    dims = (3, 5, 17, 8)
    rng = np.random.default_rng(11 + 4 * mr.ACTIVATIONS.index(activation) + len(yfunction))
    packed = draw_network(rng, dims)
    xoffset, xscale = rng.uniform(-1., 1., 3), rng.uniform(0.5, 2., 3)
    yoffset, yscale = rng.normal(0., 1., 8), rng.uniform(0.5, 2., 8)
    X = xoffset + xscale * rng.uniform(0., 1., (16, 3))
    args = ([activation] * 2, xoffset, xscale, yoffset, yscale, yfunction)
    value, J = jr.mlp_jacobian(packed, dims, args[0], X, *args[1:], dtype=LD)
    assert value.dtype == LD and J.shape == (16, 3, 8)
    assert np.array_equal(value, mr.predict(packed, dims, args[0], X, *args[1:], dtype=LD))
    fd = central_differences(lambda Xp: mr.predict(packed, dims, args[0], Xp, *args[1:], dtype=LD), X, xscale)
    assert_blocks(J, fd, '%s, %s' % (activation, yfunction or 'no y function'))
    J64 = jr.mlp_jacobian(packed, dims, args[0], X, *args[1:], dtype='f8')[1]
    assert J64.dtype == np.float64 and np.abs(J64 - J).max() <= 1e-12 * np.abs(J).max()


def taylor_case(rng, B=16, ndim=3, T=65, M=9):
    powers = rng.integers(0, 4, (T, ndim)).astype('i4')
    powers[0] = 0
    powers[T // 2, rng.integers(ndim)] = 15
    return dict(center=rng.uniform(-0.5, 0.5, ndim), powers=powers, derivatives=rng.normal(0., 1., (T, M)), X=rng.uniform(-1., 1., (B, ndim)))


def test_taylor_helper_against_central_differences():
    c = taylor_case(np.random.default_rng(3))
    J = jr.taylor_jacobian(c['center'], c['powers'], c['derivatives'], c['X'], dtype=LD)
    assert J.dtype == LD and J.shape == (16, 3, 9)
    fd = central_differences(lambda Xp: jr.taylor_predict(c['center'], c['powers'], c['derivatives'], Xp, dtype=LD), c['X'], np.ones(3))
    assert_blocks(J, fd, 'taylor')


def test_taylor_helper_power_rules():
    """Power 0 of the row's own parameter: exactly 0 whatever x holds; of another one: the factor is skipped; power 1 drops the factor."""
    powers = np.array([[0, 0], [1, 0], [0, 2], [1, 1]], dtype='i4')
    X = np.array([[np.nan, 3.], [2., np.inf]])
    left = jr.taylor_left(np.zeros(2), powers, X)
    assert np.array_equal(left[0], [[0., 1., 0., 3.], [0., 0., 6., np.nan]], equal_nan=True)
    assert np.array_equal(left[1], [[0., 1., 0., np.inf], [0., 0., np.inf, 2.]])


FAKE = ctypes.c_void_p(8)      # a non-null pointer nobody reads: every call here returns before its first device call


def mlp_call(B=4, ndim=3, widths=(5, 17), M=8, col0=0, ncols=8, ldv=8, ldj=8, pointers=None, yfunction=0):
    from cosmoprimo_amd import _lib
    L = len(widths)
    p = [FAKE] * 8 if pointers is None else pointers      # d_x, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, d_value, d_jac
    return _lib.load().cp_mlp_jacobian(p[0], B, ndim, L, (ctypes.c_int * L)(*widths), (ctypes.c_int * L)(*([0] * L)), M, p[1], p[2], p[3], p[4], p[5], yfunction, col0, ncols,
                                       p[6], ldv, p[7], ldj, 0, None)


def taylor_call(B=4, ndim=3, T=20, max_power=3, M=8, col0=0, ncols=8, ldj=8, pointers=None):
    from cosmoprimo_amd import _lib
    p = [FAKE] * 5 if pointers is None else pointers      # d_x, d_center, d_powers, d_derivatives, d_jac
    return _lib.load().cp_taylor_jacobian(p[0], B, p[1], p[2], ndim, T, max_power, p[3], M, col0, ncols, p[4], ldj, 0, None)


@pytest.mark.parametrize('call,npointers', [(mlp_call, 8), (taylor_call, 5)], ids=['mlp', 'taylor'])
def test_argument_checks_come_before_any_device_call(call, npointers):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    for k in range(npointers):      # each null pointer
        assert call(pointers=[None if j == k else FAKE for j in range(npointers)]) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert call(ldj=7) == _lib.CP_EINVAL and b'row stride' in lib.cp_last_error()
    for col0, ncols in ((-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)):
        assert call(col0=col0, ncols=ncols, ldj=16) == _lib.CP_EINVAL and b'columns' in lib.cp_last_error()
    assert call(B=-1) == _lib.CP_EINVAL
    assert call(B=0) == _lib.CP_OK and call(B=0, pointers=[None] * npointers) == _lib.CP_OK
    assert call(ndim=33) == _lib.CP_EUNSUPPORTED
    # rows B ndim beyond the 2^31 - 1 row tiles of 64 that the grid holds; the largest count below is refused only for its null pointers
    most = (2**31 - 1) * 64 // 3
    assert call(B=most + 1) == _lib.CP_EUNSUPPORTED and b'2^37' in lib.cp_last_error()
    assert call(B=2**62) == _lib.CP_EUNSUPPORTED
    assert call(B=most, pointers=[None] * npointers) == _lib.CP_EINVAL
    with pytest.raises(NotImplementedError):
        _lib.check(call(B=most + 1))


def test_argument_checks_of_the_network_and_the_polynomial():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    assert mlp_call(widths=(5, 65)) == _lib.CP_EUNSUPPORTED and b'width 65' in lib.cp_last_error()
    assert mlp_call(widths=(5, 0)) == _lib.CP_EINVAL
    assert mlp_call(widths=(8,) * 9) == _lib.CP_EUNSUPPORTED
    assert mlp_call(yfunction=3) == _lib.CP_EINVAL
    assert mlp_call(ldv=7) == _lib.CP_EINVAL and b'row stride' in lib.cp_last_error()
    assert taylor_call(max_power=16) == _lib.CP_EUNSUPPORTED
    assert taylor_call(max_power=-1) == _lib.CP_EINVAL and taylor_call(T=0) == _lib.CP_EINVAL
