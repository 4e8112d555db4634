"""CPU: the host side of the Taylor emulator (cosmoprimo_amd/emulators/tools) against tests/golden/taylor.npz, the reference's own grids, terms and
coefficients for a toy function (tools/gen_taylor_golden.py): grids and term lists are equal bit for bit and in order, and the finite-difference operator
S reproduces the reference's coefficients as ``S @ Y``.

Tolerance (derived, not measured).  Both sides compute the same dot products in different orders: for row t and column m the allowed difference is
``K eps sum_i |S_ti| |Y_im|`` with eps = 2^-53 and K = 2 (n + ndim + 2): n the non-zero entries of the row (the standard summation bound), ndim + 2 for the
products that form a weight, the factor 2 because the reference and this code each carry that error.  numpy's ``S @ Y`` on the build machine used 0.054
of it at most."""
import numpy as np
import pytest

CONFIGS = [(3, 2), (4, 2), (2, 4), ({'a': 3, 'b': 1, 'c': 2}, 2), ({'a': 2, 'b': 0, 'c': 1}, 2)]
SIZES = [(33, 20), (57, 35), (61, 10), (17, 8), (9, 4)]
EPS = 2.**-53


def dot_bound(A, B, ndim):
    """The bound of the module docstring for every entry of A @ B."""
    n = (A != 0).sum(axis=1)
    return (2 * (n + ndim + 2))[:, None] * EPS * (np.abs(A) @ np.abs(B))


def sampler_of(g, i):
    from cosmoprimo_amd.emulators import DiffSampler
    order, accuracy = CONFIGS[i]
    return DiffSampler(None, {str(name): tuple(limits) for name, limits in zip(g['names'], g['limits'])}, order=order, accuracy=accuracy)


@pytest.mark.parametrize('i', range(len(CONFIGS)))
def test_points(golden, i):
    g = golden('taylor')
    samples = sampler_of(g, i).points()
    names = [str(name) for name in g['names']]
    assert list(samples) == names
    X = samples.matrix()
    assert X.shape == (SIZES[i][0], 3) and np.array_equal(X, g['c%d_X' % i])
    assert np.array_equal(np.array(samples.attrs['cidx']), g['c%d_cidx' % i])
    assert [samples.attrs['order'][name] for name in names] == g['c%d_order' % i].tolist()
    assert [samples.attrs['accuracy'][name] for name in names] == g['c%d_accuracy' % i].tolist()


@pytest.mark.parametrize('i', range(len(CONFIGS)))
def test_terms_and_operator(golden, i):
    from cosmoprimo_amd.emulators.tools import taylor_operator
    g = golden('taylor')
    X, Y = g['c%d_X' % i], g['c%d_Y' % i]
    center, powers, S = taylor_operator(X, g['c%d_cidx' % i], g['c%d_order' % i], g['c%d_accuracy' % i])
    assert np.array_equal(center, g['c%d_center' % i])
    assert powers.shape == (SIZES[i][1], 3) and np.array_equal(powers, g['c%d_powers' % i])
    assert S.shape == (SIZES[i][1], SIZES[i][0])
    ratio = np.abs(S @ Y - g['c%d_derivatives' % i]) / dot_bound(S, Y, 3)
    print('config %d: S @ Y against the reference, largest fraction of the bound %.3g' % (i, ratio.max()))
    assert ratio.max() <= 1.


def test_monomials_times_derivatives(golden):
    """The prediction as numpy forms it (monomials by repeated multiplication, then a matrix product) stays inside the same bound against the reference's
    predictions: the bound the device kernel is held to in test_taylor_gpu.py."""
    g = golden('taylor')
    for i in range(len(CONFIGS)):
        powers, derivatives = g['c%d_powers' % i], g['c%d_derivatives' % i]
        d = g['c%d_Xq' % i] - g['c%d_center' % i]
        mono = np.ones((len(d), len(powers)))
        for t, power in enumerate(powers):
            for j, p in enumerate(power):
                if p > 0:
                    v = d[:, j]
                    for _ in range(1, p):
                        v = v * d[:, j]
                    mono[:, t] *= v
        ratio = np.abs(mono @ derivatives - g['c%d_Yq' % i]) / dot_bound(mono, derivatives, 3)
        print('config %d: monomials @ derivatives against the reference, largest fraction of the bound %.3g' % (i, ratio.max()))
        assert ratio.max() <= 1.


@pytest.mark.parametrize('accuracy,match', [(3, 'EVEN'), (1, 'EVEN'), (0, '< 1'), (-2, '< 1'), ({'a': 2, 'b': 3}, 'EVEN'), ({'a': 2}, 'not specified')])
def test_accuracy_errors(accuracy, match):
    from cosmoprimo_amd.emulators import DiffSampler
    with pytest.raises(ValueError, match=match):
        DiffSampler(None, {'a': (0., 1.), 'b': (0., 1.)}, order=2, accuracy=accuracy)


def test_accuracy_is_not_checked_for_fixed_parameters():
    from cosmoprimo_amd.emulators import DiffSampler
    sampler = DiffSampler(None, {'a': (0., 1.), 'b': (2., 4.)}, order={'a': 1, 'b': None}, accuracy={'a': 2, 'b': 3})
    samples = sampler.points()
    assert samples.matrix().tolist() == [[0., 3.], [1., 3.], [0.5, 3.]] and samples.attrs['cidx'] == (2,)


def test_argument_checks_come_before_any_device_call():
    """(This test runs without a device.)"""
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    assert lib.cp_taylor_predict(None, 4, None, None, 33, 5, 1, None, 8, None, 0, None) == _lib.CP_EUNSUPPORTED and b'cp_taylor_predict' in lib.cp_last_error()
    assert lib.cp_taylor_predict(None, 4, None, None, 3, 5, 16, None, 8, None, 0, None) == _lib.CP_EUNSUPPORTED
    assert lib.cp_taylor_predict(None, 4, None, None, 3, 5, 2, None, 8, None, 0, None) == _lib.CP_EINVAL and b'null' in lib.cp_last_error()
    assert lib.cp_taylor_predict(None, -1, None, None, 3, 5, 2, None, 8, None, 0, None) == _lib.CP_EINVAL
    assert lib.cp_taylor_predict(None, 4, None, None, 3, 0, 2, None, 8, None, 0, None) == _lib.CP_EINVAL
    assert lib.cp_taylor_predict(None, 0, None, None, 3, 5, 2, None, 8, None, 0, None) == _lib.CP_OK
    assert lib.cp_taylor_fit(None, 5, 9, None, 8, None, 0, None) == _lib.CP_EINVAL and b'cp_taylor_fit' in lib.cp_last_error()
    assert lib.cp_taylor_fit(None, 0, 9, None, 8, None, 0, None) == _lib.CP_EINVAL
