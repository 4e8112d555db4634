"""CPU: the yardstick of the contracted second derivatives (tests/vjp2_reference.py) before any device is asked.  (a) Every case that the GPU tests run has
a rounding level of at most 32 floors -- the float64 restatement of C = sum_c q d^2 value against the longdouble truth, per pair (i, j) over the batch --,
so that 16 levels stay a meaningful allowance; a case above the cap is redrawn (``seed=``, tools/search_vjp2_seeds.py), the cap never moved.  (b) The
restatement has the structure the device relies on: relu without a y function and a Taylor expansion of order 1 are exactly 0, and the cotangent enters
linearly (twice the cotangent: exactly twice the result).  (c) The sign and convention of Emulator.chi2_hessian: the central difference of the restated
Gauss-Newton gradient in longdouble, step 1e-6 xscale, against -(F - C), within 1e-8 of the point's largest |hessian| (truncation about 1e-12, rounding
about 1e-19 / 1e-6: four decades of margin)."""
import numpy as np
import pytest

import vjp2_reference as cr

MLP, TAYLOR = cr.mlp_cases(), cr.taylor_cases()


@pytest.mark.parametrize('options', MLP, ids=[cr.case_id(case) for case in MLP])
def test_mlp_levels(options):
    cfg, case = cr.mlp_case(**options)
    level = cr.level(case)
    print('level %.1f floors' % level)
    assert np.isfinite(np.asarray(case['truth'], dtype='f8')).all()
    assert level <= cr.CAP, 'redraw this case (seed=)'
    if options.get('activations') == 'relu':
        assert not case['truth'].any() and not case['restated'].any()


@pytest.mark.parametrize('options', TAYLOR, ids=[cr.case_id(case) for case in TAYLOR])
def test_taylor_levels(options):
    cfg, case = cr.taylor_case(**options)
    level = cr.level(case)
    print('level %.1f floors' % level)
    assert level <= cr.CAP, 'redraw this case (seed=)'
    if options.get('order') == 1 or options.get('T') == 1:
        assert not case['truth'].any() and not case['restated'].any()


def test_linear_in_the_cotangent():
    cfg, case = cr.mlp_case(yfunction='arcsinh')
    second = cr.mlp_second(cfg, 'f8')
    assert np.array_equal(cr.contract(second, 2. * case['q'], 'f8'), 2. * case['restated'])


def test_mirror():
    C = np.arange(12.).reshape(2, 6)
    H = cr.full(C, 3)
    assert np.array_equal(H, H.transpose(0, 2, 1)) and np.array_equal(cr.triangle(H), C)
    assert cr.pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


@pytest.mark.parametrize('kind,options', [('mlp', dict()), ('mlp', dict(yfunction='log10')), ('mlp', dict(yfunction='arcsinh')), ('mlp', dict(activations='tanh', ndim=7, B=3)),
                                          ('taylor', dict()), ('taylor', dict(ndim=7, B=3))])
def test_sign_and_convention(kind, options):
    """d gradient_i / d theta_j = -(F - C)_ij: gradient = -1/2 d chi2 / d theta, so F - C is the full half Hessian of chi2"""
    cfg, case = (cr.mlp_case if kind == 'mlp' else cr.taylor_case)(**options)
    minus_hessian, derivative, top = cr.gradient_difference(cfg, kind)
    error = np.abs(derivative - minus_hessian).max(axis=(1, 2)) / top
    print('largest relative distance %.2e' % float(error.max()))
    assert (error <= 1e-8).all()
    assert not np.allclose(np.asarray(derivative, dtype='f8'), -np.asarray(case['normal'][0], dtype='f8'), rtol=1e-6, atol=0.), 'the residual curvature does not show in this case'
