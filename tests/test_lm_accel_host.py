"""CPU: (a) the argument checks of cp_lm_step_velocity and cp_lm_accelerate, which come back by status, in the stated order, with the entry point's name in
cp_last_error() before any device call (this test runs without a device; the pointers are fakes nobody may read); (b) the restatement of
tests/lm_accel_reference.py over every case of tests/test_lm_accel_gpu.py: the same discrete decisions in float64 and in longdouble, no gate within a
factor 1.25 of equality, the level of the tolerance rule below the caps recorded here, and with ``h = 0`` the bits of ``lm_reference.step``'s ``next``;
(c) the restated loop of Emulator.least_squares on Rosenbrock's valley written as two residuals: geodesic acceleration converges in strictly fewer
evaluations than plain Levenberg-Marquardt, and the acceleration with the wrong sign in more."""
import ctypes

import numpy as np
import pytest

import lm_accel_reference as la
import lm_reference as lr

LD = np.longdouble
FAKE = ctypes.c_void_p(8)
VELOCITY_POINTERS = 15      # x, fisher, grad, chi2, lambda, status, naccepted; xt, fisher_t, grad_t, chi2_t; lo, hi; next, velocity
ACCELERATE_POINTERS = 11      # x, fisher, grad, lambda, status; lo, hi; velocity, h; next, naccelerated
# Measured here over every case below: ``next`` of cp_lm_accelerate on the well-conditioned fits at most 31.04 floors from the truth (ndim = 32), on a matrix
# of condition number 1e10 (kind 'ill') 2.7e8 floors (ndim = 2); ``velocity`` of cp_lm_step_velocity on the cases of lm_reference.make_case at most 5.9e3
# floors (ndim = 31: relative to the fit's largest component, where ``next`` is relative to x + delta), 'ill' 7.4e9 floors (ndim = 2).  The caps are the
# next powers of two.
LEVEL_CAP, ILL_CAP, VELOCITY_CAP, ILL_VELOCITY_CAP = 32., 2.**29, 8192., 2.**33


def velocity_call(B=4, ndim=3, pointers=None, up=10., down=0.1, lmin=1e-12, lmax=1e12, ftol=1e-8):
    from cosmoprimo_amd import _lib
    p = [FAKE] * VELOCITY_POINTERS if pointers is None else pointers
    return _lib.load().cp_lm_step_velocity(B, ndim, *p[:13], up, down, lmin, lmax, ftol, p[13], p[14], 0, None)


def accelerate_call(B=4, ndim=3, pointers=None, alpha=0.75):
    from cosmoprimo_amd import _lib
    p = [FAKE] * ACCELERATE_POINTERS if pointers is None else pointers
    return _lib.load().cp_lm_accelerate(B, ndim, *p[:9], alpha, p[9], p[10], 0, None)


@pytest.mark.parametrize('call,npointers,name', [(velocity_call, VELOCITY_POINTERS, b'cp_lm_step_velocity'), (accelerate_call, ACCELERATE_POINTERS, b'cp_lm_accelerate')],
                         ids=['step_velocity', 'accelerate'])
def test_argument_checks_come_before_any_device_call(call, npointers, name):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    named = lambda words: name in lib.cp_last_error() and words in lib.cp_last_error()      # noqa: E731
    none = [None] * npointers
    assert call(B=-1) == _lib.CP_EINVAL and named(b'fits') and call(ndim=0) == _lib.CP_EINVAL and named(b'fits') and call(ndim=-3) == _lib.CP_EINVAL
    assert call(ndim=33) == _lib.CP_EUNSUPPORTED and named(b'at most 32')
    with pytest.raises(NotImplementedError):
        _lib.check(call(ndim=33))
    # the order: the counts before the cap of ndim, that before the cap of B, that before B = 0, that before the pointers, those before the scalars
    assert call(B=-1, ndim=33) == _lib.CP_EINVAL and call(B=-1, ndim=33, pointers=none) == _lib.CP_EINVAL and named(b'fits')
    assert call(B=2**62, ndim=33) == _lib.CP_EUNSUPPORTED and named(b'at most 32')
    assert call(B=0, ndim=33, pointers=none) == _lib.CP_EUNSUPPORTED and call(B=0, ndim=0) == _lib.CP_EINVAL
    for ndim in (1, 2, 3, 8, 9, 17, 32):      # the cap of B: 2^31 - 1 workgroups; the largest count is refused only for its null pointers
        most = (2**31 - 1) * lr.lanes(ndim)[2]
        assert call(B=most + 1, ndim=ndim) == _lib.CP_EUNSUPPORTED and named(b'workgroups'), ndim
        assert call(B=most + 1, ndim=ndim, pointers=none) == _lib.CP_EUNSUPPORTED
        assert call(B=most, ndim=ndim, pointers=none) == _lib.CP_EINVAL and named(b'null pointer'), ndim
    assert call(B=0) == _lib.CP_OK and call(B=0, pointers=none) == _lib.CP_OK
    for k in range(npointers):
        assert call(pointers=[None if j == k else FAKE for j in range(npointers)]) == _lib.CP_EINVAL and named(b'null pointer'), k


def test_the_scalars():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    nan, inf = float('nan'), float('inf')
    for alpha in (0., -0.75, nan, inf, -inf):
        assert accelerate_call(alpha=alpha) == _lib.CP_EINVAL and b'cp_lm_accelerate' in lib.cp_last_error() and b'alpha' in lib.cp_last_error(), alpha
    with pytest.raises(ValueError):
        _lib.check(accelerate_call(alpha=0.))
    # a null pointer comes before alpha, B = 0 and the caps before both
    assert accelerate_call(alpha=nan, pointers=[None] * ACCELERATE_POINTERS) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert accelerate_call(B=0, alpha=nan, pointers=[None] * ACCELERATE_POINTERS) == _lib.CP_OK
    assert accelerate_call(ndim=33, alpha=nan) == _lib.CP_EUNSUPPORTED
    for controls in (dict(up=1.), dict(down=0.), dict(lmin=1., lmax=0.5), dict(ftol=nan)):
        assert velocity_call(**controls) == _lib.CP_EINVAL and b'cp_lm_step_velocity' in lib.cp_last_error() and b'ftol' in lib.cp_last_error(), controls
    assert velocity_call(up=1., pointers=[None] * VELOCITY_POINTERS) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert velocity_call(B=0, up=1., pointers=[None] * VELOCITY_POINTERS) == _lib.CP_OK


EXPECTED = {'pass': True, 'refuse': False, 'zero-h': True, 'nan-h': False, 'inf-h': False, 'zero-v': False, 'terminal': False, 'cross': True, 'pivot': False, 'ill': True}


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_levels_and_decisions_of_the_accelerate_cases(ndim):
    worst, worst_ill = 0., 0.
    for B in lr.batch_sizes(ndim):
        state, v, h, lo, hi, kinds = la.make_case(ndim, B)
        what = (ndim, B)
        for dtype in ('f8', LD):      # the gate is a discrete decision and sits on no rounding
            ratio = la.gate_ratio(state, v, h, lo, hi, dtype=dtype)
            finite = ratio[np.isfinite(ratio)]
            assert not ((finite > 0.8) & (finite < 1.25)).any(), what
        next64, taken64 = la.accelerate(state, v, h, lo, hi, dtype='f8')
        nextld, takenld = la.accelerate(state, v, h, lo, hi, dtype=LD)
        assert next64.dtype == np.float64 and nextld.dtype == LD and np.array_equal(taken64, takenld), what
        assert np.isfinite(next64).all() and (next64 >= lo).all() and (next64 <= hi).all(), what
        plain = state['x'] + v      # the plain step, the bits of cp_lm_step's next: x + delta, clipped
        plain = np.where(plain < lo, lo, np.where(plain > hi, hi, plain))
        for b, kind in enumerate(kinds):      # what each kind is there for
            assert taken64[b] == EXPECTED.get(kind, ndim > 1), (what, b, kind)
            if kind in ('terminal', 'pivot', 'zero-v'):
                assert np.array_equal(next64[b], state['x'][b]), (what, b, kind)
            if kind in ('refuse', 'nan-h', 'inf-h', 'zero-h'):
                assert np.array_equal(next64[b], plain[b]), (what, b, kind)
            if kind == 'pass':
                assert not np.array_equal(next64[b], plain[b]), (what, b, kind)
            if kind == 'cross':
                assert next64[b, 0] in (lo[0], hi[0]) and nextld[b, 0] in (lo[0], hi[0]), (what, b)
            if kind == 'bounds':
                finite = [i for i in range(ndim) if np.isfinite(lo[i])][:2]
                assert next64[b, finite[0]] == hi[finite[0]] == state['x'][b, finite[0]], (what, b)      # held: exactly on its bound
        ill = np.array([kind == 'ill' for kind in kinds])
        if (~ill).any():
            worst = max(worst, lr.worst_level(nextld[~ill], next64[~ill]))
        if ill.any():
            worst_ill = max(worst_ill, lr.worst_level(nextld[ill], next64[ill]))
    print('ndim = %d: next at most %.4g floors from the truth, %.3g on the ill-conditioned fits' % (ndim, worst, worst_ill))
    assert worst <= LEVEL_CAP and worst_ill <= ILL_CAP


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_zero_curvature_is_the_plain_step(ndim):
    """With h = 0 the acceleration is zero: ``next`` has the bits of ``lm_reference.step``'s, whether the gate lets the (empty) correction through or not."""
    for B in lr.batch_sizes(ndim)[-2:]:
        state, trial, lo, hi, kinds = lr.make_case(ndim, B)
        new, nxt, held, v = la.step_velocity(state, trial, lo, hi, dtype='f8', **lr.CONTROLS)
        again, taken = la.accelerate(new, v, np.zeros((B, ndim)), lo, hi, dtype='f8')
        assert again.tobytes() == nxt.tobytes(), (ndim, B)
        running = new['status'] == 0
        assert not taken[~running].any() and (v[~running] == 0).all() and (v[held] == 0).all(), (ndim, B)
        assert taken[running].sum() > 0.8 * running.sum(), (ndim, B)


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_levels_of_the_velocity(ndim):
    worst, worst_ill = 0., 0.
    for B in lr.batch_sizes(ndim):
        state, trial, lo, hi, kinds = lr.make_case(ndim, B)
        new64, next64, held64, v64 = la.step_velocity(state, trial, lo, hi, dtype='f8', **lr.CONTROLS)
        newld, nextld, heldld, vld = la.step_velocity(state, trial, lo, hi, dtype=LD, **lr.CONTROLS)
        assert np.array_equal(v64 == 0, vld == 0) and np.array_equal(held64, heldld), (ndim, B)
        ill = np.array([kind == 'ill' for kind in kinds])
        if (~ill).any():
            worst = max(worst, lr.worst_level(vld[~ill], v64[~ill]))
        if ill.any():
            worst_ill = max(worst_ill, lr.worst_level(vld[ill], v64[ill]))
    print('ndim = %d: velocity at most %.4g floors from the truth, %.3g on the ill-conditioned fits' % (ndim, worst, worst_ill))
    assert worst <= VELOCITY_CAP and worst_ill <= ILL_VELOCITY_CAP


def test_rosenbrock():
    """Rosenbrock's valley as two residuals from (-1.2, 1), an open box, the default controls.  Measured with this restatement: 46 evaluations without the
    correction, 26 with it, 64 with the sign of the acceleration flipped -- which is what tells a correct rule from a wrong one."""
    plain, accelerated, flipped = la.fit_rosenbrock(False), la.fit_rosenbrock(True), la.fit_rosenbrock(True, sign=-1.)
    print('evaluations: plain %d, accelerated %d (%d corrections taken), with the wrong sign %d' % (plain[0], accelerated[0], accelerated[2], flipped[0]))
    for count, x, taken in (plain, accelerated, flipped):
        assert count < 500 and np.abs(x - 1.).max() < 1e-6
    assert accelerated[0] < plain[0] and accelerated[2] > 0 and plain[2] == 0
    assert flipped[0] > accelerated[0]
