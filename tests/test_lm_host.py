"""CPU: (a) the argument checks of cp_lm_step, cp_spd_inverse and cp_lm_layout, which come back by status, in the stated order, with the entry point's name in
cp_last_error() before any device call (this test runs without a device; the pointers are fakes nobody may read); (b) cp_lm_layout against the stated rule;
(c) the restatement of tests/lm_reference.py against numpy.linalg, and over every case of tests/test_lm_step_gpu.py: the level of the tolerance rule
below the caps recorded here, and the same discrete decisions in float64 and in longdouble."""
import ctypes

import numpy as np
import pytest

import lm_reference as lr

LD = np.longdouble
FAKE = ctypes.c_void_p(8)
STEP_POINTERS = 14      # x, fisher, grad, chi2, lambda, status, naccepted; xt, fisher_t, grad_t, chi2_t; lo, hi; next
# Measured here over every case below (parameters on scales over two decades: condition numbers of 1e3 to 1e5): ``next`` of the well-conditioned fits at
# most 3.9e3 floors from the truth (ndim = 31), an inverse 360 floors (ndim = 32); a fit on a matrix of condition number 1e10 (kind 'ill') 1.3e10 floors, an
# inverse at 1e6 6.7e5 floors.  The caps are the next powers of two.
LEVEL_CAP, INVERSE_CAP, ILL_CAP, ILL_INVERSE_CAP = 4096., 512., 2.**34, 2.**20


def step_call(B=4, ndim=3, pointers=None, up=10., down=0.1, lmin=1e-12, lmax=1e12, ftol=1e-8):
    from cosmoprimo_amd import _lib
    p = [FAKE] * STEP_POINTERS if pointers is None else pointers
    return _lib.load().cp_lm_step(B, ndim, *p[:13], up, down, lmin, lmax, ftol, p[13], 0, None)


def inverse_call(B=4, ndim=3, pointers=None):
    from cosmoprimo_amd import _lib
    p = [FAKE] * 3 if pointers is None else pointers
    return _lib.load().cp_spd_inverse(B, ndim, p[0], p[1], p[2], 0, None)


@pytest.mark.parametrize('call,npointers,name', [(step_call, STEP_POINTERS, b'cp_lm_step'), (inverse_call, 3, b'cp_spd_inverse')], ids=['step', 'inverse'])
def test_argument_checks_come_before_any_device_call(call, npointers, name):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    named = lambda words: name in lib.cp_last_error() and words in lib.cp_last_error()      # noqa: E731
    none = [None] * npointers
    assert call(B=-1) == _lib.CP_EINVAL and named(b'fits') and call(ndim=0) == _lib.CP_EINVAL and named(b'fits') and call(ndim=-3) == _lib.CP_EINVAL
    assert call(ndim=33) == _lib.CP_EUNSUPPORTED and named(b'at most 32')
    with pytest.raises(NotImplementedError):
        _lib.check(call(ndim=33))
    # the order: the counts before the cap of ndim, that before the cap of B, that before B = 0, that before the pointers
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


def test_the_scalars_of_the_step():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    nan = float('nan')
    bad = [dict(up=1.), dict(up=0.5), dict(up=nan), dict(down=0.), dict(down=1.5), dict(down=-0.1), dict(down=nan), dict(lmin=0.), dict(lmin=-1.), dict(lmin=nan),
           dict(lmin=1., lmax=0.5), dict(lmax=nan), dict(ftol=-1e-9), dict(ftol=nan)]
    for controls in bad:
        assert step_call(**controls) == _lib.CP_EINVAL and b'cp_lm_step' in lib.cp_last_error() and b'ftol' in lib.cp_last_error(), controls
    with pytest.raises(ValueError):
        _lib.check(step_call(up=1.))
    # a null pointer comes before the scalars, B = 0 before both
    assert step_call(up=1., pointers=[None] * STEP_POINTERS) == _lib.CP_EINVAL and b'null pointer' in lib.cp_last_error()
    assert step_call(B=0, up=1., pointers=[None] * STEP_POINTERS) == _lib.CP_OK
    assert step_call(ndim=33, up=1.) == _lib.CP_EUNSUPPORTED


def test_layout():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    G, per = ctypes.c_int(), ctypes.c_int()
    for ndim in range(1, 33):
        assert lib.cp_lm_layout(ndim, ctypes.byref(G), ctypes.byref(per)) == _lib.CP_OK
        want = lr.lanes(ndim)
        assert G.value == want[0] and per.value == want[2], ndim
        assert G.value >= ndim and (G.value == 1 or G.value // 2 < ndim) and G.value & (G.value - 1) == 0 and per.value % (64 // G.value) == 0
    assert lib.cp_lm_layout(0, ctypes.byref(G), ctypes.byref(per)) == _lib.CP_EINVAL and b'cp_lm_layout' in lib.cp_last_error()
    assert lib.cp_lm_layout(33, ctypes.byref(G), ctypes.byref(per)) == _lib.CP_EUNSUPPORTED
    assert lib.cp_lm_layout(33, None, None) == _lib.CP_EUNSUPPORTED and lib.cp_lm_layout(3, None, ctypes.byref(per)) == _lib.CP_EINVAL


@pytest.mark.parametrize('ndim', [1, 2, 5, 16, 32])
def test_restatement_against_numpy_linalg(ndim):
    """numpy.linalg works in float64: the longdouble restatement agrees with it as far as float64 and the condition number go, and solves its own system in
    longdouble as far as longdouble goes."""
    rng = np.random.default_rng(ndim)
    B = 6
    F = np.stack([lr.spd(rng, ndim) for b in range(B)])
    g = rng.standard_normal((B, ndim))
    lam = 10.**rng.uniform(-4., -1., B)
    state = dict(x=np.zeros((B, ndim)), fisher=F, gradient=g, chi2=np.ones(B), status=np.zeros(B, dtype='i4'), naccepted=np.ones(B, dtype='i4'))
    state['lambda'] = lam / 10.
    trial = dict(x=np.ones((B, ndim)), fisher=F[::-1], gradient=-g, chi2=np.full(B, 2.))      # rejected: lambda goes up by 10, the step leaves from the state
    big = np.full(ndim, np.inf)
    for dtype in ('f8', LD):
        new, nxt, held = lr.step(state, trial, -big, big, dtype=dtype)
        assert nxt.dtype == np.dtype(dtype) and not held.any() and (new['status'] == 0).all() and (new['naccepted'] == 1).all()
        A = F + new['lambda'].astype('f8')[:, None, None] * F * np.eye(ndim)
        want = np.linalg.solve(A, g[..., None])[..., 0]
        cond = np.linalg.cond(A).max()
        assert np.abs(nxt - want).max() <= 16 * cond * 2.3e-16 * np.abs(want).max(), dtype
        inv, info = lr.spd_inverse(F, dtype=dtype)
        assert not info.any() and np.array_equal(inv, inv.transpose(0, 2, 1))
        assert np.abs(inv - np.linalg.inv(F)).max() <= 16 * np.linalg.cond(F).max() * 2.3e-16 * np.abs(inv).max(), dtype
    A = (F + new['lambda'][:, None, None] * F * np.eye(ndim)).astype(LD)
    eps = float(np.finfo(LD).eps)
    assert np.abs(np.einsum('bij,bj->bi', A, nxt) - g).max() <= 16 * cond * eps * np.abs(g).max()
    assert np.abs(np.einsum('bij,bjk->bik', F.astype(LD), inv) - np.eye(ndim)).max() <= 16 * np.linalg.cond(F).max() * eps
    # a held parameter is out of the system: the others solve the reduced one
    if ndim > 1:
        state['x'][:, 0], state['gradient'][:, 0] = 1., np.abs(g[:, 0])
        lo, hi = np.full(ndim, -5.), np.full(ndim, 5.)
        hi[0] = 1.
        new, nxt, held = lr.step(state, trial, lo, hi, dtype=LD)
        assert held[:, 0].all() and not held[:, 1:].any() and (nxt[:, 0] == 1.).all()
        A = (F + new['lambda'].astype('f8')[:, None, None] * F * np.eye(ndim))[:, 1:, 1:]
        want = np.clip(np.linalg.solve(A, g[:, 1:, None])[..., 0], -5., 5.)
        assert np.abs(nxt[:, 1:] - want).max() <= 16 * np.linalg.cond(A).max() * 2.3e-16 * np.abs(want).max()


def expected_status(kind, before):
    return {'equal': 1, 'ftol': 1, 'first-bad': 3, 'lmax': 2, 'terminal': before, 'zero-diagonal': 3, 'indefinite': 3}.get(kind, 0)


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_levels_and_decisions_of_the_device_cases(ndim):
    worst, worst_ill = 0., 0.
    for B in lr.batch_sizes(ndim):
        state, trial, lo, hi, kinds = lr.make_case(ndim, B)
        new64, next64, held64 = lr.step(state, trial, lo, hi, dtype='f8', **lr.CONTROLS)
        newld, nextld, heldld = lr.step(state, trial, lo, hi, dtype=LD, **lr.CONTROLS)
        assert nextld.dtype == LD and next64.dtype == np.float64
        assert np.array_equal(new64['status'], newld['status']) and np.array_equal(new64['naccepted'], newld['naccepted']) and np.array_equal(held64, heldld), (ndim, B)
        assert np.array_equal(new64['lambda'], newld['lambda'].astype('f8'))
        assert [int(s) for s in new64['status']] == [expected_status(kind, int(before)) for kind, before in zip(kinds, state['status'])], (ndim, B)
        for b, kind in enumerate(kinds):      # what each kind is there for
            accepted = new64['naccepted'][b] == state['naccepted'][b] + 1
            assert accepted == (kind in ('half', 'equal', 'first', 'bounds', 'zero-diagonal', 'indefinite', 'ftol')), (kind, b)
            if kind == 'bounds':
                finite = [i for i in range(ndim) if np.isfinite(lo[i])][:4]
                assert [bool(h) for h in held64[b, finite]] == [True, False, True, False][:len(finite)] and held64[b].sum() == len(finite[::2])
            if kind == 'lmax':
                assert new64['lambda'][b] == 1e12
            if new64['status'][b] != 0:
                assert np.array_equal(next64[b], new64['x'][b])
        ill = np.array([kind == 'ill' for kind in kinds])
        if (~ill).any():
            worst = max(worst, lr.worst_level(nextld[~ill], next64[~ill]))
        if ill.any():
            worst_ill = max(worst_ill, lr.worst_level(nextld[ill], next64[ill]))
    print('ndim = %d: next at most %.3g floors from the truth, %.3g on the ill-conditioned fits' % (ndim, worst, worst_ill))
    assert worst <= LEVEL_CAP and worst_ill <= ILL_CAP
    worst, worst_ill = 0., 0.
    for B in lr.batch_sizes(ndim):
        A, failing = lr.make_matrices(ndim, B)
        inv64, info64 = lr.spd_inverse(A, 'f8')
        invld, infold = lr.spd_inverse(A, LD)
        assert np.array_equal(info64, infold) and {b: int(info64[b]) for b in np.flatnonzero(info64)} == failing, (ndim, B)
        good = info64 == 0
        assert np.isnan(inv64[~good]).all() and np.isfinite(inv64[good]).all()
        ill = np.arange(B) % 5 == 4
        if (good & ~ill).any():
            worst = max(worst, lr.worst_level(invld[good & ~ill], inv64[good & ~ill]))
        if (good & ill).any():
            worst_ill = max(worst_ill, lr.worst_level(invld[good & ill], inv64[good & ill]))
    print('ndim = %d: an inverse at most %.3g floors from the truth, %.3g on the ill-conditioned ones' % (ndim, worst, worst_ill))
    assert worst <= INVERSE_CAP and worst_ill <= ILL_INVERSE_CAP
