"""CPU: (a) Philox4x32-10 of tests/hmc_reference.py against its known answers, and the uniforms strictly inside (0, 1); (b) the argument checks of
cp_hmc_factor and cp_hmc_step, which come back by status, in the stated order, with the entry point's name in cp_last_error() before any device call (this
test runs without a device; the pointers are fakes nobody may read); (c) properties of the restatement itself: its substitutions are the halves of
``lm_reference.solve``, a trajectory run backwards comes back to its start, the energy error of a trajectory on a quadratic chi2 stays below the leapfrog
bound, and 1024 chains on a Gaussian posterior pass the statistic of tests/test_emulator_hmc_gpu.py at the bounds 1024 chains imply; (d) over every case of
tests/test_hmc_step_gpu.py: the same discrete decisions in float64 and in longdouble, no chain within the tie margin of its acceptance test, and the level
of every block below the cap recorded here."""
import ctypes

import numpy as np
import pytest

import hmc_reference as hr
import lm_reference as lr

LD = np.longdouble
FAKE = ctypes.c_void_p(8)
STEP_POINTERS = 20      # x, grad, chi2, status, naccepted, nout; z, h0, eps, out; xt, grad_t, chi2_t; factor, lo, hi, step; next, sample, sample_chi2
# Measured here over every case below: z at most 237 floors from the truth (ndim = 1: a block of one entry, r cos(angle) next to a zero of the cosine), next
# 9.98, h0 10.1, eps 1.89 (all three at ndim = 1 or 2), a sample 1 (it is copied), a factor 22.3 (ndim = 32).  The caps are the next powers of two.
LEVEL_CAP = {'z': 256., 'next': 16., 'h0': 16., 'eps': 2., 'sample': 1., 'factor': 32.}
# |H1 - h0| over (h0 - chi2_min / 2) of 6 x 0.25 trajectories on a quadratic chi2 under its own Fisher metric, 256 chains: at most 0.01581 measured
# (ndim = 2; 0.01558 at ndim = 3, 0.01484 at ndim = 8), the bound 0.01587.
ENERGY_BOUND = 0.25**2 / (4. * (1. - 0.25**2 / 4.))


def test_philox_known_answers():
    for counter, key, want in hr.KNOWN_ANSWERS:
        assert tuple(int(w) for w in hr.philox(counter, key)) == want
    # arrays of counters: each entry is its own stream
    w = hr.philox((np.arange(5), 0, 3, 16), (42, 0))
    assert all(tuple(int(v[b]) for v in w) == tuple(int(v) for v in hr.philox((b, 0, 3, 16), (42, 0))) for b in range(5))
    assert len({tuple(int(v[b]) for v in w) for b in range(5)}) == 5


@pytest.mark.parametrize('dtype', ['f8', LD])
def test_uniforms_strictly_inside(dtype):
    for wa in (0, 0xffffffff):
        for wb in (0, 0xffffffff):
            u = hr.uniform(wa, wb, dtype)
            assert u.dtype == np.dtype(dtype) and 0. < u < 1., (wa, wb, u)
    assert hr.uniform(0, 0, dtype) == 2.**-54 and hr.uniform(0xffffffff, 0xffffffff, dtype) == 1. - 2.**-53
    # the minimum binds for the largest integer alone: one below it the stated sum stands, in float64 rounded to even
    assert hr.uniform(0xffffffff, 0xffffffbf, 'f8') == 1. - 2.**-52 and hr.uniform(0xffffffff, 0xffffffbf, LD) == LD(1.) - LD(1.5) * LD(2.)**-53
    z = hr.normals(7, np.arange(64), 3, 5)
    assert np.isfinite(z).all() and np.isfinite(hr.jitter_and_energy(7, np.arange(64), 3)[1]).all()


def factor_call(B=4, ndim=3, pointers=None):
    from cosmoprimo_amd import _lib
    p = [FAKE] * 3 if pointers is None else pointers
    return _lib.load().cp_hmc_factor(B, ndim, p[0], p[1], p[2], 0, None)


def step_call(B=4, ndim=3, pointers=None, t_close=-1, t_open=-1, jitter=0.1, seed=0):
    from cosmoprimo_amd import _lib
    p = [FAKE] * STEP_POINTERS if pointers is None else pointers
    return _lib.load().cp_hmc_step(B, ndim, t_close, t_open, *p[:17], jitter, seed, *p[17:], 0, None)


@pytest.mark.parametrize('call,npointers,name', [(step_call, STEP_POINTERS, b'cp_hmc_step'), (factor_call, 3, b'cp_hmc_factor')], ids=['step', 'factor'])
def test_argument_checks_come_before_any_device_call(call, npointers, name):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    named = lambda words: name in lib.cp_last_error() and words in lib.cp_last_error()      # noqa: E731
    none = [None] * npointers
    assert call(B=-1) == _lib.CP_EINVAL and named(b'chains') and call(ndim=0) == _lib.CP_EINVAL and named(b'chains') and call(ndim=-3) == _lib.CP_EINVAL
    assert call(ndim=33) == _lib.CP_EUNSUPPORTED and named(b'at most 32')
    with pytest.raises(NotImplementedError):
        _lib.check(call(ndim=33))
    # the order: the counts before the cap of ndim, that before the cap of B, that before B = 0, that before the pointers
    assert call(B=-1, ndim=33) == _lib.CP_EINVAL and call(B=-1, ndim=33, pointers=none) == _lib.CP_EINVAL and named(b'chains')
    assert call(B=2**62, ndim=33) == _lib.CP_EUNSUPPORTED and named(b'at most 32')
    assert call(B=0, ndim=33, pointers=none) == _lib.CP_EUNSUPPORTED and call(B=0, ndim=0) == _lib.CP_EINVAL
    for ndim in (1, 2, 3, 8, 9, 17, 32):      # the cap of B: 2^31 - 1 workgroups; the largest count is refused only for its null pointers
        most = (2**31 - 1) * hr.lanes(ndim)[2]
        assert call(B=most + 1, ndim=ndim) == _lib.CP_EUNSUPPORTED and named(b'workgroups'), ndim
        assert call(B=most + 1, ndim=ndim, pointers=none) == _lib.CP_EUNSUPPORTED
        assert call(B=most, ndim=ndim, pointers=none) == _lib.CP_EINVAL and named(b'null pointer'), ndim
    assert call(B=0) == _lib.CP_OK and call(B=0, pointers=none) == _lib.CP_OK
    for k in range(npointers):
        assert call(pointers=[None if j == k else FAKE for j in range(npointers)]) == _lib.CP_EINVAL and named(b'null pointer'), k


def test_the_trajectory_numbers_the_sample_pointers_and_the_jitter():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    named = lambda words: b'cp_hmc_step' in lib.cp_last_error() and words in lib.cp_last_error()      # noqa: E731
    none = [None] * STEP_POINTERS
    # a trajectory number of 2^32 or more: after the cap of B, before B = 0 and before the pointers
    for flags in (dict(t_close=2**32), dict(t_open=2**32), dict(t_close=2**40, t_open=3), dict(t_close=2**32, pointers=none), dict(t_open=2**32, B=0)):
        assert step_call(**flags) == _lib.CP_EUNSUPPORTED and named(b'2^32'), flags
    assert step_call(t_close=2**32, ndim=33) == _lib.CP_EUNSUPPORTED and named(b'at most 32')
    assert step_call(t_close=2**32, B=-1) == _lib.CP_EINVAL
    assert step_call(t_close=2**32, B=(2**31 - 1) * hr.lanes(3)[2] + 1) == _lib.CP_EUNSUPPORTED and named(b'workgroups')
    assert step_call(t_close=2**32 - 1, t_open=2**32 - 1, pointers=none) == _lib.CP_EINVAL and named(b'null pointer')
    assert step_call(t_close=-5, t_open=-2**40, pointers=none) == _lib.CP_EINVAL and named(b'null pointer')      # < 0: no close, no open
    # the two sample pointers may be null together, and only together
    both = [FAKE] * 18 + [None, None]
    assert step_call(B=0, pointers=both) == _lib.CP_OK
    assert step_call(pointers=both, jitter=2.) == _lib.CP_EINVAL and named(b'jitter')      # past the pointers: refused for its jitter
    for one in ([FAKE] * 18 + [None, FAKE], [FAKE] * 18 + [FAKE, None]):
        assert step_call(pointers=one, jitter=2.) == _lib.CP_EINVAL and named(b'null pointer')
    # 0 <= jitter < 1 and not a NaN, after the pointers, B = 0 before both
    for jitter in (-0.1, 1., 1.5, float('nan'), float('inf')):
        assert step_call(jitter=jitter) == _lib.CP_EINVAL and named(b'jitter'), jitter
        assert step_call(jitter=jitter, pointers=none) == _lib.CP_EINVAL and named(b'null pointer')
        assert step_call(jitter=jitter, B=0, pointers=none) == _lib.CP_OK
    with pytest.raises(ValueError):
        _lib.check(step_call(jitter=1.))


@pytest.mark.parametrize('ndim', [1, 2, 5, 16, 32])
def test_substitutions_are_the_halves_of_the_solve(ndim):
    rng = np.random.default_rng(ndim)
    B = 6
    metric = np.stack([lr.spd(rng, ndim) for b in range(B)])
    r = rng.standard_normal((B, ndim))
    for dtype in ('f8', LD):
        L, status = hr.factor(metric, np.zeros(B, dtype='i4'), dtype)
        assert L.dtype == np.dtype(dtype) and not status.any() and (np.triu(L, 1) == 0).all()
        both = hr.backward(L, hr.forward(L, r.astype(dtype)))
        assert np.array_equal(both, lr.solve(L, r.astype(dtype)))      # (the same values: a longdouble has padding bytes)
        assert np.abs(np.einsum('bij,bkj->bik', L, L) - metric).max() <= 64 * np.finfo(dtype).eps * np.abs(metric).max()
    bad = metric.copy()
    bad[1, ndim - 1, ndim - 1] *= -1.
    assert list(hr.factor(bad, np.array([0, 0, 1, 0, 2, 0], dtype='i4'))[1]) == [0, 3, 1, 0, 2, 0]


def leapfrog_there_and_back(model, B, dtype, seed=5, nleapfrog=6, step_size=0.25):
    """(start, back, drawn z, z at the end of the way back, h0, H1 - h0 of the way there) of B trajectories with jitter = 0 in ``dtype``, through
    :func:`hmc_reference.step` alone.  The way back: the momentum negated, half a kick by a close, a drift by an inner step under a zero gradient, then
    whole steps and the close's half kick."""
    rng = np.random.default_rng(seed)
    lo, hi = model.limits(1e3)
    sd = np.sqrt(np.diag(np.linalg.inv(model.fisher)))
    start = model.mode + sd * rng.standard_normal((B, model.ndim))
    evaluate = lambda x: tuple(np.asarray(v).astype(dtype) for v in model.evaluate(np.asarray(x).astype(LD)))      # noqa: E731
    fisher, g, chi = evaluate(start)
    zero = np.zeros(B, dtype='i4')
    state = dict(x=start.astype(dtype), gradient=g, chi2=chi, status=zero, naccepted=zero, nout=zero, z=np.zeros((B, model.ndim), dtype=dtype), h0=np.zeros(B, dtype=dtype),
                 eps=np.zeros(B, dtype=dtype), out=zero)
    L = hr.factor(fisher, zero, dtype)[0]
    go = lambda state, x, gradient=None, **kwargs: hr.step(state, dict(zip(hr.TRIAL, (x,) + (evaluate(x)[1:] if gradient is None else (gradient, evaluate(x)[2])))),  # noqa: E731
                                                           L, lo, hi, step_size, jitter=0., seed=seed, dtype=dtype, **kwargs)
    state, x, extra = go(state, state['x'], t_open=0)
    drawn, h0 = hr.normals(seed, np.arange(B), 0, model.ndim, dtype), state['h0']
    for leap in range(nleapfrog - 1):
        state, x, extra = go(state, x)
    end = x
    state['h0'] = np.full(B, np.inf, dtype=dtype)      # accepted whatever e is
    state, x, extra = go(state, end, t_close=0)
    assert extra['accept'].all() and not state['out'].any()
    energy = 0.5 * state['chi2'] + 0.5 * hr.squares(state['z']) - h0
    state['z'] = -state['z']
    state, x, extra = go(state, end, t_close=1)      # half a kick
    state, x, extra = go(state, end, gradient=np.zeros_like(state['z']))      # a drift
    for leap in range(nleapfrog - 1):
        state, x, extra = go(state, x)
    back = x
    state, x, extra = go(state, back, t_close=2)
    return start, back, drawn, state['z'], h0, energy


@pytest.mark.parametrize('ndim', [2, 3, 8])
def test_a_trajectory_is_reversible_and_keeps_its_energy(ndim):
    model = hr.LinearModel(ndim)
    B = 256
    start, back64, drawn64, z64, h0, energy = leapfrog_there_and_back(model, B, 'f8')
    start, backld, drawnld, zld, h0ld, energyld = leapfrog_there_and_back(model, B, LD)
    assert np.abs(backld - start).max() < 1e-16 * np.abs(start).max()      # the truth comes back as far as longdouble goes
    hr.assert_levels(start, backld, back64, 'ndim = %d: back at the start' % ndim)
    hr.assert_levels(-drawn64, -drawnld, z64, 'ndim = %d: the momentum back at the start, negated' % ndim)
    print('ndim = %d: back at most %.3g floors from the start' % (ndim, hr.worst_level(backld, back64)))
    # the leapfrog bound on a quadratic chi2 under its own Fisher metric: |H1 - h0| <= eps^2 / (4 (1 - eps^2 / 4)) (h0 - chi2_min / 2)
    above = h0 - 0.5 * model.evaluate(model.mode[None])[2]
    assert (above > 0).all()
    ratio = float((np.abs(energy) / above).max())
    print('ndim = %d: |H1 - h0| at most %.4g of the energy above the mode (bound %.4g)' % (ndim, ratio, ENERGY_BOUND))
    assert ratio <= ENERGY_BOUND and ratio > 1e-6


@pytest.mark.parametrize('ndim', [2, 3])
def test_exactness_of_the_restatement(ndim):
    """The statistic of tests/test_emulator_hmc_gpu.py::test_exactness on the restatement alone, with 1024 chains: 5 / sqrt(B) = 0.156 and 5 sqrt(2 / B) = 0.221."""
    model = hr.LinearModel(ndim)
    B = 1024
    lo, hi = model.limits()
    samples, chi2, state = hr.run(model.evaluate, np.tile(model.mode, (B, 1)), lo, hi, nsamples=1, nwarmup=20, seed=42)
    assert not state['nout'].any() and not state['status'].any()
    w = model.whiten(samples[0])
    mean, cov = w.mean(axis=0), np.cov(w.T, bias=True)
    acceptance = state['naccepted'].mean() / 21.
    print('ndim = %d: |mean| at most %.3f, covariance at most %.3f from the identity, acceptance %.3f' % (ndim, np.abs(mean).max(), np.abs(cov - np.eye(ndim)).max(), acceptance))
    assert np.abs(mean).max() < 5. / np.sqrt(B) and np.abs(cov - np.eye(ndim)).max() < 5. * np.sqrt(2. / B) and acceptance > 0.9
    again = hr.run(model.evaluate, np.tile(model.mode, (B, 1)), lo, hi, nsamples=1, nwarmup=20, seed=42)[0]
    other = hr.run(model.evaluate, np.tile(model.mode, (B, 1)), lo, hi, nsamples=1, nwarmup=20, seed=43)[0]
    assert again.tobytes() == samples.tobytes() and not np.array_equal(other, samples)
    assert np.array_equal(chi2[0], model.evaluate(samples[0])[2])


def expected(kind, flags, before, e):
    """(status, accepted, nout + 1) of a chain of ``kind`` under ``flags``."""
    closing, opening = (value is not None for value in hr.FLAGS[flags])
    status = {'frozen': before, 'bad-pivot': 3}.get(kind, 3 if kind == 'bad-step' and opening else 0)
    running = kind not in ('frozen', 'bad-pivot')
    accepted = closing and running and (kind in ('accept', 'leave', 'bad-step') or (kind == 'coin' and e > 0.7))
    return status, accepted, closing and kind == 'out'


@pytest.mark.parametrize('ndim', hr.NDIMS)
def test_levels_and_decisions_of_the_device_cases(ndim):
    worst = dict.fromkeys(LEVEL_CAP, 0.)
    seen = set()
    for B in hr.batch_sizes(ndim):
        state, trial, metric, lo, hi, step_size, kinds = hr.make_case(ndim, B, seed=ndim)
        seen.update(kinds)
        (L64, status64), (Lld, statusld) = hr.factor(metric, state['status'], 'f8'), hr.factor(metric, state['status'], LD)
        assert np.array_equal(status64, statusld) and [s == 3 for s in status64] == [kind == 'bad-pivot' or (kind == 'frozen' and s == 3) for kind, s in zip(kinds, status64)]
        good = status64 != 3
        if good.any():
            worst['factor'] = max(worst['factor'], hr.worst_level(Lld[good], L64[good]))
        state = dict(state, status=status64)
        for flags, (t_close, t_open) in hr.FLAGS.items():
            what = (ndim, B, flags)
            new64, next64, extra64 = hr.step(state, trial, L64, lo, hi, step_size, t_close, t_open, hr.JITTER, hr.SEED, 'f8')
            newld, nextld, extrald = hr.step(state, trial, L64, lo, hi, step_size, t_close, t_open, hr.JITTER, hr.SEED, LD)
            assert nextld.dtype == LD and next64.dtype == np.float64
            assert all(np.array_equal(new64[name], newld[name]) for name in hr.INTEGERS) and np.array_equal(extra64['accept'], extrald['accept']), what
            # the tie condition: no chain within 1e-9 max(1, |h0|, |H1|) of its acceptance test, in the truth
            decided = ~np.isnan(extrald['margin'])
            assert np.array_equal(decided, ~np.isnan(extra64['margin']))
            assert not (np.abs(extrald['margin'][decided]) <= 1e-9 * extrald['scale'][decided]).any(), what
            e = hr.jitter_and_energy(hr.SEED, np.arange(B), t_close, 'f8')[1] if t_close is not None else np.zeros(B)
            for b, kind in enumerate(kinds):      # what each kind is there for
                status, accepted, counted = expected(kind, flags, int(state['status'][b]), e[b])
                assert (int(new64['status'][b]), bool(extra64['accept'][b]), int(new64['nout'][b] - state['nout'][b])) == (status, accepted, int(counted)), (what, kind, b)
                assert new64['naccepted'][b] == state['naccepted'][b] + int(accepted)
                if flags in ('inner', 'open') and new64['status'][b] == 0:
                    assert new64['out'][b] == int(kind in ('leave', 'nan-gradient' if flags == 'inner' else None) or (kind == 'out' and flags == 'inner')), (what, kind, b)
                if new64['status'][b] != 0 or (new64['out'][b] and flags != 'inner'):
                    assert np.array_equal(next64[b], new64['x'][b])
            assert (next64[np.isfinite(next64).all(axis=1)] >= lo).all() and (next64[np.isfinite(next64).all(axis=1)] <= hi).all()
            for name, f8, ld in (('z', new64['z'], newld['z']), ('next', next64, nextld), ('h0', new64['h0'], newld['h0']), ('eps', new64['eps'], newld['eps'])):
                worst[name] = max(worst[name], hr.worst_level(ld, f8))
            if t_close is not None:
                worst['sample'] = max(worst['sample'], hr.worst_level(extrald['sample'], extra64['sample']))
                assert np.array_equal(extra64['sample'], new64['x'] if t_open is None else extra64['sample']) and np.array_equal(extra64['sample_chi2'], new64['chi2'])
    print('ndim = %d: floors from the truth at most %s' % (ndim, ', '.join('%s %.3g' % item for item in worst.items())))
    assert all(worst[name] <= LEVEL_CAP[name] for name in worst), worst
    assert seen == set(hr.KINDS) or max(hr.batch_sizes(ndim)) < len(hr.KINDS)
