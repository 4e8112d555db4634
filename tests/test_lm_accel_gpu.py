"""GPU: cp_lm_step_velocity and cp_lm_accelerate (csrc/cp_lm.hip) against their restatement in tests/lm_accel_reference.py, at the edges of the launch: ndim on
both sides of every count of lanes per fit, B one below, at and one above the fits per wave and per workgroup and at three workgroups + 2.  Around every
output stand sentinels, the inputs are compared with what was uploaded, every call is made twice on fresh copies (the same bits).
cp_lm_step_velocity, on the cases of ``lm_reference.make_case``: the state and ``next`` bits of cp_lm_step, ``velocity`` by the level rule and exactly 0 where
nothing moves.  cp_lm_accelerate, on the cases of ``lm_accel_reference.make_case`` (every batch mixes its KINDS): the counter and the set of fits that take
the correction exactly, ``next`` by the level rule (a block is one fit; 16 levels), a fit that does not take it the bits of the plain step -- of the
restatement, and of cp_lm_step itself when the two launches are chained on the device --, a fit that is over the bits of ``x``, a held parameter exactly on
its bound, and a NaN in fit b reaches fit b only."""
import functools

import numpy as np
import pytest

import lm_accel_reference as la
import lm_reference as lr
from test_lm_step_gpu import Guarded, device_step, layout_sizes, same_bits

pytestmark = pytest.mark.gpu
LD = np.longdouble
COUNTER = 5      # where the counters start


def device_step_velocity_once(state, trial, lo, hi, controls):
    import torch
    from cosmoprimo_amd import _lib
    B, n = state['x'].shape
    s = [Guarded(state[name]) for name in lr.STATE]
    t = [Guarded(trial[name]) for name in lr.TRIAL]
    bounds = [Guarded(lo), Guarded(hi)]
    out, velocity = Guarded(np.full((B, n), 123.)), Guarded(np.full((B, n), 321.))
    c = controls
    _lib.check(_lib.load().cp_lm_step_velocity(B, n, *[g.ptr() for g in s + t + bounds], c['up'], c['down'], c['lmin'], c['lmax'], c['ftol'], out.ptr(), velocity.ptr(), 0,
                                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for g, before in zip(t + bounds, [trial[name] for name in lr.TRIAL] + [lo, hi]):
        assert same_bits(g.host(), np.asarray(before, dtype='f8')), 'an input was written'
    return {name: g.host() for name, g in zip(lr.STATE, s)}, out.host(), velocity.host()


def device_step_velocity(state, trial, lo, hi, controls=lr.CONTROLS):
    first, again = (device_step_velocity_once(state, trial, lo, hi, controls) for call in range(2))
    assert same_bits(first[1], again[1]) and same_bits(first[2], again[2]) and all(same_bits(first[0][name], again[0][name]) for name in lr.STATE), 'two calls differ'
    return first


def device_accelerate_once(state, v, h, lo, hi, alpha):
    import torch
    from cosmoprimo_amd import _lib
    B, n = state['x'].shape
    before = [state[name] for name in la.ACCEL] + [lo, hi, v, h]
    read = [Guarded(array) for array in before]
    out, counter = Guarded(np.full((B, n), 123.)), Guarded(np.full(B, COUNTER, dtype='i4'))
    _lib.check(_lib.load().cp_lm_accelerate(B, n, *[g.ptr() for g in read], alpha, out.ptr(), counter.ptr(), 0, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for g, array in zip(read, before):
        assert same_bits(g.host(), np.ascontiguousarray(array, dtype='i4' if np.asarray(array).dtype.kind == 'i' else 'f8')), 'an input was written'
    return out.host(), counter.host()


def device_accelerate(state, v, h, lo, hi, alpha=la.ALPHA):
    first, again = (device_accelerate_once(state, v, h, lo, hi, alpha) for call in range(2))
    assert same_bits(first[0], again[0]) and same_bits(first[1], again[1]), 'two calls differ'
    assert first[1].dtype == np.int32 and ((first[1] == COUNTER) | (first[1] == COUNTER + 1)).all()
    return first[0], first[1] == COUNTER + 1


@functools.lru_cache(maxsize=None)
def step_case(ndim, B):
    made = lr.make_case(ndim, B)
    return made, la.step_velocity(*made[:4], dtype='f8', **lr.CONTROLS), la.step_velocity(*made[:4], dtype=LD, **lr.CONTROLS)


@functools.lru_cache(maxsize=None)
def accelerate_case(ndim, B):
    made = la.make_case(ndim, B)
    return made, la.accelerate(*made[:5], dtype='f8'), la.accelerate(*made[:5], dtype=LD)


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_step_velocity(ndim):
    sizes = layout_sizes(ndim)
    assert sizes == lr.batch_sizes(ndim)
    for B in sizes:
        (state, trial, lo, hi, kinds), (new64, next64, held64, v64), (newld, nextld, heldld, vld) = step_case(ndim, B)
        what = 'step_velocity, ndim = %d, B = %d' % (ndim, B)
        plain, plain_next = device_step(state, trial, lo, hi)
        new, nxt, v = device_step_velocity(state, trial, lo, hi)
        assert same_bits(nxt, plain_next) and all(same_bits(new[name], plain[name]) for name in lr.STATE), what
        assert np.array_equal(new['status'], new64['status']), what
        running = new['status'] == 0
        assert np.array_equal(v == 0, v64 == 0) and (v[~running] == 0).all() and (v[held64] == 0).all(), what
        moved = np.where(new['x'] + v < lo, lo, np.where(new['x'] + v > hi, hi, new['x'] + v))      # next is x + velocity, clipped, where the fit runs
        assert same_bits(nxt[running], moved[running]), what
        lr.assert_within(v, vld, v64, what)
        print('%s: velocity has the bits of the float64 restatement: %s' % (what, same_bits(v, v64)))


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_accelerate(ndim):
    seen = set()
    for B in layout_sizes(ndim):
        (state, v, h, lo, hi, kinds), (next64, taken64), (nextld, takenld) = accelerate_case(ndim, B)
        seen.update(kinds)
        what = 'accelerate, ndim = %d, B = %d' % (ndim, B)
        nxt, taken = device_accelerate(state, v, h, lo, hi)
        assert np.array_equal(taken, taken64) and np.array_equal(taken64, takenld), what
        lr.assert_within(nxt, nextld, next64, what)
        assert (nxt >= lo).all() and (nxt <= hi).all(), what
        plain = state['x'] + v
        plain = np.where(plain < lo, lo, np.where(plain > hi, hi, plain))
        x = state['x']
        held = (state['status'] == 0)[:, None] & (((x >= hi) & (state['gradient'] > 0)) | ((x <= lo) & (state['gradient'] < 0)))
        plain = np.where(held, x, plain)
        kind = np.array(kinds)
        over = (state['status'] != 0) | (kind == 'pivot')
        assert same_bits(nxt[over], x[over]) and not taken[over].any(), what      # finished, or a failing pivot: x, the counter untouched
        assert same_bits(nxt[~taken & ~over], plain[~taken & ~over]), what      # refused or not finite: the plain step
        assert same_bits(nxt[held], x[held]) and held[kind == 'bounds'].any(axis=1).all(), what      # a held parameter stays exactly on its bound
        crossing = kind == 'cross'
        assert np.isin(nxt[crossing, 0], (lo[0], hi[0])).all(), what      # clipped to the bound exactly
        print('%s: next has the bits of the float64 restatement: %s' % (what, same_bits(nxt, next64)))
    assert seen == set(la.KINDS) or max(layout_sizes(ndim)) < len(la.KINDS)


@pytest.mark.parametrize('ndim', [1, 3, 8, 17, 32])
def test_chained_on_the_device(ndim):
    """cp_lm_step_velocity, then cp_lm_accelerate on what it left: the fits that do not take the correction hold the bits of cp_lm_step's ``next``."""
    B = max(layout_sizes(ndim))
    (state, v64, h, lo, hi, kinds), (next64, taken64), _ = accelerate_case(ndim, B)
    before = dict(state, chi2=np.full(B, np.inf), naccepted=np.zeros(B, dtype='i4'))      # nothing accepted yet: the trial is accepted as it is, lambda stays
    trial = dict(x=state['x'], fisher=state['fisher'], gradient=state['gradient'], chi2=np.ones(B))
    after, plain_next = device_step(before, trial, lo, hi)
    again, nxt0, v = device_step_velocity(before, trial, lo, hi)
    assert same_bits(nxt0, plain_next) and all(same_bits(after[name], again[name]) for name in lr.STATE)
    kind = np.array(kinds)
    assert all(same_bits(after[name], state[name]) for name in ('x', 'fisher', 'gradient', 'lambda')) and (after['status'][kind == 'pivot'] == 3).all()
    nxt, taken = device_accelerate(after, v, h, lo, hi)
    assert np.array_equal(taken, taken64) and taken.any() and not taken.all()
    assert same_bits(nxt[~taken], plain_next[~taken])
    over = after['status'] != 0
    assert same_bits(nxt[over], after['x'][over]) and not taken[over].any()
    moving = taken & np.array([k in ('pass', 'bounds', 'ill') for k in kinds])
    assert (nxt[moving] != plain_next[moving]).any(axis=1).all()


@pytest.mark.parametrize('ndim', [1, 3, 8, 17, 32])
def test_a_nan_reaches_its_own_fit_only(ndim):
    B = max(layout_sizes(ndim))
    (state, v, h, lo, hi, kinds), (next64, taken64), _ = accelerate_case(ndim, B)
    clean, clean_taken = device_accelerate(state, v, h, lo, hi)
    hit = [b for b, kind in enumerate(kinds) if kind in ('pass', 'zero-h', 'ill')][:3]      # a NaN curvature, a NaN velocity, a NaN matrix entry
    assert len(hit) == 3
    state = {name: value.copy() for name, value in state.items()}
    v, h = v.copy(), h.copy()
    h[hit[0], ndim - 1] = np.nan
    v[hit[1], 0] = np.nan
    state['fisher'][hit[2], ndim - 1, 0] = np.nan
    nxt, taken = device_accelerate(state, v, h, lo, hi)
    others = np.ones(B, dtype='?')
    others[hit] = False
    assert same_bits(nxt[others], clean[others]) and np.array_equal(taken[others], clean_taken[others])
    assert not taken[hit].any()
    assert np.isfinite(nxt[hit[0]]).all() and np.isnan(nxt[hit[1], 0]) and same_bits(nxt[hit[2]], state['x'][hit[2]])      # refused; the plain step; a pivot
    want, want_taken = la.accelerate(state, v, h, lo, hi, dtype='f8')
    assert np.array_equal(taken, want_taken) and np.array_equal(np.isnan(nxt), np.isnan(want))


def test_alpha_and_an_open_box():
    """Another alpha than the default turns refusals into corrections, and a box that is open everywhere holds nothing."""
    ndim, B = 5, 33
    state, v, h, lo, hi, kinds = la.make_case(ndim, B, seed=3)
    big = np.full(ndim, np.inf)
    for bounds in ((lo, hi), (-big, big)):
        for alpha in (la.ALPHA, 2.):      # the kind 'refuse' sits at 3 times the default gate: 4 sa = 3 x 0.75^2 sv < 2^2 sv
            nxt, taken = device_accelerate(state, v, h, *bounds, alpha=alpha)
            next64, taken64 = la.accelerate(state, v, h, *bounds, alpha=alpha, dtype='f8')
            nextld, takenld = la.accelerate(state, v, h, *bounds, alpha=alpha, dtype=LD)
            assert np.array_equal(taken, taken64) and np.array_equal(taken64, takenld)
            assert taken[[kind == 'refuse' for kind in kinds]].all() == (alpha == 2.)
            lr.assert_within(nxt, nextld, next64, 'alpha = %g' % alpha)
