"""GPU: cp_lm_step and cp_spd_inverse (csrc/cp_lm.hip) against their restatement in tests/lm_reference.py, at the edges of the launch: ndim on both sides of
every count of lanes per fit, B one below, at and one above the fits per wave and per workgroup (from cp_lm_layout) and at three workgroups + 2.  Every
batch mixes the kinds of ``lm_reference.KINDS`` by construction.  ``status``, ``naccepted`` and the held set are compared exactly, ``lambda`` and the
copied state bit for bit, ``next`` and the inverses by the level rule (a block is one fit; 16 levels).  Around every output stand sentinels, the inputs are
compared with what was uploaded, every call is made twice on fresh copies of the state (the same bits), and a NaN in fit b reaches fit b only."""
import ctypes
import functools

import numpy as np
import pytest

import lm_reference as lr

pytestmark = pytest.mark.gpu
LD = np.longdouble
GUARD = 32
SENTINEL = {'f8': -7.25e77, 'i4': -123456789}


def layout_sizes(ndim):
    from cosmoprimo_amd import _lib
    G, per = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().cp_lm_layout(ndim, ctypes.byref(G), ctypes.byref(per)))
    per_wave, per_workgroup = 64 // G.value, per.value
    sizes = {per_wave - 1, per_wave, per_wave + 1, per_workgroup - 1, per_workgroup, per_workgroup + 1, 3 * per_workgroup + 2}
    return sorted(size for size in sizes if size > 0)


class Guarded(object):
    """An array on the device between two runs of sentinels."""

    def __init__(self, array):
        import torch
        array = np.ascontiguousarray(array)
        self.shape, self.kind = array.shape, 'i4' if array.dtype.kind == 'i' else 'f8'
        self.buffer = torch.full((array.size + 2 * GUARD,), SENTINEL[self.kind], dtype=torch.int32 if self.kind == 'i4' else torch.float64, device='cuda:0')
        self.buffer[GUARD:GUARD + array.size] = torch.as_tensor(array.reshape(-1).astype(self.kind), device='cuda:0')
        self.size = array.size

    def ptr(self):
        return self.buffer.data_ptr() + GUARD * self.buffer.element_size()

    def host(self):
        whole = self.buffer.cpu().numpy()
        assert (whole[:GUARD] == SENTINEL[self.kind]).all() and (whole[GUARD + self.size:] == SENTINEL[self.kind]).all(), 'a sentinel was overwritten'
        return whole[GUARD:GUARD + self.size].reshape(self.shape).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_step_once(state, trial, lo, hi, controls):
    import torch
    from cosmoprimo_amd import _lib
    B, n = state['x'].shape
    s = [Guarded(state[name]) for name in lr.STATE]
    t = [Guarded(trial[name]) for name in lr.TRIAL]
    bounds = [Guarded(lo), Guarded(hi)]
    out = Guarded(np.full((B, n), 123.))
    c = controls
    _lib.check(_lib.load().cp_lm_step(B, n, *[g.ptr() for g in s + t + bounds], c['up'], c['down'], c['lmin'], c['lmax'], c['ftol'], out.ptr(), 0,
                                      torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    for g, before in zip(t + bounds, [trial[name] for name in lr.TRIAL] + [lo, hi]):
        assert same_bits(g.host(), np.asarray(before, dtype='f8')), 'an input was written'
    return {name: g.host() for name, g in zip(lr.STATE, s)}, out.host()


def device_step(state, trial, lo, hi, controls=lr.CONTROLS):
    new, nxt = device_step_once(state, trial, lo, hi, controls)
    again, nxt2 = device_step_once(state, trial, lo, hi, controls)
    assert same_bits(nxt, nxt2) and all(same_bits(new[name], again[name]) for name in lr.STATE), 'two calls differ'
    return new, nxt


def device_inverse(A):
    import torch
    from cosmoprimo_amd import _lib
    B, n = A.shape[:2]
    results = []
    for call in range(2):
        a, inv, info = Guarded(A), Guarded(np.full(A.shape, 123.)), Guarded(np.full(B, 99, dtype='i4'))
        _lib.check(_lib.load().cp_spd_inverse(B, n, a.ptr(), inv.ptr(), info.ptr(), 0, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert same_bits(a.host(), A)
        results.append((inv.host(), info.host()))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])
    return results[0]


@functools.lru_cache(maxsize=None)
def case(ndim, B):
    """The batch and its restatements, computed once: (state, trial, lo, hi, kinds), (new, next, held) in float64 and in longdouble."""
    made = lr.make_case(ndim, B)
    return made, lr.step(*made[:4], dtype='f8', **lr.CONTROLS), lr.step(*made[:4], dtype=LD, **lr.CONTROLS)


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_step(ndim):
    sizes = layout_sizes(ndim)
    assert sizes == lr.batch_sizes(ndim)
    seen = set()
    for B in sizes:
        (state, trial, lo, hi, kinds), (new64, next64, held64), (newld, nextld, heldld) = case(ndim, B)
        seen.update(kinds)
        new, nxt = device_step(state, trial, lo, hi)
        what = 'ndim = %d, B = %d' % (ndim, B)
        assert np.array_equal(new['status'], new64['status']) and np.array_equal(new['naccepted'], new64['naccepted']), what
        assert new['status'].dtype == np.int32 and same_bits(new['lambda'], new64['lambda']), what
        for name in ('x', 'fisher', 'gradient', 'chi2'):      # copied where accepted, untouched elsewhere: the trial's or the state's bits
            assert same_bits(new[name], new64[name]), (what, name)
        frozen = state['status'] != 0
        assert all(same_bits(new[name][frozen], state[name][frozen]) for name in lr.STATE) and same_bits(nxt[frozen], state['x'][frozen])
        over = new['status'] != 0
        assert same_bits(nxt[over], new['x'][over]), what
        # the held set: a held parameter stays exactly where it is; a free one of a running fit moves (unless the box clips it back: as in the restatement)
        running = ~over
        assert same_bits(nxt[running][held64[running]], new['x'][running][held64[running]]) and np.array_equal(nxt == new['x'], next64 == new64['x']), what
        moved = (nxt != new['x'])[running]
        assert not moved[held64[running]].any() and moved[~held64[running]].sum() > 0.9 * moved[~held64[running]].size, what
        lr.assert_within(nxt, nextld, next64, what)
        assert (nxt >= lo).all() and (nxt <= hi).all()
        print('%s: next has the bits of the float64 restatement: %s' % (what, same_bits(nxt, next64)))
        ill = np.array([kind == 'ill' for kind in kinds])
        if ill.any() and ndim > 1:      # the rule still tells the reference from a neighbour at a condition number of 1e10
            lr.assert_within(next64[ill], nextld[ill], next64[ill], what + ', ill-conditioned, the restatement itself')
            other = dict(state, **{'lambda': state['lambda'] * 3.})
            neighbour = lr.step(other, trial, lo, hi, dtype='f8', **lr.CONTROLS)[1]
            with pytest.raises(AssertionError):
                lr.assert_within(neighbour[ill], nextld[ill], next64[ill], what + ', ill-conditioned, a step with three times the damping')
    assert seen == set(lr.KINDS) or max(sizes) < len(lr.KINDS)


@pytest.mark.parametrize('ndim', [1, 3, 8, 17, 32])
def test_a_nan_reaches_its_own_fit_only(ndim):
    B = max(layout_sizes(ndim))
    (state, trial, lo, hi, kinds), (new64, next64, held64), _ = case(ndim, B)
    clean, clean_next = device_step(state, trial, lo, hi)
    hit = [b for b, kind in enumerate(kinds) if kind in ('half', 'worse')][:2]      # an accepted trial with a NaN gradient, a state with a NaN matrix entry
    assert len(hit) == 2
    state, trial = {name: value.copy() for name, value in state.items()}, {name: value.copy() for name, value in trial.items()}
    trial['gradient'][hit[0], ndim - 1] = np.nan
    state['fisher'][hit[1], ndim - 1, 0] = np.nan
    new, nxt = device_step(state, trial, lo, hi)
    others = np.ones(B, dtype='?')
    others[hit] = False
    assert same_bits(nxt[others], clean_next[others]) and all(same_bits(new[name][others], clean[name][others]) for name in lr.STATE)
    assert np.isnan(nxt[hit[0]]).any() and new['status'][hit[0]] == 0 and new['naccepted'][hit[0]] == clean['naccepted'][hit[0]]
    assert new['status'][hit[1]] == 3 and same_bits(nxt[hit[1]], state['x'][hit[1]])      # the NaN meets a pivot
    want = lr.step(state, trial, lo, hi, dtype='f8', **lr.CONTROLS)
    assert np.array_equal(new['status'], want[0]['status']) and np.array_equal(np.isnan(nxt), np.isnan(want[1]))


def test_controls_and_an_open_box():
    """Other controls than the defaults, and a box that is open everywhere."""
    ndim, B = 5, 33
    state, trial, lo, hi, kinds = lr.make_case(ndim, B, seed=3)
    controls = dict(up=3., down=1., lmin=1e-3, lmax=1e3, ftol=0.6)
    big = np.full(ndim, np.inf)
    for bounds in ((lo, hi), (-big, big)):
        new, nxt = device_step(state, trial, *bounds, controls=controls)
        new64, next64, held64 = lr.step(state, trial, *bounds, dtype='f8', **controls)
        newld, nextld, heldld = lr.step(state, trial, *bounds, dtype=LD, **controls)
        assert np.array_equal(new64['status'], newld['status']) and np.array_equal(held64, heldld)
        assert np.array_equal(new['status'], new64['status']) and np.array_equal(new['naccepted'], new64['naccepted']) and same_bits(new['lambda'], new64['lambda'])
        assert (new['status'][[kind == 'half' for kind in kinds]] == 1).all()      # ftol = 0.6 takes a halved chi2 for converged
        lr.assert_within(nxt, nextld, next64, 'controls')


@functools.lru_cache(maxsize=None)
def matrices(ndim, B):
    A, failing = lr.make_matrices(ndim, B)
    return A, failing, lr.spd_inverse(A, 'f8'), lr.spd_inverse(A, LD)


@pytest.mark.parametrize('ndim', lr.NDIMS)
def test_inverse(ndim):
    for B in layout_sizes(ndim):
        A, failing, (inv64, info64), (invld, infold) = matrices(ndim, B)
        inv, info = device_inverse(A)
        what = 'inverse, ndim = %d, B = %d' % (ndim, B)
        assert info.dtype == np.int32 and np.array_equal(info, info64) and {b: int(info[b]) for b in np.flatnonzero(info)} == failing, what
        assert same_bits(inv, inv.transpose(0, 2, 1)), what
        good = info == 0
        assert np.isnan(inv[~good]).all() and np.isfinite(inv[good]).all(), what
        if good.any():
            lr.assert_within(inv[good], invld[good], inv64[good], what)
            print('%s: the bits of the float64 restatement: %s' % (what, same_bits(inv[good], inv64[good])))
