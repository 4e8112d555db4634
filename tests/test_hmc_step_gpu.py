"""GPU: cp_hmc_factor and cp_hmc_step (csrc/cp_hmc.hip) through ``hmc_factor`` and ``hmc_step`` against their restatement in tests/hmc_reference.py, at the edges
of the launch: ndim on both sides of every count of lanes per chain, B = 1, the chains of a workgroup (from cp_lm_layout) and one more, each of the four
combinations of closing and opening a trajectory, with and without the sample pointers.  Every batch mixes the kinds of ``hmc_reference.KINDS`` by
construction.  Accept, ``out``, ``status``, ``naccepted`` and ``nout`` are compared exactly, the state copied on acceptance and a frozen chain's buffers bit for
bit, ``z``, ``h0``, ``eps``, ``next`` and ``sample`` by the level rule (a block is one chain; 16 levels).  Around every buffer the kernel writes stand sentinels,
the inputs are compared with what was uploaded, every call is made twice on fresh copies (the same bits), and the first chains of a longer batch are the
chains of a shorter one bit for bit.  tests/test_hmc_host.py holds the tie condition of these cases: no chain decides within 1e-9 of its threshold."""
import ctypes
import functools

import numpy as np
import pytest

import hmc_reference as hr

pytestmark = pytest.mark.gpu
LD = np.longdouble
GUARD = 32
SENTINEL = {'f8': -7.25e77, 'i4': -123456789}
WRITTEN = hr.STATE + hr.TRAJECTORY


def layout_sizes(ndim):
    from cosmoprimo_amd import _lib
    G, per = ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().cp_lm_layout(ndim, ctypes.byref(G), ctypes.byref(per)))
    return sorted({1, per.value, per.value + 1})


class Guarded(object):
    """A contiguous device tensor (``view``) between two runs of sentinels."""

    def __init__(self, array):
        import torch
        array = np.ascontiguousarray(array)
        self.shape, self.kind, self.size = array.shape, 'i4' if array.dtype.kind == 'i' else 'f8', array.size
        self.buffer = torch.full((array.size + 2 * GUARD,), SENTINEL[self.kind], dtype=torch.int32 if self.kind == 'i4' else torch.float64, device='cuda:0')
        self.view = self.buffer[GUARD:GUARD + array.size].view(self.shape)
        self.view.copy_(torch.as_tensor(array.astype(self.kind), device='cuda:0'))

    def host(self):
        whole = self.buffer.cpu().numpy()
        assert (whole[:GUARD] == SENTINEL[self.kind]).all() and (whole[GUARD + self.size:] == SENTINEL[self.kind]).all(), 'a sentinel was overwritten'
        return whole[GUARD:GUARD + self.size].reshape(self.shape).copy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device_step_once(state, trial, L, lo, hi, step_size, flags, with_sample=True):
    """(new state, next, sample, sample_chi2) of one ``hmc_step``; the sample buffers hold 123. where the kernel does not write them."""
    import torch
    from cosmoprimo_amd.emulators.tools import hmc_step
    B, n = state['x'].shape
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype='f8'), device='cuda:0')      # noqa: E731
    s = {name: Guarded(state[name]) for name in WRITTEN}
    t = {name: up(trial[name]) for name in hr.TRIAL}
    read = [up(a) for a in (L, lo, hi, step_size)]
    sample, sample_chi2 = Guarded(np.full((B, n), 123.)), Guarded(np.full(B, 123.))
    t_close, t_open = hr.FLAGS[flags]
    nxt = hmc_step({name: g.view for name, g in s.items()}, t, *read, t_close=t_close, t_open=t_open, jitter=hr.JITTER, seed=hr.SEED,
                   sample=sample.view if with_sample else None, sample_chi2=sample_chi2.view if with_sample else None)
    torch.cuda.synchronize()
    assert tuple(nxt.shape) == (B, n) and nxt.dtype == torch.float64
    for tensor, before in zip(list(t.values()) + read, [trial[name] for name in hr.TRIAL] + [L, lo, hi, step_size]):
        assert same_bits(tensor.cpu().numpy(), np.ascontiguousarray(before, dtype='f8')), 'an input was written'
    return {name: g.host() for name, g in s.items()}, nxt.cpu().numpy(), sample.host(), sample_chi2.host()


def device_step(state, trial, L, lo, hi, step_size, flags):
    """Two calls with the sample pointers (the same bits) and one without (the same bits but for the samples, which stay untouched)."""
    new, nxt, sample, sample_chi2 = device_step_once(state, trial, L, lo, hi, step_size, flags)
    again = device_step_once(state, trial, L, lo, hi, step_size, flags)
    assert all(same_bits(new[name], again[0][name]) for name in WRITTEN) and all(same_bits(a, b) for a, b in zip((nxt, sample, sample_chi2), again[1:])), 'two calls differ'
    without = device_step_once(state, trial, L, lo, hi, step_size, flags, with_sample=False)
    assert all(same_bits(new[name], without[0][name]) for name in WRITTEN) and same_bits(nxt, without[1]), 'the sample pointers change the step'
    assert (without[2] == 123.).all() and (without[3] == 123.).all()
    return new, nxt, sample, sample_chi2


@functools.lru_cache(maxsize=None)
def case(ndim, B):
    """The batch (its status as cp_hmc_factor leaves it) and its factors in float64, computed once."""
    state, trial, metric, lo, hi, step_size, kinds = hr.make_case(ndim, B, seed=ndim)
    L, status = hr.factor(metric, state['status'], 'f8')
    return dict(state, status=status), trial, metric, L, lo, hi, step_size, kinds, state['status']


@functools.lru_cache(maxsize=None)
def restated(ndim, B, flags):
    state, trial, metric, L, lo, hi, step_size, kinds, before = case(ndim, B)
    t_close, t_open = hr.FLAGS[flags]
    return tuple(hr.step(state, trial, L, lo, hi, step_size, t_close, t_open, hr.JITTER, hr.SEED, dtype) for dtype in ('f8', LD))


@pytest.mark.parametrize('ndim', hr.NDIMS)
def test_factor(ndim):
    import torch
    from cosmoprimo_amd.emulators.tools import hmc_factor
    sizes = layout_sizes(ndim)
    assert sizes == hr.batch_sizes(ndim)
    for B in sizes:
        state, trial, metric, L64, lo, hi, step_size, kinds, before = case(ndim, B)
        Lld = hr.factor(metric, before, LD)[0]
        results = []
        for call in range(2):
            status, m = Guarded(before), torch.as_tensor(metric, device='cuda:0')
            L = hmc_factor(m, status.view)
            torch.cuda.synchronize()
            assert same_bits(m.cpu().numpy(), metric)
            results.append((L.cpu().numpy(), status.host()))
        assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])
        L, status = results[0]
        what = 'factor, ndim = %d, B = %d' % (ndim, B)
        assert status.dtype == np.int32 and np.array_equal(status, state['status']), what      # 3 where a pivot fails, as it was elsewhere (1 and 2 included)
        good = np.array([kind != 'bad-pivot' for kind in kinds])
        assert (status[~good] == 3).all() and (np.triu(L, 1) == 0.).all(), what
        if good.any():
            hr.assert_levels(L[good], Lld[good], L64[good], what)
            print('%s: the bits of the float64 restatement: %s' % (what, same_bits(L[good], L64[good])))


@pytest.mark.parametrize('ndim', hr.NDIMS)
def test_step(ndim):
    seen = set()
    for B in layout_sizes(ndim):
        state, trial, metric, L, lo, hi, step_size, kinds, before = case(ndim, B)
        seen.update(kinds)
        for flags, (t_close, t_open) in hr.FLAGS.items():
            (new64, next64, extra64), (newld, nextld, extrald) = restated(ndim, B, flags)
            new, nxt, sample, sample_chi2 = device_step(state, trial, L, lo, hi, step_size, flags)
            what = 'ndim = %d, B = %d, %s' % (ndim, B, flags)
            for name in hr.INTEGERS:      # the discrete results: exactly
                assert new[name].dtype == np.int32 and np.array_equal(new[name], new64[name]), (what, name)
            assert np.array_equal(new['naccepted'] - state['naccepted'], extra64['accept'].astype('i4')), what
            for name in ('x', 'gradient', 'chi2'):      # copied where accepted, untouched elsewhere: the trial's or the state's bits
                assert same_bits(new[name], new64[name]), (what, name)
            frozen = state['status'] != 0
            assert all(same_bits(new[name][frozen], state[name][frozen]) for name in WRITTEN) and same_bits(nxt[frozen], state['x'][frozen]), what
            over = new['status'] != 0
            assert same_bits(nxt[over], new['x'][over]), what
            for name, dev, f8, ld in (('z', new['z'], new64['z'], newld['z']), ('h0', new['h0'], new64['h0'], newld['h0']), ('eps', new['eps'], new64['eps'], newld['eps']),
                                      ('next', nxt, next64, nextld)):
                hr.assert_levels(dev, ld, f8, '%s, %s' % (what, name))
            inside = np.isfinite(nxt).all(axis=1)
            assert (nxt[inside] >= lo).all() and (nxt[inside] <= hi).all() and np.array_equal(inside, np.isfinite(next64).all(axis=1)), what
            if t_close is not None:      # the sample is the state after the decision, frozen chains included
                assert same_bits(sample, new['x']) and same_bits(sample_chi2, new['chi2']), what
                hr.assert_levels(sample, extrald['sample'], extra64['sample'], what + ', sample')
            else:
                assert (sample == 123.).all() and (sample_chi2 == 123.).all(), what
            print('%s: z and next have the bits of the float64 restatement: %s, %s' % (what, same_bits(new['z'], new64['z']), same_bits(nxt, next64)))
    assert seen == set(hr.KINDS) or max(layout_sizes(ndim)) < len(hr.KINDS)


@pytest.mark.parametrize('ndim', [1, 3, 8, 17, 32])
def test_the_first_chains_of_a_longer_batch(ndim):
    """A chain's stream and its arithmetic depend on (seed, b, t) only: the first 3 chains of B = 5 are the chains of B = 3, bit for bit -- and, past a
    workgroup, the first chains of the largest batch those of the batch without its last chain."""
    for long, short in ((5, 3), (max(layout_sizes(ndim)), max(layout_sizes(ndim)) - 1)):
        state, trial, metric, lo, hi, step_size, kinds = hr.make_case(ndim, long, seed=2)
        L, status = hr.factor(metric, state['status'], 'f8')
        state = dict(state, status=status)
        cut = lambda d: {name: value[:short] for name, value in d.items()}      # noqa: E731
        for flags in hr.FLAGS:
            whole = device_step_once(state, trial, L, lo, hi, step_size, flags)
            part = device_step_once(cut(state), cut(trial), L[:short], lo, hi, step_size[:short], flags)
            assert all(same_bits(whole[0][name][:short], part[0][name]) for name in WRITTEN), (ndim, flags)
            assert all(same_bits(a[:short], b) for a, b in zip(whole[1:], part[1:])), (ndim, flags)
