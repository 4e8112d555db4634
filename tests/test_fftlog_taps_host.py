"""CPU: tests/fftlog_taps_truth.py is what it says before tests/test_fftlog_large_truth_gpu.py judges a kernel by it.
(a) ``truth`` (a sparse circular correlation, no FFT) equals a direct O(Np^2) longdouble DFT of the promised transform irfft(conj(rfft(z) u)) post,
    to longdouble rounding, at Np = 64 ... 1024;
(b) ``restated`` is ``oracle.fftlog.apply`` driven through a ``Tables`` object filled with the synthetic tables (Np = 2^14, two kernel indices,
    odd npad - n, both keep_padding values): the restatement that sets the allowance is the oracle every other FFTLog test uses;
(c) the level of the float64 restatement stays below CAP = 32 x FLOOR at every case of the ladder up to 2^22 (measured 5.1 ... 7.4);
(d) a u table with one tap moved by one sample is caught by ``check``."""
import numpy as np
import pytest

import fftlog_taps_truth as tt
from oracle import fftlog as ofl

LD, CLD = tt.LD, tt.CLD


def direct_dft(rows, n, npad, pre, post, u_ld, extrap, keep_padding):
    """irfft(conj(rfft(z) u), Np) post with both transforms as matrix products in longdouble, the phases reduced in integers."""
    in_left, in_right, out_left = tt.widths(n, npad)
    z = ofl.pad(np.asarray(rows, dtype=LD), (in_left, in_right), extrap) * pre.astype(LD)
    j = np.arange(npad, dtype='i8')
    phase = (LD(8) * np.arctan(LD(1)) / LD(npad)) * ((j[:, None] * j[None, :]) % npad).astype(LD)
    w = np.cos(phase) + 1j * np.sin(phase)              # exp(+2 pi i j k / Np)
    spec = (z.astype(CLD) @ np.conj(w))[..., :npad // 2 + 1] * u_ld
    spec = np.conj(spec)
    spec[..., 0], spec[..., -1] = spec[..., 0].real, spec[..., -1].real      # what irfft reads of the DC and Nyquist bins
    full = np.concatenate([spec, np.conj(spec[..., 1:-1])[..., ::-1]], axis=-1)
    g = (full @ w).real / LD(npad) * post.astype(LD)
    return g if keep_padding else g[..., out_left:out_left + n]


@pytest.mark.parametrize('npad', [64, 128, 256, 512, 1024])
def test_truth_is_the_promised_transform(npad):
    eps = float(np.finfo(LD).eps)
    for nker, n, extrap, keep in [(1, npad // 3 | 1, 'edge', False), (3, npad // 2 - 3, (0, 'edge'), True), (2, npad - 1, 0, True), (2, npad, 0, False)]:
        syn = tt.tables(npad, nker, seed=n)
        rows = tt.base_rows(n, seed=1)
        for ker in range(nker):
            got = tt.truth(rows, n, npad, syn.pre[ker], syn.post[ker], syn.taps[ker], extrap, keep)
            ref = direct_dft(rows, n, npad, syn.pre[ker], syn.post[ker], tt.u_table(npad, syn.taps[ker], dtype=LD), extrap, keep)
            assert got.dtype == LD and got.shape == ref.shape == (2, npad if keep else n)
            err = float(np.abs(got - ref).max() / np.abs(ref).max())
            # two sums of Np terms each, every term rounded once: 4 Np eps is the worst case, the usual error its square root
            assert err <= 4 * npad * eps, (npad, nker, n, extrap, keep, err)
            # and the float64 table handed to a plan is that u, rounded: per tap a phase <= 2 pi off by three roundings (6 pi 2^-53), cos and
            # sin an ulp each, both components: 16 x 2^-52 x |h_t| covers it
            assert np.abs(syn.u[ker] - tt.u_table(npad, syn.taps[ker], dtype=LD)).max() <= 16 * np.abs(syn.taps[ker][1]).sum() * 2.**-52


def test_nonfinite_rows_are_nan_throughout():
    n, npad = 41, 64
    syn = tt.tables(npad)
    rows = np.stack([tt.base_rows(n)[0]] * 3)
    rows[1, 7], rows[2, 40] = np.nan, np.inf
    got = tt.truth(rows, n, npad, syn.pre[0], syn.post[0], syn.taps[0], 'edge')
    assert np.isfinite(got[0]).all() and np.isnan(got[1:]).all()
    assert np.array_equal(got[0], tt.truth(rows[0], n, npad, syn.pre[0], syn.post[0], syn.taps[0], 'edge'))


@pytest.mark.parametrize('keep', [False, True])
def test_restated_is_the_oracle(keep):
    npad, n, nker = 1 << 14, 5461, 2
    assert (npad - n) % 2 == 1
    syn = tt.tables(npad, nker, seed=3)
    t = ofl.Tables()
    t.n, t.npad, t.nker = n, npad, nker
    t.in_left, t.in_right, t.out_left = tt.widths(n, npad)
    t.out_right = t.in_left
    assert t.in_left != t.out_left
    t.pre, t.post, t.u = syn.pre, syn.post, syn.u
    rows = tt.batch(tt.base_rows(n), 3, nker)
    for extrap in (0, 'edge', (0, 'edge')):
        ref = ofl.apply(t, rows, extrap=extrap, keep_padding=keep)
        for ker in range(nker):
            got = tt.restated(rows[:, ker], n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep)
            np.testing.assert_array_equal(got, ref[:, ker])


@pytest.mark.parametrize('npad', [p for p in tt.LADDER if p <= 1 << 22])
def test_levels_of_the_ladder(npad):
    n, nbatch, nker, modes = tt.ladder_case(npad)
    assert n % 2 == 1 and (npad - n) % 2 == 1
    syn = tt.tables(npad, nker)
    for extrap, keep in modes:
        base, true, level = tt.base_case(n, npad, syn, extrap, keep)
        print('Np = 2^%d, %s, keep_padding=%s: level %.3g FLOOR' % (npad.bit_length() - 1, extrap, keep, float(level.max() / tt.FLOOR)))
        assert float(level.max()) <= tt.CAP * tt.FLOOR, (npad, extrap, keep)
        assert (np.abs(true).max(axis=-1) > 0.5).all()
        # exact scaling: the restatement of a scaled row is the scaled restatement, so one level serves every row of a batch
        rows = tt.batch(base, nbatch, nker)
        if npad == 1 << 14:
            for ker in range(nker):
                a = tt.restated(rows[:, ker], n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep)
                b = tt.restated(base, n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep)[np.arange(nbatch) % 2]
                np.testing.assert_array_equal(a, b * np.ldexp(1., tt.exponents(nbatch, nker)[:, ker])[:, None])


def test_a_moved_tap_is_caught():
    npad = 1 << 14
    n, nbatch, nker, modes = tt.ladder_case(npad)
    syn = tt.tables(npad, nker)
    extrap, keep = modes[0]
    base, true, level = tt.base_case(n, npad, syn, extrap, keep)
    honest = np.stack([tt.restated(base, n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep) for ker in range(nker)], axis=1)
    assert tt.check(honest, true, level, 'the restatement itself') <= 1. / tt.ALLOW
    for moved in range(5):
        shifts, weights = syn.taps[1]
        shifts = shifts.copy()
        shifts[moved] = (shifts[moved] + 1) % npad
        wrong = honest.copy()
        wrong[:, 1] = tt.restated(base, n, npad, syn.pre[1], syn.post[1], tt.u_table(npad, (shifts, weights)), extrap, keep)
        assert tt.check(wrong, true, level, 'tap %d moved by one sample' % moved) > 1e10
    with pytest.raises(AssertionError):
        wrong = honest.copy()
        wrong[1, 0, 5] = np.nan
        tt.check(wrong, true, level, 'a NaN the truth does not have')
    zero = np.zeros((1, 8), dtype=LD)
    assert tt.check(np.zeros((1, 8)), zero, tt.FLOOR, 'a zero row') == 0. and tt.check(np.full((1, 8), 1e-300), zero, tt.FLOOR, 'not quite zero') == np.inf
