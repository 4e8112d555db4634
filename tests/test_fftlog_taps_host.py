"""CPU: tests/fftlog_taps_truth.py is what it says before tests/test_fftlog_large_truth_gpu.py and tests/test_fftlog_fused_truth_gpu.py judge a kernel by it.
(a) ``truth`` (a sparse circular correlation, no FFT) equals a direct O(Np^2) longdouble DFT of the promised transform irfft(conj(rfft(z) u)) post,
    to longdouble rounding, at Np = 4 ... 1024 (up to 32 with the small-size taps), once with 'log' padding of the exact-ratio rows;
(b) ``restated`` is ``oracle.fftlog.apply`` driven through a ``Tables`` object filled with the synthetic tables (Np = 2^14, two kernel indices,
    odd npad - n, both keep_padding values): the restatement that sets the allowance is the oracle every other FFTLog test uses;
(c) the level of the float64 restatement stays below CAP = 32 x FLOOR at every case of the ladder up to 2^22 (measured 5.1 ... 7.4);
(d) a u table with one tap moved by one sample is caught by ``check``, at a large and at a fused size;
(e) the same cap for every case of the fused ladder Np = 4 ... 8192 (measured 2.0 ... 12.8), the taps of Np >= 2^14 as they were recorded, and the
    pair factor of the fused kernel's contract;
(f) the zero and subnormal rows of the fused device test through the CPU emulation of the kernel's phases (tests/host_emu)."""
import numpy as np
import pytest

import fftlog_taps_truth as tt
from oracle import fftlog as ofl
from test_fftlog_host import emu      # noqa: F401  (the fixture: the kernel's phases compiled for the CPU)

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


@pytest.mark.parametrize('npad', [4, 8, 16, 32, 64, 128, 256, 512, 1024])
def test_truth_is_the_promised_transform(npad):
    eps = float(np.finfo(LD).eps)
    cases = [(1, npad // 3 | 1, 'edge', False), (3, max(npad // 2 - 3, 2), (0, 'edge'), True), (2, npad - 1, 0, True), (2, npad, 0, False), (3, max(npad // 2, 3), 'log', True)]
    for nker, n, extrap, keep in cases:
        syn = tt.tables(npad, nker, seed=n)
        rows = tt.log_rows(n, npad, seed=1, negative=n >= 4) if extrap == 'log' else tt.base_rows(n, seed=1)
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


def test_taps_of_the_large_sizes_are_unchanged():
    """tests/test_fftlog_large_truth_gpu.py and its recorded fractions rest on the taps of Np >= 2^14; the small-size rule ends at Np = 32."""
    npad = 1 << 16
    for ker in range(3):
        shifts, weights = tt.taps(npad, ker)
        np.testing.assert_array_equal(shifts, [3 * ker, 1, npad // 3 + 7 + 11 * ker, npad - 5 - ker, npad // 2 + 1 + 2 * ker])
        np.testing.assert_array_equal(weights, np.roll(np.array([0.9, -0.7, 1.3, -1.1, 0.6]), ker) * (1. + 0.125 * ker))
    np.testing.assert_array_equal(tt.taps(64, 0)[0], [0, 1, 28, 59, 33])
    for npad in (4, 8, 16, 32):
        for ker in range(3):
            shifts, weights = tt.taps(npad, ker)
            assert shifts.size == weights.size == min(5, npad - 1) == np.unique(shifts % npad).size
            assert {0, 1} <= set(shifts.tolist()) and shifts.max() > npad // 2 and weights.min() < 0. < weights.max()
    np.testing.assert_array_equal(tt.exponents(3, 2), tt.EXPONENTS[:6].reshape(3, 2))
    np.testing.assert_array_equal(tt.exponents(4097, 1)[-1], tt.EXPONENTS[:1])


@pytest.mark.parametrize('npad', tt.FUSED_LADDER)
def test_levels_of_the_fused_ladder(npad):
    """A condition on the inputs of tests/test_fftlog_fused_truth_gpu.py that the reference alone decides: the float64 restatement of every case
    of the ladder, with the exponent tables of its tests (a) and (b), stays below CAP x FLOOR (measured 2.0 ... 12.8 FLOOR; no case had to be
    redrawn or dropped).  The subnormal rows of its test (f) are the one exemption, stated there."""
    worst = 0.
    for nker in (1, 3):
        syn = tt.tables(npad, nker)
        for n, extrap, keep, kind in tt.fused_cases(npad):
            tables = [tt.fused_table(extrap, tt.FUSED_NBATCH, nker)]
            if npad in (16, 512, 4096) and not tt.homogeneous(extrap):      # (where the padding scales with the row every table shares the base rows' level)
                tables += [tt.pair_table(tt.FUSED_NBATCH, nker, d) for d in (0, 2)]
            for table in tables:
                batch = tt.fused_batch(n, npad, syn, extrap, keep, kind, tt.FUSED_NBATCH, table)
                assert float(batch.level.max()) <= tt.CAP * tt.FLOOR, (npad, nker, n, extrap, keep, kind)
                assert batch.factor.min() >= 1. and batch.factor.max() <= 2.**(tt.SPREAD + 1)
                assert (batch.factor[-1] == 1.).all()      # the row without a partner
                if table is None:      # EXPONENTS: the first two pairs of either nker are far outside the spread
                    assert (batch.factor == 1.).all()
                worst = max(worst, float(batch.level.max()))
    print('Np = %d: level at most %.3g FLOOR' % (npad, worst / tt.FLOOR))


def test_pair_tables_and_factor():
    """Exponent tables with chosen pair distances, and the factor of the kernel's contract: 1 outside the spread, the pair's larger magnitude over
    the row's own inside."""
    for nker in (1, 3):
        for difference in (0, 2, 12):
            e = tt.exponents(9, nker, tt.pair_table(9, nker, difference))
            np.testing.assert_array_equal(np.abs(e[0:8:2] - e[1:8:2]), difference)
            if difference:
                assert ((e[0:8:2] - e[1:8:2]) > 0).any() and ((e[0:8:2] - e[1:8:2]) < 0).any()
    top = np.array([[1.], [4.], [3.], [2.**12], [0.], [1.], [np.inf], [1.], [5.]])
    np.testing.assert_array_equal(tt.pair_factor(top)[:, 0], [4., 1., 1., 1., 1., 1., 1., 1., 1.])


def test_a_moved_tap_is_caught_at_a_fused_size():
    npad, nker = 512, 3
    n, extrap, keep, kind = tt.fused_cases(npad, ('half_zero',))[0]
    syn = tt.tables(npad, nker)
    batch = tt.fused_batch(n, npad, syn, extrap, keep, kind, tt.FUSED_NBATCH)
    honest = np.stack([tt.restated(batch.rows[:, ker], n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep) for ker in range(nker)], axis=1)
    assert tt.check(batch.comparable(honest), batch.true, batch.level, 'the restatement itself') <= 1. / tt.ALLOW
    for moved in range(5):
        shifts, weights = syn.taps[2]
        shifts = shifts.copy()
        shifts[moved] = (shifts[moved] + 1) % npad
        wrong = honest.copy()
        wrong[:, 2] = tt.restated(batch.rows[:, 2], n, npad, syn.pre[2], syn.post[2], tt.u_table(npad, (shifts, weights)), extrap, keep)
        assert tt.check(batch.comparable(wrong), batch.true, batch.level, 'Np = 512, tap %d moved by one sample' % moved) > 1e10


@pytest.mark.parametrize('npad,n,extrap', [(16, 5, 'edge'), (512, 256, 'edge'), (4096, 2048, 0), (2048, 1024, 'log')])
def test_zero_and_subnormal_rows_through_the_emulation(emu, npad, n, extrap):      # noqa: F811
    """The pairs of test_zero_and_subnormal_rows of the device file -- (zero, 2^24), (2^-13, zero), (subnormal, 2^3), a zero row alone -- through
    the kernel's own phases on the CPU (decode_info, fix_input, fix_output of csrc/cp_fftlog_body.h; the emulation takes the magnitudes straight
    from the rows): the zero rows exactly 0, the subnormal row within ALLOW of its own level."""
    syn = tt.tables(npad, 1)
    kind = 'log' if extrap == 'log' else 'dense'
    base, base_true, base_level = tt.base_case(n, npad, syn, extrap, False, kind=kind)
    rows = np.zeros((7, 1, n))
    rows[1, 0], rows[2, 0], rows[4, 0], rows[5, 0] = np.ldexp(base[1], 24), np.ldexp(base[0], -13), np.ldexp(base[0], -1030), np.ldexp(base[1], 3)
    t = ofl.Tables()
    t.n, t.npad, t.nker, t.pre, t.post, t.u = n, npad, 1, syn.pre, syn.post, syn.u
    with np.errstate(all='ignore'):
        got = emu(t, rows, tt.extrap_codes(extrap))
        true = tt.truth(rows[:, 0], n, npad, syn.pre[0], syn.post[0], syn.taps[0], extrap)[:, None]
        level = tt.levels(true, tt.restated(rows[:, 0], n, npad, syn.pre[0], syn.post[0], syn.u[0], extrap)[:, None])[1]
    for i in (0, 3, 6):
        if extrap == 'log':      # no end ratio: 0 / 0
            assert np.isnan(true[i]).all() and np.isnan(got[i]).all()
        else:
            assert (got[i] == 0.).all(), 'zero row %d: the largest element %.3g' % (i, float(np.abs(got[i]).max()))
    np.testing.assert_array_equal(level[[1, 2, 5], 0], base_level[[1, 0, 1], 0])
    assert tt.check(got, true, level, 'Np = %d, the emulated kernel on zero and subnormal rows' % npad) <= 1.
