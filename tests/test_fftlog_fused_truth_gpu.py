"""GPU: the LDS-resident fused FFTLog kernel (csrc/cp_fftlog_body.h, cp_fftlog_kernel.h; padded lengths Np = 4 ... 8192) against exact longdouble truth
at EVERY size and variant, through the C ABI (cp_fftlog_plan_create with synthetic tables, cp_fftlog_execute, cp_fftlog_execute_window,
cp_fftlog_plan_destroy).  The kernel table u is made of a few taps, which turns the promised transform into a sparse circular correlation that needs no
FFT (tests/fftlog_taps_truth.py, held to a direct DFT and to oracle.fftlog.apply by tests/test_fftlog_taps_host.py, which also holds the level of
every case used here below CAP = 32 FLOOR).  Outputs go into a buffer of canaries with one more element behind it.

Allowance: ALLOW = 16 x the rounding level of the float64 numpy restatement, per row, relative to the row's largest |truth|.  One amendment, the
kernel's documented contract: two batch items share one complex transform, and a pair whose tilted magnitudes lie within CP_ROW_SCALE_SPREAD = 4
binades is not rescaled -- there a row's allowance is relative to the larger tilted magnitude of its pair (tt.pair_factor).  The exponents in use are
0, 2 (inside the spread), 12 and the +-300 of tt.EXPONENTS (outside).  Every test prints the largest fraction of the allowance it used.

  test_every_size_and_variant   (a) tt.fused_cases of every Np: GENERIC (odd n, odd Np - n; n = Np - 1; 2 n = Np with keep_padding), HALF, HALF_ZERO, LOG
                                (exact-ratio rows, one negative end ratio), nker = 1 and 3, five batch items
  test_pairs_equal_in_scale     (b) the same cases at Np = 16, 512, 4096 with all exponents 0 (the path without fix-up) and pairs 2^2 and 2^12 apart
  test_more_pairs_than_the_grid (c) Np = 16, 512, 4096, 8192, every variant: 3 G + 2 pairs (nker = 1) and 3 G + 3 (nker = 3), the last ones incomplete
  test_window                   (d) cp_fftlog_execute_window at Np = 512, 4096: columns inside against the truth, outside still the canary
  test_nonfinite_rows           (e) (NaN, live) and (live, +Inf) pairs, a NaN padding value; GENERIC below a wave, HALF, HALF_ZERO (screened ahead)
  test_zero_and_subnormal_rows  (f) (zero, 2^24), (2^-13, zero), (subnormal, 2^3) and a zero row alone, at GENERIC 16, HALF 512, HALF_ZERO 4096, LOG 2048

Largest fraction of the allowance measured on the MI355X (against the truth; 1 is the limit, 1/16 = 0.0625 numpy's own distance), per Np = 4 ... 8192:
  GENERIC   0.108 0.334 0.126 0.136 0.106 0.115 0.116 0.090 0.096 0.091 0.085 0.086      LOG  0.149 0.238 0.147 0.147 0.111 0.150 0.099 0.099 0.094 0.097 0.089 0.090
  HALF (512 ...)  0.095 0.083 0.086 0.082 0.079      HALF_ZERO  0.072 0.076 0.078 0.083 0.070
  (Np = 8, 16: the restatement is a handful of operations, its level sits on the floor of 1.1e-16, and the kernel's butterflies are 3-5 such units away; the CPU emulation
  of the phases gives the same 0.334.)  (b) at most 0.263 (Np = 16), 0.102, 0.091; (c) 0.187 (Np = 16), at most 0.090 above; (d) 0.072; (e) 0.087; (f) partners 0.087, the
  subnormal rows 0.05 ... 0.11 of allowances whose levels are 69, 146, 179, 334 FLOOR.  38 tests in 10.4 s.
Found by test_zero_and_subnormal_rows: decode_info rescaled a pair only when both exponent fields were non-zero -- a row of zeros beside a live partner came back as the
rounding of the partner's half of the packed transform (7.7e-10 ... 2.6e-8 beside a row of 2^24) and a subnormal row beside a normal one was lost in its partner's rounding.
The magnitude field now keeps 0 for rows that ARE zero and counts a subnormal row as exponent field 1; see decode_info.
Mutations of a scratch copy of the kernel sources: CP_ROW_SCALE_SPREAD = 400 fails every test with pairs more than 4 binades apart (38 ... 1e119 allowances), passes the pairs
2^0 and 2^2 apart; nxt_ker replaced by the current index fails (c) with nker = 3 at Np = 512, 4096, 8192 (HALF, HALF_ZERO: 2e14) and passes nker = 1; out_left for in_left
fails exactly the cases with odd Np - n (1e14 ... 7e14); the window's out_last one short fails test_window alone (canary); one entry of the U table swapped with its
neighbour at Np = 4096 fails every test of that size (6e11 ... 3e12) and no other.
"""
import time

import numpy as np
import pytest

import fftlog_taps_truth as tt
from fftlog_device import CANARY, Plan, lib      # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

SLAB = 1024      # batch items compared at a time (longdouble copies of a whole batch of (c) take hundreds of MB)


def compare(batch, got, what):
    """Largest fraction of the allowance over the batch; the allowance of a row is ALLOW x level x factor x max|truth|."""
    allowed = batch.level * batch.factor
    return max(tt.check(batch.comparable(got, slice(lo, lo + SLAB)), batch.true[lo:lo + SLAB], allowed[lo:lo + SLAB], what) for lo in range(0, got.shape[0], SLAB))


def run(plan, syn, n, npad, extrap, keep, kind, nbatch, table, what):
    """One batch of a case through the plan: the largest fraction of the allowance."""
    batch = tt.fused_batch(n, npad, syn, extrap, keep, kind, nbatch, table)
    with np.errstate(all='ignore'):
        got = plan(batch.rows, extrap, keep)
    return compare(batch, got, what)


def by_plan(cases):
    """The cases grouped by row length: one plan serves every padding and keep_padding of its (n, Np, nker)."""
    sizes = sorted(set(c[0] for c in cases))
    return [(n, [c for c in cases if c[0] == n]) for n in sizes]


def attempt(failed, what, *args):
    """One case: its fraction of the allowance, or inf where it breaks a rule outright (a canary left, a NaN out of place); every case of a test is
    run before the test fails, so that the list says which cases a defect reaches."""
    try:
        fraction = run(*args, what)
    except AssertionError as exc:
        print('%s: %s' % (what, exc))
        fraction = np.inf
    if not fraction <= 1.:
        failed.append('%s: %.3g' % (what, fraction))
    return fraction


def sweep(lib, npad, table_of, label):      # noqa: F811
    worst, failed = {}, []
    for nker in (1, 3):
        syn = tt.tables(npad, nker)
        for n, cases in by_plan(tt.fused_cases(npad)):
            with Plan(lib, n, syn) as plan:
                for _, extrap, keep, kind in cases:
                    variant = tt.variant_of(n, npad, extrap, keep)
                    what = 'Np = %d %s, n = %d, nker = %d, %s, keep_padding=%s, %s rows, %s' % (npad, variant, n, nker, extrap, keep, kind, label)
                    fraction = attempt(failed, what, plan, syn, n, npad, extrap, keep, kind, tt.FUSED_NBATCH, table_of(extrap, tt.FUSED_NBATCH, nker))
                    worst[variant] = max(worst.get(variant, 0.), fraction)
    print('Np = %d, %s: largest fraction per variant %s' % (npad, label, ', '.join('%s %.3f' % kv for kv in sorted(worst.items()))))
    assert not failed, '%d cases over their allowance:\n%s' % (len(failed), '\n'.join(failed))


@pytest.mark.parametrize('npad', tt.FUSED_LADDER)
def test_every_size_and_variant(lib, npad):      # noqa: F811
    start = time.time()
    sweep(lib, npad, tt.fused_table, 'exponents of the ladder')
    print('Np = %d: %.1f s' % (npad, time.time() - start))


@pytest.mark.parametrize('difference', [0, 2, 12])
@pytest.mark.parametrize('npad', [16, 512, 4096])
def test_pairs_equal_in_scale(lib, npad, difference):      # noqa: F811
    """difference 0: every pair equal in scale and different in content -- gate(info) == 0, no fix-up, the production case; 2: inside the spread, the
    smaller row is held to the larger one's magnitude; 12: outside, each row to its own."""
    sweep(lib, npad, lambda extrap, nbatch, nker: tt.pair_table(nbatch, nker, difference), 'pairs 2^%d apart' % difference)


def grid_cases(npad):
    """One cropped case per variant of the size (the smallest outputs: all rows are compared)."""
    half, third = npad // 2, (npad // 3) | 1
    cases = [('generic', third, 'edge', 'dense'), ('log', min(half, tt.LOG_MAX_N - 1 if npad > 2 * tt.LOG_MAX_N else half), 'log', 'log')]
    if npad >= tt.HALF_MIN:
        cases += [('half', half, 'edge', 'dense'), ('half_zero', half, 0, 'dense')]
    return cases


@pytest.mark.parametrize('nker', [1, 3])
@pytest.mark.parametrize('npad', [16, 512, 4096, 8192])
def test_more_pairs_than_the_grid(lib, npad, nker):      # noqa: F811
    """Persistent workgroups past their second pair: with G an upper bound of any variant's grid, nker = 1 takes 2 (3 G + 1) + 1 batch items (3 G + 2
    pairs: every workgroup a third pair, some a fourth, the last pair incomplete) and nker = 3 takes 2 G + 1 (3 G + 3 pairs, the last three incomplete,
    the next pair's factors of another kernel index fetched ahead).  All rows are compared; the truth comes through the 2^e batches of two base rows."""
    import torch
    start = time.time()
    grid = tt.grid_bound(npad, torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    nbatch = 2 * (3 * grid + 1) + 1 if nker == 1 else 2 * grid + 1
    syn = tt.tables(npad, nker)
    failed = []
    for variant, n, extrap, kind in grid_cases(npad):
        assert tt.variant_of(n, npad, extrap, False) == variant
        with Plan(lib, n, syn) as plan:
            assert 0 < plan.grid(nbatch) <= grid and ((nbatch + 1) // 2) * nker > 3 * grid
            what = 'Np = %d %s, n = %d, nker = %d, %d batch items on a grid of at most %d' % (npad, variant, n, nker, nbatch, grid)
            attempt(failed, what, plan, syn, n, npad, extrap, False, kind, nbatch, None)
    assert not failed, '\n'.join(failed)
    print('Np = %d, nker = %d: %.1f s' % (npad, nker, time.time() - start))


@pytest.mark.parametrize('npad', [512, 4096])
def test_window(lib, npad):      # noqa: F811
    """VAR_HALF_ZERO_WINDOW against the truth: the columns of the window as the whole-row transform has them, every other column still the canary."""
    n, nker, nbatch = npad // 2, 3, tt.FUSED_NBATCH
    syn = tt.tables(npad, nker)
    batch = tt.fused_batch(n, npad, syn, 0, False, 'dense', nbatch)
    windows = [(0, 1), (n - 1, 1), (n // 3, min(257, n - n // 3)), (0, n), (n // 2, 0)]
    with Plan(lib, n, syn) as plan:
        for first, count in windows:
            got = plan.run(batch.rows, 0, False, window=(first, count))
            inside = np.zeros(n, dtype=bool)
            inside[first:first + count] = True
            assert (got[..., ~inside] == CANARY).all(), 'window [%d, %d): columns outside were written' % (first, first + count)
            assert not (got[..., inside] == CANARY).any(), 'window [%d, %d): columns inside were not written' % (first, first + count)
            if count:
                # (the allowance stays that of the whole row: relative to the row's largest |truth|, which may lie outside the window)
                top = np.abs(batch.true).max(axis=-1)
                dist = np.abs(batch.comparable(got)[..., inside] - batch.true[..., inside]).max(axis=-1)
                fraction = float((dist / (tt.LD(tt.ALLOW) * batch.level * batch.factor * top)).max())
                print('Np = %d, window [%d, %d): largest fraction of the allowance %.3g' % (npad, first, first + count, fraction))
                assert fraction <= 1.
        # any other variant stores whole rows
        edge = tt.fused_batch(n, npad, syn, 'edge', False, 'dense', nbatch)
        got = plan.run(edge.rows, 'edge', False, window=(n // 3, 5))
        assert not (got == CANARY).any()
        assert compare(edge, got, "Np = %d, 'edge' padding through cp_fftlog_execute_window: whole rows" % npad) <= 1.


SCREENED = [(16, 5, 'edge', 'generic'), (512, 256, 'edge', 'half'), (4096, 2048, 0, 'half_zero'), (2048, 1024, 'log', 'log')]


def explicit_rows(npad, n, extrap, syn, items, scaled, special):
    """rows, truth and level (items, 1, .) of a batch of ``items`` rows given row by row: ``scaled`` {item: (base row, exponent)} through the truth of the base rows,
    ``special`` {item: row} each through its own truth and level (formed from the row as it is); every other item is a row of zeros."""
    kind = 'log' if extrap == 'log' else 'dense'
    base, base_true, base_level = tt.base_case(n, npad, syn, extrap, False, kind=kind)
    rows, true, level = np.zeros((items, 1, n)), np.zeros((items, 1, n), dtype=tt.LD), np.full((items, 1), tt.FLOOR)
    for i, (b, e) in scaled.items():
        rows[i, 0], true[i, 0], level[i, 0] = np.ldexp(base[b], e), np.ldexp(base_true[b, 0], e), base_level[b, 0]
    with np.errstate(all='ignore'):
        for i in list(special) + [i for i in range(items) if i not in scaled and i not in special]:
            if i in special:
                rows[i, 0] = special[i](base)
            true[i, 0] = tt.truth(rows[i, 0], n, npad, syn.pre[0], syn.post[0], syn.taps[0], extrap)
            level[i, 0] = tt.levels(true[i, 0], tt.restated(rows[i, 0], n, npad, syn.pre[0], syn.post[0], syn.u[0], extrap))[1]
    return rows, true, level


@pytest.mark.parametrize('npad,n,extrap,variant', SCREENED[:3])
def test_nonfinite_rows(lib, npad, n, extrap, variant):      # noqa: F811
    """A row that is not finite comes back NaN throughout and leaves its pair partner within the partner's own allowance: the pairs (NaN, 2^-40),
    (2^10, +Inf), a finite pair behind them (screened a pair ahead at HALF_ZERO) and a row alone.  Then a NaN as the left padding value: every
    row NaN, as in the truth (a variant that pads; HALF_ZERO never forms its padding)."""
    assert tt.variant_of(n, npad, extrap, False) == variant
    syn = tt.tables(npad, 1)

    def with_value(b, where, value):
        def make(base):
            row = base[b].copy()
            row[where] = value
            return row
        return make

    rows, true, level = explicit_rows(npad, n, extrap, syn, 7, {1: (1, -40), 2: (0, 10), 4: (0, 3), 5: (1, -9), 6: (0, -13)},
                                      {0: with_value(0, n // 3, np.nan), 3: with_value(1, 0, np.inf)})
    assert np.isnan(true[0]).all() and np.isnan(true[3]).all() and np.isfinite(true[[1, 2, 4, 5, 6]].astype('f8')).all()
    with Plan(lib, n, syn) as plan:
        with np.errstate(all='ignore'):
            got = plan(rows, extrap, False)
            assert tt.check(got, true, level, 'Np = %d %s, (NaN, live) (live, +Inf) pairs' % (npad, variant)) <= 1.
            if variant != 'half_zero':
                got = plan(rows, (np.nan, extrap), False)
                assert np.isnan(got).all(), 'a NaN padding value makes every row NaN'
                assert np.isnan(tt.truth(rows[1, 0], n, npad, syn.pre[0], syn.post[0], syn.taps[0], (np.nan, extrap))).all()


@pytest.mark.parametrize('npad,n,extrap,variant', SCREENED)
def test_zero_and_subnormal_rows(lib, npad, n, extrap, variant):      # noqa: F811
    """Rows of zeros and of subnormal samples beside a live partner: the pairs (zero, 2^24), (2^-13, zero), (subnormal, 2^3) and a zero row alone.  The
    zero rows come back exactly 0 -- what the partner's rounding leaves in the other half of the packed transform is not their result --, the
    partners stay within their own allowance, the subnormal row within an allowance of its own level.  That row is base row 0 times 2^-1030 as
    float64 holds it, truth and level formed from the row as it is; its tilted samples and results are subnormal, the level of the restatement is
    hundreds of FLOOR (printed) and exempt from the cap of 32 in this test alone, as in tests/test_fftlog_large_truth_gpu.py.
    Under 'log' padding a row of zeros has no end ratio (0 / 0): the truth, numpy and the kernel all give NaN throughout for it."""
    assert tt.variant_of(n, npad, extrap, False) == variant
    syn = tt.tables(npad, 1)
    rows, true, level = explicit_rows(npad, n, extrap, syn, 7, {1: (1, 24), 2: (0, -13), 5: (1, 3)}, {4: lambda base: np.ldexp(base[0], -1030)})
    assert 0. < tt.tilted_top(rows[4, 0], n, npad, syn.pre[0], extrap) < 2.**-1022
    zeros = [0, 3, 6]
    print('Np = %d %s: level of the subnormal row %.3g FLOOR' % (npad, variant, float(level[4, 0] / tt.FLOOR)))
    with Plan(lib, n, syn) as plan:
        with np.errstate(all='ignore'):
            got = plan(rows, extrap, False)
    for i in zeros:
        if extrap == 'log':
            assert np.isnan(true[i]).all() and np.isnan(got[i]).all()
        else:
            assert (true[i] == 0).all()
            assert (got[i] == 0.).all(), 'zero row %d: %d elements are not 0, the largest %.3g' % (i, int((got[i] != 0.).sum()), float(np.abs(got[i]).max()))
    normal = np.arange(rows.shape[0]) != 4
    assert tt.check(got[normal], true[normal], level[normal], 'Np = %d %s, zero rows and their partners' % (npad, variant)) <= 1.
    assert tt.check(got[4:5], true[4:5], level[4:5], 'Np = %d %s, the subnormal row' % (npad, variant)) <= 1.
