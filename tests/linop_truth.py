"""
Extended-precision truth of the operator kernels of csrc/cp_spline.hip -- ``spline_apply_kernel<4 | 8 | 16>`` (the band on the vector ALUs),
``spline_outer_kernel<2 | 4 | 8>`` (the same with an outer-product epilogue), ``linop_mfma_kernel<false | true>`` (the block-banded GEMM on the matrix
cores) and ``linop_mid_mfma_kernel`` (the contraction along the middle axis) -- and of the host code their plans come from (``cp_spline_operator``,
``plan_from_dense``).  numpy only; shared by tests/test_linop_truth_host.py and tests/test_linop_truth_gpu.py.

Spline plans   truth: tests/spline_truth.py, ``slopes`` in longdouble over all knots and the cubic of the query's interval, with the derivative order
               nu = 0, 1, 2 (a query on an interior knot belongs to the interval that begins there, the last knot to the last interval, as the
               bisection of cp_spline_operator has it; ``extrapolate`` continues the end cubics, NaN outside otherwise, a NaN query stays NaN).
               Rule: spline_truth.levels / assert_within unchanged -- a block is a row, distances against the row's largest |truth|, the level the
               float64 restatement's distance floored at FLOOR = 1.1e-16, ALLOW = 16 levels, a case used while its level is at most CAP = 32 floors.
               Two restatements, entry by entry the one farther from the truth (its level is the larger of the two): the plain float64 solve
               (``slopes(..., dtype='f8')``) and the float64 product with the float64 operator of the unit rows (sigma_truth.spline_operator).
Dense plans    truth: the longdouble product W y (sigma_truth.band_truth at any n), the middle axis einsum('qj,bjc->bqc'); restatement numpy's
               float64 product.  Rule: sigma_truth.relative / blocks / levels / fraction, a block one (row, 64 queries) -- one (batch entry, 64 queries,
               all columns) for the middle axis --, the scale sum_j |W[q, j]| |y[j]| in longdouble, a dot product's own forward-error scale; the same
               FLOOR, ALLOW and CAP.  Weights uniform(0.5, 1.5) of random sign: nothing is identically zero but rows of zeros, whose truth is 0.
Epilogues      sqrt is IEEE: the device's roots are held SQUARED, by the linear rule with SQRT_EXTRA = 3 FLOOR of the value added (the root within
               half an ulp, squared: twice that and the rounding of the square; sigma_truth.MIXED_EXTRA with FLOOR for the 1e-16 of geo_sqrt).
               exp10: the relative distance from the longdouble 10**x is at most ln 10 times the argument's absolute allowance + EXP10_EXTRA = 4e-15,
               the bound test_exp10_epilogue_over_the_whole_line asserts for exp10_mid.  ``scale`` is a power of two but in one case per kernel (3.0).
Rows           seven base rows per case; row i of a batch is base row i % 7 times 2**e_i (spline_truth.batch / unscale: exact, so no truth is computed
               for more than seven rows).  Splines: spline_truth.base_rows.  Dense: 'spread' rows uniform(0.5, 1.5) 2**-e_j, e_j uniform in 0 ... 40
               per knot (sigma_truth's: a few samples dominate a sum of any width), positive where a root follows, of random sign otherwise.
Restated plan  :func:`plan_of`: plan_from_dense -- the band above 1e-18 of a row's maximum, rows of zeros placed beside their neighbours, the tiles
               (first query, count, first knot, span) with the SPAN_CAP cut, span_max, the windows of 64 and of 16 queries rounded to 16 knots,
               sub_windows, prefer_dense, col_first / col_last.  :func:`band_sum` and :func:`window_sum` are the two contractions in float64 in the
               kernels' order, :func:`grouped_store` the store; they exist for the mutations of tests/test_linop_truth_host.py only.
Out of scope   rows that vary by many decades INSIDE one band: what plan_from_dense cuts is bounded by 1e-18 max_j |W[q, j]| sum_j |y_j| over the knots
               outside the band, a property of the design; the rows here stay within 2**40 (dense) or are smooth (splines).

Grid of the spline cases: (family, n, end condition, nu), n in 5, 16, 17, 100, 481, 1000 -- below and at the n >= 16 of prefer_dense, n % 16 = 5, 0, 1, 4,
1, 8 (the partial last chunk), more knots than SPAN_CAP --, families uniform, geom1.05, saw1.5x16, logk_pad (n >= 6) and sigma_r (n >= 100); natural and
clamped with nu = 0, 1, 2, not-a-knot with nu = 0, not-a-knot derivatives on uniform at 100 and 481 knots.  Left out: alt1e3 (thousands of floors), sigma_r
below 100 knots (43 to 1354), jitter100 and saw2x40 (over the cap in the derivatives), not-a-knot derivatives elsewhere (40 to 120 on geom1.05, saw1.5x16).
Measured levels (tests/test_linop_truth_host.py: both restatements, the query sets 'knots', 'beyond' and 'outside'), in FLOORs, of the cases in use: nu = 0 at
most 20.5 (natural), 17.8 (clamped), 19.0 (not-a-knot); nu = 1 at most 24.0 (natural), 26.8 (clamped), 19.3 (not-a-knot); nu = 2 at most 31.5 (natural),
28.8 (clamped), 29.2 (not-a-knot); the further query sets (:func:`extra_cases`) at most 30.0.  Over the cap: OVER_CAP, 16 of the 186 cases of the grid (33.4 to
77.5), all derivatives -- the product with the float64 operator of the unit rows, the second restatement, is the farther one there.
"""
import functools

import numpy as np

import sigma_truth as sg
import spline_truth as st
from spline_truth import LD, FLOOR, ALLOW, CAP, NBASE

TILE_Q, SPAN_CAP = 256, 480      # csrc/cp_spline.hip
LINOP_ROWS = 64                  # 16 LINOP_MT: rows of a matrix-core tile
SUB_FRACTION = 0.67              # CP_LINOP_SUB_FRACTION
SQRT_EXTRA = 3 * FLOOR
EXP10_EXTRA = 4e-15
LN10 = float(np.log(LD(10)))
POST_NONE, POST_SQRT, POST_EXP10 = 0, 1, 2      # CP_SPLINE_POST_*
PATHS = {None: 0, 'valu': 16, 'mfma': 32}       # CP_SPLINE_PATH_*
BC = {'natural': 0, 'clamped': 1, 'not-a-knot': 2}

SIZES = [5, 16, 17, 100, 481, 1000]
SPLINE_FAMILIES = ['uniform', 'geom1.05', 'saw1.5x16', 'logk_pad', 'sigma_r']
QUERY_KINDS = ['knots', 'beyond', 'outside', 'thinned', 'crowded']
COUNTS = [1, 255, 256, 257, 513]
ROW_COUNTS = [1, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65]
MANY_ROWS = 8704

# (family, n, end condition, nu): the level in FLOORs measured by tests/test_linop_truth_host.py over the query sets 'knots', 'beyond' and 'outside' --
# over the cap, not used on the device; the host test holds every entry to being over the cap and the list to a tenth of the grid.  All are derivatives:
# the float64 restatements form c2 = (slope - s_k) / h - t, which cancels where neighbouring spacings differ by 1.5^15 (saw1.5x16) or the knots are a factor
# 1.23 apart (sigma_r with 100 knots).
OVER_CAP = {('uniform', 17, 'natural', 2): 40.4, ('geom1.05', 481, 'clamped', 1): 45.5, ('geom1.05', 1000, 'natural', 1): 39.8,
            ('saw1.5x16', 17, 'natural', 2): 35.3, ('saw1.5x16', 17, 'clamped', 1): 36.0, ('saw1.5x16', 17, 'clamped', 2): 43.2,
            ('saw1.5x16', 481, 'natural', 1): 59.9, ('saw1.5x16', 481, 'natural', 2): 58.3, ('saw1.5x16', 481, 'clamped', 1): 41.0,
            ('saw1.5x16', 481, 'clamped', 2): 61.8, ('saw1.5x16', 1000, 'natural', 1): 36.2, ('saw1.5x16', 1000, 'natural', 2): 34.5,
            ('sigma_r', 100, 'natural', 1): 33.4, ('sigma_r', 100, 'natural', 2): 48.4, ('sigma_r', 100, 'clamped', 1): 77.5,
            ('sigma_r', 100, 'clamped', 2): 72.4}
MAIN_KINDS = ['knots', 'beyond', 'outside']      # every case of the grid in use
EXTRA_KINDS = ['thinned', 'crowded', 'counted']


def extra_cases():
    """(family, n, end condition, nu) -> the further query sets it is used with.  'thinned', 'crowded' and the counted sets put few queries against a
    row's largest value, or all of them where a derivative is small: their levels pass the cap in most derivative cases and on saw1.5x16 (up to 226
    floors at nu = 0, thousands at nu = 1), so they run at nu = 0 on the other four families (measured: at most 13 floors) and, thinned and crowded, on the
    derivatives of the natural spline through 100 uniform knots (at most 30)."""
    out = {}
    for name, sizes in (('uniform', SIZES[1:]), ('geom1.05', SIZES[1:]), ('logk_pad', [16, 17, 100, 481]), ('sigma_r', [100, 481, 1000])):
        for n in sizes:
            for bc in st.BCS:
                out[(name, n, bc, 0)] = EXTRA_KINDS
    out[('uniform', 5, 'natural', 0)] = ['thinned']      # one query
    out[('uniform', 100, 'natural', 1)] = out[('uniform', 100, 'natural', 2)] = ['thinned', 'crowded']
    return out


def query_sets(key):
    """[(label, xq, extrapolate)] of a case of the grid in use."""
    x = st.knots(key[0], key[1])
    sets = []
    for kind in MAIN_KINDS + extra_cases().get(key, []):
        if kind == 'counted':
            sets += [('counted%d' % count, counted(x, count), False) for count in COUNTS]
        else:
            sets.append((kind,) + queries(x, kind))
    return sets


def spline_grid():
    grid = []
    for name in SPLINE_FAMILIES:
        for n in SIZES:
            if (name == 'logk_pad' and n < 6) or (name == 'sigma_r' and n < 100):
                continue
            for bc in ('natural', 'clamped'):
                grid += [(name, n, bc, nu) for nu in (0, 1, 2)]
            grid.append((name, n, 'not-a-knot', 0))
            if name == 'uniform' and n in (100, 481):
                grid += [(name, n, 'not-a-knot', 1), (name, n, 'not-a-knot', 2)]
    return grid


def spline_used():
    return [key for key in spline_grid() if key not in OVER_CAP]


def queries(x, kind):
    """(xq, extrapolate) of a query set: 'knots' the knots, the midpoints and a random point per interval; 'beyond' spline_truth.rows_beyond with the
    end cubics continued, 'outside' the same without; 'thinned' one query per 8 intervals; 'crowded' 300 queries in three intervals (one full tile
    under a span of a few knots)."""
    x = np.asarray(x)
    n = x.size
    if kind == 'knots':
        return st.rows_queries(x), False
    if kind in ('beyond', 'outside'):
        return st.rows_beyond(x), kind == 'beyond'
    if kind == 'thinned':
        return 0.5 * (x[:-1:8] + x[1::8]), False
    if kind == 'crowded':
        j = max((n - 1) // 2 - 1, 0)
        return np.sort(np.random.default_rng(n).uniform(x[j], x[j + 3], 300)), False
    raise ValueError(kind)


def counted(x, count):
    """``count`` ascending queries, uniform over the intervals and inside them, the first and the last knot among them."""
    rng = np.random.default_rng(count)
    j = rng.integers(0, len(x) - 1, count)
    q = np.sort(x[j] + rng.uniform(0., 1., count) * (x[j + 1] - x[j]))
    if count >= 2:
        q[0], q[-1] = x[0], x[-1]
    return q


@functools.lru_cache(maxsize=None)
def spline_case(name, n, bc):
    """x, y (7, n), the slopes of the rows in longdouble and float64 and the float64 slopes of the unit rows."""
    x, y = st.knots(name, n), st.base_rows(name, n)
    case = dict(x=x, y=y, s_ld=st.slopes(x, y, bc), s_f8=st.slopes(x, y, bc, 'f8'), unit_f8=st.slopes(x, np.eye(n), bc, 'f8'))
    return sg._freeze(case)


@functools.lru_cache(maxsize=None)
def unit_slopes_ld(name, n, bc):
    """(n, n) longdouble: the slopes of the unit rows (the operator's truth), once per case."""
    s = st.slopes(st.knots(name, n), np.eye(n), bc)
    s.flags.writeable = False
    return s


def operator_truth(name, n, bc, nu, xq, extrapolate):
    """(nq, n) longdouble: the spline operator as the spline of the unit rows."""
    return np.ascontiguousarray(st.evaluate(st.knots(name, n), np.eye(n), unit_slopes_ld(name, n, bc), xq, extrapolate, nu).T)


def operator_f8(case, nu, xq, extrapolate):
    """(nq, n) float64: the float64 spline of the unit rows (sigma_truth.spline_operator for any end condition and order)."""
    return np.ascontiguousarray(st.evaluate(case['x'], np.eye(case['x'].size), case['unit_f8'], xq, extrapolate, nu).T)


def spline_values(case, nu, xq, extrapolate, scale=1.):
    """(truth (7, nq) longdouble, float64 (7, nq)): entry by entry the restatement farther from the truth."""
    x, y = case['x'], case['y']
    truth = st.evaluate(x, y, case['s_ld'], xq, extrapolate, nu) * LD(scale)
    plain = st.evaluate(x, y, case['s_f8'], xq, extrapolate, nu) * scale
    product = sg.band_product(operator_f8(case, nu, xq, extrapolate), y) * scale
    return truth, sg.farther(truth, plain, product)


def spline_level(truth, f64):
    """The largest level of the rows, in FLOORs."""
    top, level = st.levels(truth, f64)
    assert (top > 0).all()
    return float(level.max() / FLOOR)


def restated_spline(case, nu, xq, extrapolate, mutation=None):
    """The float64 spline of the rows with the PPoly coefficients of cp_spline_operator.  Mutations: 'no_factor_2' nu = 1 without the 2 on c2;
    'knot_below' a query on a knot assigned to the interval below."""
    x, y, s = case['x'], case['y'], case['s_f8']
    n = x.size
    xq = np.asarray(xq, dtype='f8')
    k = np.clip(np.searchsorted(x, xq, side='left' if mutation == 'knot_below' else 'right') - 1, 0, n - 2)
    k = np.where(xq != xq, 0, k)
    h = x[k + 1] - x[k]
    slope = (y[:, k + 1] - y[:, k]) / h
    t = (s[:, k] + s[:, k + 1] - 2. * slope) / h
    c3, c2, c1, c0 = t / h, (slope - s[:, k]) / h - t, s[:, k], y[:, k]
    u = xq - x[k]
    if nu == 0:
        v = c0 + u * (c1 + u * (c2 + u * c3))
    elif nu == 1:
        v = c1 + u * ((1. if mutation == 'no_factor_2' else 2.) * c2 + u * 3. * c3)
    else:
        v = 2. * c2 + 6. * c3 * u
    outside = (xq != xq) if extrapolate else ~((xq >= x[0]) & (xq <= x[-1]))
    v[:, outside] = np.nan
    return v


# ---- dense operators -----------------------------------------------------------------------------------------------------------------------------
def dense_weights(n, bands, seed=0):
    """W (nq, n): ``bands`` a list of (first knot, width), None for a NaN query, 'zero' for a row of zeros; entries uniform(0.5, 1.5) of random sign."""
    rng = np.random.default_rng([len(bands), n, seed, 5])
    w = np.zeros((len(bands), n))
    for q, band in enumerate(bands):
        if band is None:
            w[q] = np.nan
        elif band != 'zero':
            a, width = band
            assert 0 <= a and a + width <= n and width >= 1, (band, n)
            w[q, a:a + width] = rng.uniform(0.5, 1.5, width) * rng.choice([-1., 1.], width)
    return w


def band_layout(n, nq, bw, kind, seed=0):
    """Bands of width bw: 'random' first knots anywhere, 'sweep' first knots rising with the query (the 16-query windows are then a part of the 64-query
    ones); the first band from knot 0, the last to knot n - 1, one narrower band against knot n - 1 (padded to the common width it reaches beyond it);
    NaN queries first, last and in the middle of a tile, rows of zeros first, between banded rows and last, where nq has room."""
    rng = np.random.default_rng([n, nq, bw, seed, 9])
    first = np.sort(rng.integers(0, n - bw + 1, nq)) if kind == 'sweep' else rng.integers(0, n - bw + 1, nq)
    bands = [(int(a), bw) for a in first]
    bands[0], bands[-1] = (0, bw), (n - bw, bw)
    if nq >= 16:
        narrow = (bw + 1) // 2
        bands[-5] = (n - narrow, narrow)
        bands[1], bands[-2] = None, None
        bands[2], bands[-3] = 'zero', 'zero'
        bands[0], bands[3] = 'zero', (0, bw)
        bands[-1], bands[-4] = None, (n - bw, bw)
    if nq >= 160:
        bands[100], bands[133] = None, 'zero'
    return bands


def dense_cases():
    """name -> (n, nq, bands or None for a full operator)."""
    cases = {'full_%dx%d' % (n, nq): (n, nq, None) for n, nq in [(16, 1), (17, 64), (100, 65), (341, 257), (1000, 1030), (1024, 256)]}
    for bw in (1, 7, 8, 9, 17):
        cases['random_bw%d' % bw] = (100, 130, band_layout(100, 130, bw, 'random'))      # sub_windows false
    for bw in (9, 17):
        cases['sweep_bw%d' % bw] = (1000, 257, band_layout(1000, 257, bw, 'sweep'))      # sub_windows true
    return cases


def spread_rows(n, seed=0, signed=False, shape=None):
    """(7, n) (or (7, n) + shape): uniform(0.5, 1.5) 2**-e_j, e_j uniform in 0 ... 40 per knot; signed: of random sign."""
    rng = np.random.default_rng([n, seed, 77])
    full = (NBASE, n) + tuple(shape or ())
    e = rng.integers(0, 41, n).reshape((1, n) + (1,) * len(shape or ()))
    rows = rng.uniform(0.5, 1.5, full) * np.ldexp(1., -e)
    return rows * rng.choice([-1., 1.], full) if signed else rows


def finite_weights(w):
    return np.where(np.isnan(w[:, :1]), 0., w)


def dense_truth(w, y, scale=1.):
    """(truth, scale), each (rows, nq) longdouble: W y times ``scale`` and sum_j |W| |y| times |scale|; NaN / 1 for a NaN query."""
    nanq = np.isnan(w[:, 0])
    wl, yl = finite_weights(w).astype(LD), np.asarray(y).astype(LD)
    true = (yl @ wl.T) * LD(scale)
    mag = (np.abs(yl) @ np.abs(wl).T) * abs(LD(scale))
    true[:, nanq] = np.nan
    mag[:, nanq | (mag[0] == 0)] = 1
    return true, mag


def dense_product(w, y, scale=1.):
    return sg.band_product(w, y) * scale


def mid_truth(w, y, scale=1.):
    """(truth, scale) (nb, nq, m) longdouble of y (nb, n, m)."""
    nanq = np.isnan(w[:, 0])
    wl, yl = finite_weights(w).astype(LD), np.asarray(y).astype(LD)
    true = np.einsum('qj,bjc->bqc', wl, yl) * LD(scale)
    mag = np.einsum('qj,bjc->bqc', np.abs(wl), np.abs(yl)) * abs(LD(scale))
    true[:, nanq] = np.nan
    mag[:, nanq] = 1
    return true, mag


def mid_product(w, y, scale=1.):
    out = np.einsum('qj,bjc->bqc', finite_weights(w), np.asarray(y, dtype='f8')) * scale
    out[:, np.isnan(w[:, 0])] = np.nan
    return out


def tile(a, count):
    """Row i of a batch belongs to base row i % 7."""
    return np.asarray(a)[np.arange(count) % NBASE]


# ---- the rule with the epilogues -------------------------------------------------------------------------------------------------------------------
def exp10_truth(arg):
    with np.errstate(invalid='ignore'):
        return np.power(LD(10), arg)


def unscaled(got, e):
    """got (rows, ...) in longdouble times 2**-e_i, exactly; e None: as it is."""
    got = np.asarray(got).astype(LD)
    if e is None:
        return got
    return got * np.ldexp(LD(1), -np.asarray(e))[(slice(None),) + (None,) * (got.ndim - 1)]


def dense_fraction(got, true, scale, level, post=POST_NONE, what='', block_axes=1, e=None):
    """The largest fraction of the allowance a block of ``got`` uses.  true, scale: those of the ARGUMENT of the epilogue, for the base row i % 7 of row i;
    e: the exponents of the rows (row i = base row times 2**e_i), taken out of the values -- of their squares behind a root -- exactly.
    got (rows, nq) or (nb, nq, m) (block_axes = 2: a block takes all columns)."""
    got, true, scale = np.asarray(got).astype(LD), np.asarray(true), np.asarray(scale)
    if true.shape[0] != got.shape[0]:
        true, scale = tile(true, got.shape[0]), tile(scale, got.shape[0])
    assert e is None or post != POST_EXP10
    if level.shape[0] != got.shape[0]:
        level = tile(level, got.shape[0])
    per_query = np.repeat(level, sg.BLOCK, axis=1)[:, :got.shape[1]]      # the level of a query's block
    if block_axes == 2:
        per_query = per_query[:, :, None]
    if post == POST_SQRT:      # roots held squared: NaN where the truth is negative
        true = np.where(true < 0, np.nan, true)
        allowed = ALLOW * per_query * scale + SQRT_EXTRA * np.abs(np.where(np.isnan(true), 0, true))
        assert not ((np.abs(true) <= allowed) & (true != 0)).any(), '{}: the argument of a root within its allowance of zero has no sign'.format(what)
        got = unscaled(got * got, e)
    elif post == POST_EXP10:
        allowed = LN10 * (ALLOW * per_query * scale) + EXP10_EXTRA
        true = exp10_truth(true)
        with np.errstate(invalid='ignore'):
            got, true = got / true, np.where(np.isnan(true), np.nan, LD(1))
    else:
        allowed = ALLOW * per_query * scale
        got = unscaled(got, e)
    nan = np.isnan(true)
    assert got.shape == true.shape, (what, got.shape, true.shape)
    assert np.array_equal(np.isnan(got), nan), '{}: NaN in other places than the truth has them'.format(what)
    used = np.asarray(np.where(nan, 0, np.abs(got - true)) / allowed, dtype='f8')
    worst = float(used.max()) if used.size else 0.
    print('%s: largest fraction of the allowance %.3g (level at most %.3g FLOOR)' % (what, worst, float(level.max() / FLOOR)))
    return worst


def dense_levels(true, scale, f64, block_axes=1):
    """(rows, nblocks): sigma_truth.levels; the middle axis takes the largest entry over the columns first."""
    if block_axes == 2:
        rel = sg.relative(f64, true, scale).max(axis=-1)
        return np.maximum(FLOOR, sg.blocks(rel))
    return sg.levels(true, scale, [f64])


def spline_fraction(got, truth, f64, post=POST_NONE, what='', e=None, first=0):
    """The row rule of spline_truth.assert_within with the epilogues' extras: got (rows, nq), row i belonging to base row (first + i) % 7 times 2**e_i;
    truth, f64 (7, nq) those of the ARGUMENT of the epilogue.  Returns the largest fraction of the allowance."""
    assert e is None or post != POST_EXP10 and first % NBASE == 0
    top, level = st.levels(truth, f64)
    got = np.asarray(got).astype(LD)
    truth, top, level = tile(truth, len(got)), tile(top, len(got)), tile(level, len(got))
    allowed = (ALLOW * level * top)[:, None] * np.ones(truth.shape[1])
    if post == POST_SQRT:
        truth = np.where(truth < 0, np.nan, truth)
        allowed = allowed + SQRT_EXTRA * np.abs(np.where(np.isnan(truth), 0, truth))
        assert not ((np.abs(truth) <= allowed) & (truth != 0)).any(), '{}: the argument of a root within its allowance of zero has no sign'.format(what)
        got = unscaled(got * got, e)
    elif post == POST_EXP10:
        allowed = LN10 * allowed + EXP10_EXTRA
        truth = exp10_truth(truth)
        with np.errstate(invalid='ignore'):
            got, truth = got / truth, np.where(np.isnan(truth), np.nan, LD(1))
    else:
        got = unscaled(got, e)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert np.array_equal(np.isnan(got), np.isnan(truth)), '{}: NaN in other places than the truth has them'.format(what)
    used = np.asarray(np.where(np.isnan(truth), 0, np.abs(got - truth)) / allowed, dtype='f8')
    worst = float(used.max()) if used.size else 0.
    print('%s: largest fraction of the allowance %.3g (level at most %.3g FLOOR)' % (what, worst, float(level.max() / FLOOR)))
    return worst


# ---- plan_from_dense restated ----------------------------------------------------------------------------------------------------------------------
def band_of(w):
    """(wb (bw, nq), j0, j1, bw): entries above 1e-18 of the row's maximum; j0 = -1 for a NaN query; rows of zeros get a one-entry band of weight 0 at
    the first knot of the nearest banded row before them (else after them, else knot 0)."""
    nq, n = w.shape
    j0, j1 = np.empty(nq, dtype='i4'), np.empty(nq, dtype='i4')
    bw = 1
    for q in range(nq):
        if np.isnan(w[q, 0]):
            j0[q] = j1[q] = -1
            continue
        mx = np.abs(w[q]).max()
        if mx == 0.:
            j0[q] = j1[q] = -2
            continue
        keep = np.flatnonzero(np.abs(w[q]) > mx * 1e-18)
        j0[q], j1[q] = keep[0], keep[-1]
        bw = max(bw, int(j1[q] - j0[q] + 1))
    last = -1
    for q in range(nq):
        if j0[q] >= 0:
            last = j0[q]
        elif j0[q] == -2 and last >= 0:
            j0[q] = j1[q] = last
    last = -1
    for q in range(nq - 1, -1, -1):
        if j0[q] >= 0:
            last = j0[q]
        elif j0[q] == -2:
            j0[q] = j1[q] = last if last >= 0 else 0
    wb = np.zeros((bw, nq))
    for q in range(nq):
        if j0[q] >= 0:
            m = j1[q] - j0[q] + 1
            wb[:m, q] = w[q, j0[q]:j1[q] + 1]
    return wb, j0, j1, bw


def _windows(j0, j1, nq, n, size, count):
    raw = np.zeros((count, 2), dtype='i8')
    for t in range(count):
        q = np.arange(size * t, min(size * (t + 1), nq))
        q = q[j0[q] >= 0] if q.size else q
        if q.size:
            raw[t] = j0[q].min(), j1[q].max() + 1
    return raw


def plan_of(w):
    """dict of what plan_from_dense derives from a dense operator: n, nq, bw, wb, j0, j1, tiles (ntiles, 4), span_max, n_pad, nq_pad, win64 / win16
    (the windows rounded to 16 knots; raw64 / raw16 unrounded), sub_windows, prefer_dense, dense (a dense copy is kept), col_first, col_last."""
    w = np.asarray(w, dtype='f8')
    nq, n = w.shape
    wb, j0, j1, bw = band_of(w)
    tiles, span_max, q0 = [], 1, 0
    while q0 < nq:
        lo, hi, q = n, 0, q0
        while q < nq and q - q0 < TILE_Q:
            nlo, nhi = lo, hi
            if j0[q] >= 0:
                nlo, nhi = min(lo, int(j0[q])), max(hi, min(int(j0[q]) + bw, n))
            if q > q0 and nhi > nlo and nhi - nlo > SPAN_CAP:
                break
            lo, hi = nlo, nhi
            q += 1
        if hi <= lo:
            lo, hi = 0, 1
        tiles.append((q0, q - q0, lo, hi - lo))
        span_max = max(span_max, hi - lo)
        q0 = q
    n_pad, nq_pad = (n + 15) // 16 * 16, (nq + 63) // 64 * 64
    raw64, raw16 = _windows(j0, j1, nq, n, 64, nq_pad // 64), _windows(j0, j1, nq, n, 16, nq_pad // 16)
    rounded = lambda raw: np.stack([raw[:, 0] // 16 * 16, (raw[:, 1] + 15) // 16 * 16], axis=1)
    win64, win16 = rounded(raw64), rounded(raw16)
    work, work_sub = 64. * (win64[:, 1] - win64[:, 0]).sum(), 16. * (win16[:, 1] - win16[:, 0]).sum()
    dense_bytes = n_pad * nq_pad * 8
    dense = dense_bytes <= (256 << 20)
    sub_windows = bool(work_sub <= SUB_FRACTION * work)
    prefer_dense = bool(n >= 16 and work <= 3.5 * nq * bw)
    if dense:
        valu_fits = 4 * span_max * 8 <= 160 * 1024
        near = n >= 16 and work <= 5. * nq * bw
        if not prefer_dense and not near and valu_fits and dense_bytes > (16 << 20):
            dense = False
    if not dense:
        prefer_dense = sub_windows = False
    tiles = np.array(tiles, dtype='i8')
    col_first, col_last = int(tiles[:, 2].min()), int((tiles[:, 2] + tiles[:, 3]).max())
    if dense:
        for lo, hi in win64:
            if hi > lo:
                col_first, col_last = min(col_first, int(lo)), max(col_last, int(hi))
    col_last = min(col_last, n)
    col_first = min(col_first, col_last)
    return dict(n=n, nq=nq, bw=bw, wb=wb, j0=j0, j1=j1, tiles=tiles, span_max=span_max, n_pad=n_pad, nq_pad=nq_pad, raw64=raw64, raw16=raw16, win64=win64,
                win16=win16, sub_windows=sub_windows, prefer_dense=prefer_dense, dense=dense, col_first=col_first, col_last=col_last, w=w)


def apply_rows(plan, nrows):
    """R of spline_apply_kernel: 16, halved while the staged knots exceed 64 KB or half as many rows would do."""
    rows = 16
    while rows > 4 and (rows * plan['span_max'] * 8 > 64 * 1024 or rows // 2 >= nrows):
        rows //= 2
    return rows


def outer_rows(plan, nz, nrows):
    """R of spline_outer_kernel: 8, halved while knots, values and factors exceed 64 KB or half as many rows would do."""
    rows = 8
    while rows > 2 and (rows * (plan['span_max'] + TILE_Q + nz) * 8 > 64 * 1024 or rows // 2 >= nrows):
        rows //= 2
    return rows


def default_route(plan, nrows):
    valu_fits = 4 * plan['span_max'] * 8 <= 160 * 1024
    return 'mfma' if plan['dense'] and ((plan['prefer_dense'] and nrows >= 16) or not valu_fits) else 'valu'


def mid_resident(plan):
    return plan['nq_pad'] == 64 and plan['n_pad'] <= 32


def band_sum(plan, y, mutation=None):
    """spline_apply_kernel's contraction in float64 in its order: per tile, sum_i wb[i, q] ylds[min(j0[q] - tj0 + i, span - 1)].  Mutations: 'shift' the
    band one knot up; 'last_chunk' the entries from 8 floor((bw - 1) / 8) on dropped."""
    y = np.asarray(y, dtype='f8')
    wb, j0, bw = plan['wb'], plan['j0'], plan['bw']
    out = np.empty((y.shape[0], plan['nq']))
    stop = 8 * ((bw - 1) // 8) if mutation == 'last_chunk' else bw
    for q0, count, tj0, span in plan['tiles']:
        q = np.arange(q0, q0 + count)
        ok = j0[q] >= 0
        base = np.where(ok, j0[q], tj0) - tj0 + (1 if mutation == 'shift' else 0)
        staged = y[:, tj0:tj0 + span]
        acc = np.zeros((y.shape[0], count))
        for i in range(stop):
            acc = acc + wb[i, q][None, :] * staged[:, np.minimum(base + i, span - 1)]
        acc[:, ~ok] = np.nan
        out[:, q] = acc
    return out


def window_sum(plan, y, mutation=None):
    """linop_mfma_kernel's contraction in float64: per 64 queries the chunks of 16 knots of their window, per 16 queries (sub_windows) only the chunks of
    their own; behind knot n a row reads zeros.  Mutations: 'round_up' the lower end of a window rounded up to 16; 'previous_window' the 16 queries
    j + 1 take the window of the 16 queries j; 'next_row' the entries behind n are the next row's first ones."""
    y = np.asarray(y, dtype='f8')
    n, nq, n_pad, nq_pad = plan['n'], plan['nq'], plan['n_pad'], plan['nq_pad']
    wd = np.zeros((nq_pad, n_pad))
    for q in range(nq):
        if plan['j0'][q] >= 0:
            wd[q, plan['j0'][q]:plan['j1'][q] + 1] = plan['w'][q, plan['j0'][q]:plan['j1'][q] + 1]
    ypad = np.zeros((y.shape[0], n_pad))
    ypad[:, :n] = y
    if mutation == 'next_row':
        flat = np.concatenate([y.ravel(), np.zeros(n_pad)])
        ypad = np.stack([flat[r * n:r * n + n_pad] for r in range(y.shape[0])])

    def low(raw, rounded):
        return (raw + 15) // 16 * 16 if mutation == 'round_up' else rounded

    acc = np.zeros((y.shape[0], nq_pad))
    with np.errstate(invalid='ignore'):
        for t in range(nq_pad // 64):
            klo, khi = low(plan['raw64'][t, 0], plan['win64'][t, 0]), plan['win64'][t, 1]
            for s in range(4 * t, 4 * t + 4):
                slo, shi = klo, khi
                if plan['sub_windows']:
                    u = max(s - 1, 0) if mutation == 'previous_window' else s
                    slo, shi = low(plan['raw16'][u, 0], plan['win16'][u, 0]), plan['win16'][u, 1]
                for kb in range(klo, khi, 16):
                    if slo <= kb < shi:
                        acc[:, 16 * s:16 * s + 16] += ypad[:, kb:kb + 16] @ wd[16 * s:16 * s + 16, kb:kb + 16].T
    out = acc[:, :nq]
    out[:, plan['j0'] < 0] = np.nan
    return out


def out_index(row, q, nq, group):
    row, q = np.asarray(row, dtype='i8'), np.asarray(q, dtype='i8')
    if group <= 0:
        return row * nq + q
    b = row // group
    return (b * nq + q) * group + (row - b * group)


def grouped_store(values, group, mutation=None):
    """The store of linop_mfma_kernel: values (nrows, nq) written into a flat array of nrows nq elements (NaN where nothing is written; writes behind
    it are dropped) -- base + row x rstride + q x qstride per tile of 64 rows in the plain and the one-group form (group a multiple of 64), out_index
    otherwise.  Mutation 'swap_strides': row and query strides swapped."""
    nrows, nq = values.shape
    flat = np.full(nrows * nq, np.nan)
    q = np.arange(nq)
    for row0 in range(0, nrows, LINOP_ROWS):
        rowin = np.arange(min(LINOP_ROWS, nrows - row0))
        if group <= 0 or group % LINOP_ROWS == 0:
            base, rstride, qstride = row0 * nq, nq, 1
            if group > 0:
                b = row0 // group
                base, rstride, qstride = b * nq * group + (row0 - b * group), 1, group
            if mutation == 'swap_strides':
                rstride, qstride = qstride, rstride
            index = base + rowin[:, None] * rstride + q[None, :] * qstride
        else:
            index = out_index(row0 + rowin[:, None], q[None, :], nq, group)
        ok = (index >= 0) & (index < flat.size)
        flat[index[ok]] = values[row0 + rowin][ok]
    return flat


def ungroup(flat, nrows, nq, group):
    """(nrows, nq) of a flat output in the grouped layout (nrows / group, nq, group)."""
    flat = np.asarray(flat)
    if group <= 0:
        return flat.reshape(nrows, nq)
    return flat.reshape(nrows // group, nq, group).transpose(0, 2, 1).reshape(nrows, nq)


# ---- the cases of the device tests (truth and level of the seven base rows, computed once per process, read-only) -----------------------------------
MID_SHAPES = [(5, 1, 1, 1), (32, 64, 129, 3), (33, 64, 129, 3), (30, 65, 128, 2), (16, 130, 257, 2), (33, 130, 129, 350)]      # (n, nq, m, nb)
OUTER_NQ = [1, 256, 257]
OUTER_NZ = [1, 2, 3, 7, 64, 511]
OUTER_ROWS = [1, 2, 3, 5, 9]
OUTER_CASE = ('sigma_r', 1000, 'natural')


@functools.lru_cache(maxsize=None)
def dense_case(name, signed=True, scale=1.):
    """dict(w, plan, y (7, n), true, scale, f64, level (7, nblocks)) of a case of :func:`dense_cases`; true and scale those of scale x W y."""
    n, nq, bands = dense_cases()[name]
    if bands is None:
        rng = np.random.default_rng([n, nq, 3])
        w = rng.uniform(0.5, 1.5, (nq, n)) * rng.choice([-1., 1.], (nq, n))
        if nq > 3:
            w[3] = np.nan
    else:
        w = dense_weights(n, bands)
    y = spread_rows(n, signed=signed)
    true, mag = dense_truth(w, y, scale)
    f64 = dense_product(w, y, scale)
    return sg._freeze(dict(name=name, w=w, plan=plan_of(w), y=y, true=true, scale=mag, f64=f64, level=dense_levels(true, mag, f64), factor=scale))


@functools.lru_cache(maxsize=None)
def mid_case(shape, signed=True, scale=1.):
    """The same for the middle axis: y (7, n, m), true / scale / f64 (7, nq, m), level (7, nblocks)."""
    n, nq, m, nb = shape
    rng = np.random.default_rng([n, nq, m, 4])
    w = rng.uniform(0.5, 1.5, (nq, n)) * rng.choice([-1., 1.], (nq, n))
    if nq > 20:
        w[0], w[17], w[nq - 1] = np.nan, np.nan, np.nan      # a NaN query first, inside and last
    y = spread_rows(n, seed=m, signed=signed, shape=(m,))
    true, mag = mid_truth(w, y, scale)
    f64 = mid_product(w, y, scale)
    return sg._freeze(dict(shape=shape, w=w, plan=plan_of(w), y=y, true=true, scale=mag, f64=f64, level=dense_levels(true, mag, f64, 2), factor=scale))


def outer_factors(nz):
    """(7, nz) positive factors g."""
    return np.random.default_rng([nz, 6]).uniform(0.5, 1.5, (NBASE, nz))


def outer_values(nq, nz, scale=1.):
    """(xq, g (7, nz), truth (7, nq nz) longdouble, float64 (7, nq nz)) of scale x spline x g on OUTER_CASE; a NaN query among 16 or more."""
    case = spline_case(*OUTER_CASE)
    xq = counted(case['x'], nq)
    if nq >= 16:
        xq[5] = np.nan
    g = outer_factors(nz)
    truth, f64 = spline_values(case, 0, xq, False, scale)
    return xq, g, (truth[:, :, None] * g[:, None, :].astype(LD)).reshape(NBASE, -1), (f64[:, :, None] * g[:, None, :]).reshape(NBASE, -1)
