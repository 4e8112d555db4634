"""
Extended-precision truth of the step of wallish2018 that decides the most -- the second derivatives M of the clamped spline through a coefficient sequence,
the box between their two maxima and the rewriting of that box by a spline through the remaining knots (csrc/cp_wallish_dd.h, reference
bao_filter.py:377-405) -- with the cases, the float64 restatements of the three variants that run and the launch plans of the two entry points that can
be fed sequences: ``cp_wallish_dd_box`` (n = 1024: the elimination in LDS with a halo of 32 knots and two lanes sweeping towards the box; n = 2048: the
recursions in registers with mirror terms and the sweeps as composed affine maps with reciprocals) and ``cp_wallish_tail`` (the 2048 text on the XOR
layout, in place).  numpy only.  tests/test_wallish_truth_host.py holds the cases to the edges they are named for, tests/test_wallish_truth_gpu.py runs them.

Truth (the functions of tests/spline_truth.py, knots x = 1 .. n): M is the longdouble clamped solve over all n knots; the box is numpy's argmax rule on it
(first index on ties, NaN largest; an empty second range gives 0, include/cosmoprimo_amd.h) plus the offsets; the rewritten box is ``gap_truth`` over ALL
remaining knots.  A box outside [1, n - 2] or inverted removes nothing.  Yardsticks: the plain float64 solve, and for the 2048-knot routes also the float64
restatement of the scheme that runs (:func:`m_recursive`, :func:`remove_windowed` with ``composed=True``); a block's level is the larger of the two
(tests/splice_truth.py).  Rule: ALLOW = 16 levels, FLOOR = 1.1e-16, CAP = 32 FLOOR.  A block is one sequence's M, or one (sequence, box) of rewritten
knots.  A case over the cap is listed in OVER_CAP and not sent to the device.

Sequences: the DST-like decaying rows of ``spline_truth.gap_rows`` with PLANTED DIPS: y_j lowered by w U makes M largest at j (U = 8 x the largest |M| of
the row without dips), so the two maxima and every decoy stand where the case says -- first maxima weigh 8 U, second ones 2 U, a decoy outside the range
beside its edge knot 1.2 x the maximum at that knot (the pair of neighbouring dips leaves the inner knot the largest of its range).  A sequence that is not
finite has no truth (the reference raises; a Thomas solve makes every M NaN): there the device's own M decides, by the same argmax rule.

A group of cases is one launch: (n, margin_first, margin_second, offset_first, offset_second) and its sequences; GROUPS names them, ``group(n, name)``
builds them with their truths (cached).
"""
import functools

import numpy as np

import spline_truth as st

LD = np.longdouble
FLOOR, ALLOW, CAP = st.FLOOR, st.ALLOW, st.CAP
SIZES = [1024, 2048]
DD_HALO = 32           # csrc/cp_wallish_dd.h
GAP_WINDOW = 64
DD_NTAB = 40
LEAD_FACTOR = 1000.    # a decision leads its runner-up by this many times the largest |M_f64 - M_ld| of its sequence


def sqrt3(dtype):
    return np.sqrt(np.asarray(3, dtype=dtype))


def tables(dtype='f8'):
    """(ctab, gtab, c_last): c_i = 1 / (4 - c_{i-1}) from 1/2 (DdTable) and from 0 (GapTable), and 1 / (2 - (2 - sqrt 3))."""
    one = np.asarray(1, dtype=dtype)
    c, g = np.empty(DD_NTAB, dtype=dtype), np.empty(DD_NTAB, dtype=dtype)
    c[0], g[0] = one / 2, 0 * one
    for i in range(1, DD_NTAB):
        c[i], g[i] = one / (4 - c[i - 1]), one / (4 - g[i - 1])
    return c, g, one / (2 - (2 - sqrt3(dtype)))


# ---- truths ---------------------------------------------------------------------------------------------------------------------------------------

def m_truth(y, dtype=LD):
    """(rows, n): the second derivatives at the knots of the clamped spline through (1 .. n, y), a Thomas solve over all knots in ``dtype``."""
    y = np.atleast_2d(y)
    return st.knot_second_derivatives(np.arange(1, y.shape[-1] + 1), y, bc='clamped', dtype=dtype)


def argmax_in(row, lo, hi, last=False):
    """numpy's argmax over row[lo:hi] as an index of row; 0 when the range is empty."""
    if lo >= hi:
        return 0
    if last:
        return hi - 1 - int(np.argmax(row[lo:hi][::-1]))
    return lo + int(np.argmax(row[lo:hi]))


def box_rule(m, margin_first, margin_second, lower_shift=0, upper_shift=0, last=False):
    """(rows, 2): [argmax over [margin_first, n - margin_first), argmax over [that + margin_second, n - margin_first)], before the offsets.  The shifts and
    ``last`` are the mutations of tests/test_wallish_truth_host.py."""
    m = np.atleast_2d(m)
    n = m.shape[-1]
    out = np.zeros((len(m), 2), dtype='i8')
    for r, row in enumerate(m):
        hi = n - margin_first + upper_shift
        out[r, 0] = argmax_in(row, margin_first, hi, last)
        out[r, 1] = argmax_in(row, out[r, 0] + margin_second + lower_shift, hi, last)
    return out


def valid_box(a, b, n):
    return 1 <= a <= b <= n - 2


# ---- float64 restatements of the schemes that run --------------------------------------------------------------------------------------------------

def m_elimination(y, halo=DD_HALO, dtype='f8'):
    """second_derivatives_and_box<S>: lane l owns the knots [S l, S l + S) and starts both sweeps ``halo`` knots outside them from zero; reads beyond
    either end repeat the end knot."""
    y = np.atleast_2d(y).astype(dtype)
    rows, n = y.shape
    S = n // 64
    own = S * np.arange(64)
    ctab, _, c_last = tables(dtype)

    def c_of(i):
        return np.where(i >= n - 1, c_last, ctab[np.clip(i, 0, DD_NTAB - 1)])

    def yc(i):
        return y[:, np.clip(i, 0, n - 1)]

    D, M = np.empty_like(y), np.empty_like(y)
    d = np.zeros((rows, 64), dtype=dtype)
    for t in range(halo + S):
        i = own - halo + t
        d = (6 * ((yc(i + 1) - yc(i)) - (yc(i) - yc(i - 1))) - d) * c_of(i)
        if t >= halo:
            D[:, i] = d
    m = np.zeros((rows, 64), dtype=dtype)
    for t in range(halo + S):
        i = own + S + halo - 1 - t
        d = D[:, np.clip(i, 0, n - 1)]
        m = np.where(i >= n - 1, d, d - c_of(i) * m)
        if t >= halo:
            M[:, i] = m
    return M


def m_recursive(y, mirror_first=True, mirror_last=True, dtype='f8'):
    """second_derivatives_and_box_recursive: second differences over the sequence reflected about its end knots, cpur::recursions per lane, the
    neighbours' totals as carries, the mirror terms of knot 1 and knot n - 2 at the two ends (the fused multiply-adds written as two roundings)."""
    y = np.atleast_2d(y).astype(dtype)
    rows, n = y.shape
    S = n // 64
    own = S * np.arange(64)
    P = sqrt3(dtype) - 2
    left, right = y[:, np.maximum(own - 1, 0)].copy(), y[:, np.minimum(own + S, n - 1)].copy()
    left[:, 0], right[:, 63] = y[:, 1], y[:, n - 2]
    ext = np.concatenate([left[:, :, None], y.reshape(rows, 64, S), right[:, :, None]], axis=-1)
    g = (ext[..., 2:] - ext[..., 1:-1]) - (ext[..., 1:-1] - ext[..., :-2])
    for t in range(S - 2, -1, -1):
        g[..., t] = P * g[..., t + 1] + g[..., t]
    g_first, g_second = g[..., 0].copy(), g[..., 1].copy()
    f = np.zeros((rows, 64), dtype=dtype)
    f_before_last = f
    for t in range(S):
        e = P * f + g[..., t]
        f = e - P * g[..., t + 1] if t + 1 < S else e
        if t == S - 2:
            f_before_last = f
        g[..., t] = e
    f_last = f
    gin, fin = np.zeros_like(f), np.zeros_like(f)
    gin[:, :-1], fin[:, 1:] = g_first[:, 1:], f_last[:, :-1]
    p_far = P**(S - 1)
    gin[:, 63] = p_far * fin[:, 63] + f_before_last[:, 63] if mirror_last else 0
    fin[:, 0] = p_far * gin[:, 0] + g_second[:, 0] if mirror_first else 0
    c = gin
    for t in range(S - 1, -1, -1):
        c = c * P
        g[..., t] += c
    c = fin
    for t in range(S):
        c = c * P
        g[..., t] += c
    return g.reshape(rows, n) * sqrt3(dtype)


def remove_windowed(y, a, b, dtype='f8', composed=False, start=None, gtab_shift=0, loop_stop=None, clip_invalid=False):
    """remove_box<S> / gap_spline_kernel (``composed=False``: two sweeps of at most GAP_WINDOW knots towards the box, quotients as divisions) or
    remove_box_parallel (``composed=True``: a lane per knot of either window, the sweeps' steps composed as affine maps by six butterfly steps, quotients as
    products with reciprocals).  y (rows, n) -> the whole rows with [a, b] rewritten; an invalid box returns them as they are.
    Mutations: ``start`` 'clamped' / 'centred' for both kinds of start, ``gtab_shift`` -1, ``loop_stop`` 64, ``clip_invalid``."""
    y = np.atleast_2d(y).astype(dtype)
    rows, n = y.shape
    out = y.copy()
    if clip_invalid:
        a, b = max(a, 1), min(b, n - 2)
    if not valid_box(a, b, n):
        return out
    x = np.arange(1, n + 1).astype(dtype)
    z = y * (x * x)
    _, gtab, _ = tables(dtype)
    L, R = a - 1, b + 1
    g = np.asarray(R - L, dtype=dtype)
    i0, i1 = max(L - GAP_WINDOW, 0), min(R + GAP_WINDOW, n - 1)
    nl, nr = L - 1 - i0, i1 - 1 - R
    lane = np.arange(64)

    def first_slope(i, at_end):
        clamped = at_end if start is None else start == 'clamped'
        if clamped:
            return np.zeros(rows, dtype=dtype)
        return (z[:, min(i + 1, n - 1)] - z[:, max(i - 1, 0)]) / 2

    def sweep(count, knots, d):
        """d <- (3 (z_{i+1} - z_{i-1}) - d) gtab[k + 1] over the knots in their order"""
        if not composed:
            for k in range(count):
                i = knots[k]
                d = (3 * (z[:, i + 1] - z[:, i - 1]) - d) * gtab[min(k + 1, DD_NTAB - 1)]
            return d
        al, bl = np.ones((rows, 64), dtype=dtype), np.zeros((rows, 64), dtype=dtype)
        live = lane < count
        i = np.clip(knots, 1, n - 2)
        c = gtab[np.minimum(lane + 1, DD_NTAB - 1)]
        al = np.where(live, -c, al)
        bl = np.where(live, 3 * (z[:, i + 1] - z[:, i - 1]) * c, bl)
        for off in (1, 2, 4, 8, 16, 32):
            pal, pbl = al[:, lane ^ off], bl[:, lane ^ off]
            lower = (lane & off) == 0
            bl = np.where(lower, pal * bl + pbl, al * pbl + bl)
            al = al * pal
        return al[:, 0] * d + bl[:, 0]

    def table_at(k):
        k = k + gtab_shift
        return gtab[min(k, DD_NTAB - 1)] if k > 0 else 0 * gtab[0]

    inv_g = 1 / g
    cpL, dpL = 0 * g, first_slope(i0, i0 == 0)
    if L != i0:
        dpL = sweep(nl, i0 + 1 + lane, dpL)
        cp = table_at(nl) if nl > 0 else 0 * g
        den = 2 * (1 + g) - g * cp
        if composed:
            d = 3 * (g * (z[:, L] - z[:, L - 1]) + (z[:, R] - z[:, L]) * inv_g)
            cpL = 1 / den
            dpL = (d - g * dpL) * cpL
        else:
            d = 3 * (g * (z[:, L] - z[:, L - 1]) + (z[:, R] - z[:, L]) / g)
            cpL = 1 / den
            dpL = (d - g * dpL) / den
    bqR, dqR = 0 * g, first_slope(i1, i1 == n - 1)
    if R != i1:
        dqR = sweep(nr, i1 - 1 - lane, dqR)
        bq = table_at(nr) if nr > 0 else 0 * g
        den = 2 * (g + 1) - g * bq
        if composed:
            d = 3 * ((z[:, R] - z[:, L]) * inv_g + g * (z[:, R + 1] - z[:, R]))
            bqR = 1 / den
            dqR = (d - g * dqR) * bqR
        else:
            d = 3 * ((z[:, R] - z[:, L]) / g + g * (z[:, R + 1] - z[:, R]))
            bqR = 1 / den
            dqR = (d - g * dqR) / den
    zL, zR = z[:, L], z[:, R]
    if composed:
        sL = (dpL - cpL * dqR) * (1 / (1 - cpL * bqR))
        sR = dqR - bqR * sL
        slope = (zR - zL) * inv_g
        tt = (sL + sR - 2 * slope) * inv_g
        c3, c2 = tt * inv_g, (slope - sL) * inv_g - tt
    else:
        sL = (dpL - cpL * dqR) / (1 - cpL * bqR)
        sR = dqR - bqR * sL
        slope = (zR - zL) / g
        tt = (sL + sR - 2 * slope) / g
        c3, c2 = tt / g, (slope - sL) / g - tt
    stop = b if loop_stop is None else min(b, a + loop_stop - 1)
    i = np.arange(a, stop + 1)
    u = (i - L).astype(dtype)
    v = zL[:, None] + u * (sL[:, None] + u * (c2[:, None] + u * c3[:, None]))
    out[:, a:stop + 1] = v * (1 / (x[i] * x[i])) if composed else v / (x[i] * x[i])
    return out


# ---- launch plans, restated from the entry points -----------------------------------------------------------------------------------------------

def dd_box_lds(n):
    return (4 * (n + 64) + 2 * DD_NTAB) * 8      # cp_wallish_dd_box, csrc/cp_bao.hip


def dd_box_plan(nrows, n, cus=256):
    """(grid, trips of the longest workgroup): min(ceil(nrows / 4), CUs x floor(160 KiB / LDS bytes)) workgroups of four waves, a sequence per wave."""
    groups = (nrows + 3) // 4
    grid = min(groups, cus * max(160 * 1024 // dd_box_lds(n), 1))
    return grid, (groups + grid - 1) // grid


def dd_box_counts(n, cus=256):
    """1, 3, 4, 5; one full trip plus 5; two full trips plus 1 (the prefetch runs in the middle of the loop)."""
    trip = 4 * cus * max(160 * 1024 // dd_box_lds(n), 1)
    return [1, 3, 4, 5, trip + 5, 2 * trip + 1]


def tail_plan(nrows, cus=256):
    """(grid, trips): cp::balanced_grid(pairs, 2 CUs) -- the pairs dealt evenly over the fewest trips of the resident workgroups."""
    pairs = (nrows + 1) // 2
    rounds = (pairs + 2 * cus - 1) // (2 * cus)
    return (pairs + rounds - 1) // rounds, rounds


def tail_counts(cus=256):
    """rows: 1, 3, 4, 5; one full trip plus 5; two full trips plus 1 -- the odd ones end on a row without a partner."""
    trip = 2 * 2 * cus
    return [1, 3, 4, 5, trip + 5, 2 * trip + 1]


def cyclic(base, nrows):
    """(nrows, n): row i = base[i % len(base)] * 2**e_i with the exponents of ``spline_truth.batch`` (exact)."""
    return base[np.arange(nrows) % len(base)] * np.ldexp(1., st.exponents(nrows))[:, None]


def uncycled(values, nbase):
    """The rows of a device result of a ``cyclic`` batch in the scale of the rows [0, nbase) of that batch (exact: powers of two)."""
    values = np.asarray(values)
    e = st.exponents(len(values))
    return values * np.ldexp(1., e[np.arange(len(values)) % nbase] - e)[:, None]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------------

FIRST, SECOND, BESIDE, BESIDE_END, OUTSIDE = 8., 2., 1.2, 1.5, 32.      # weights of planted dips, in units of U (BESIDE_END: a decoy on an end knot, whose row of the system differs)


def cases(n, name):
    """[(case, edge, dips [(knot, weight)], other)] of a group; other: None, 'zero', 'plain' or [(knot, value)] of samples that are not finite."""
    S = n // 64
    h = n // 2
    nan, inf = np.nan, np.inf

    def two(first, second):
        return [(first, FIRST), (second, SECOND)]

    if name == 'm0_0':      # margins (0, 0), offsets (0, 0): the second range starts on the first maximum, boxes of one knot
        return [('knot_0', 'first maximum on knot S l, l = 0; box with a = 0', [(0, FIRST)], None),
                ('knot_last', 'first maximum on knot S l + S - 1, l = 63; box with b = n - 1', [(n - 1, FIRST)], None),
                ('box_1_1', 'GAP_BOXES (1, 1): L = i0, one knot', [(1, FIRST)], None),
                ('box_last', 'R = i1 = n - 1, one knot', [(n - 2, FIRST)], None),
                ('nl_0', 'L = i0 + 1: nl = 0', [(2, FIRST)], None),
                ('nr_0', 'R = i1 - 1: nr = 0', [(n - 3, FIRST)], None),
                ('nl_1', 'nl = 1: gtab[1]', [(3, FIRST)], None),
                ('nr_1', 'nr = 1: gtab[1]', [(n - 4, FIRST)], None),
                ('end_l0', 'first maximum on knot S l + S - 1, l = 0', [(S - 1, FIRST)], None),
                ('start_l1', 'first maximum on knot S l, l = 1', [(S, FIRST)], None),
                ('end_l1', 'first maximum on knot S l + S - 1, l = 1', [(2 * S - 1, FIRST)], None),
                ('start_l31', 'first maximum on knot S l, l = 31', [(31 * S, FIRST)], None),
                ('end_l31', 'first maximum on knot S l + S - 1, l = 31', [(32 * S - 1, FIRST)], None),
                ('start_l63', 'first maximum on knot S l, l = 63', [(63 * S, FIRST)], None),
                ('zero', 'all-zero sequence: first = margin_first', [], 'zero'),
                ('plain', 'no dip', [], 'plain')]
    if name == 'm1_0':      # margins (1, 0), offsets (0, 0)
        return [('at_margin', 'first maximum on margin_first', [(1, FIRST)], None),
                ('at_upper', 'first maximum on n - margin_first - 1', [(n - 2, FIRST)], None),
                ('decoys', 'larger decoys on margin_first - 1 and n - margin_first', [(5 * S + 3, FIRST), (0, OUTSIDE), (n - 1, OUTSIDE)], None),
                ('decoy_below', 'first maximum on margin_first, larger decoy one knot below', [(1, FIRST), (0, BESIDE_END * FIRST)], None),
                ('decoy_above', 'first maximum on n - margin_first - 1, larger decoy one knot above', [(n - 2, FIRST), (n - 1, BESIDE_END * FIRST)], None),
                ('plain', 'no dip', [], 'plain')]
    if name == 'm1_0_wide':      # margins (1, 0), offsets (0, n - 3)
        return [('box_all', 'GAP_BOXES (1, n - 2): all but the end knots, the strided rewrite loop', [(1, FIRST)], None),
                ('box_beyond', 'box with b > n - 2', [(7, FIRST)], None),
                ('plain', 'no dip', [], 'plain')]
    if name == 'mhalf_0':      # margins (n / 2 - 1, 0), offsets (0, 0): a range of two knots
        return [('low', 'first maximum on margin_first = S l + S - 1, l = 31, larger decoy one knot below', [(h - 1, FIRST), (h - 2, BESIDE * FIRST)], None),
                ('high', 'first maximum on n - margin_first - 1, larger decoy one knot above', [(h, FIRST), (h + 1, BESIDE * FIRST)], None),
                ('zero', 'all-zero sequence: first = margin_first', [], 'zero'),
                ('plain', 'no dip', [], 'plain')]
    if name == 'm20_5':      # margins (20, 5), offsets (-10, 20): the filter's own
        f = n - 21
        return [('at_margin', 'first maximum on margin_first, larger decoy one knot below', [(20, FIRST), (19, BESIDE * FIRST), (40, SECOND / 2)], None),
                ('at_upper', 'first maximum on n - margin_first - 1, larger decoy one knot above; empty second range; box with b < a',
                 [(f, FIRST), (f + 1, BESIDE * FIRST)], None),
                ('decoys', 'larger decoys on margin_first - 1 and n - margin_first', [(7 * S + 5, FIRST), (9 * S + 1, 2 * SECOND), (19, 10.), (n - 20, 10.)], None),
                ('second_at_lower', 'second maximum on first + margin_second, larger decoy one knot below',
                 [(3 * S + 2, FIRST), (3 * S + 7, SECOND), (3 * S + 6, BESIDE * SECOND)], None),
                ('lower_start', 'first + margin_second on a segment start, second maximum in the straddling segment', two(4 * S - 5, 4 * S + 3), None),
                ('lower_start_later', 'first + margin_second on a segment start, second maximum in a later segment', two(4 * S - 5, 6 * S + 1), None),
                ('lower_end', 'first + margin_second on a segment end, second maximum on it', two(5 * S - 6, 5 * S - 1), None),
                ('lower_end_later', 'first + margin_second on a segment end, second maximum on the next knot', two(5 * S - 6, 5 * S), None),
                ('lower_mid', 'first + margin_second mid-segment, second maximum in the straddling segment', two(8 * S + 2, 8 * S + 9), None),
                ('lower_mid_later', 'first + margin_second mid-segment, second maximum in a later segment', two(8 * S + 2, 11 * S + 4), None),
                ('empty', 'empty second range; box with b < a', [(n - 23, FIRST)], None),
                ('L_64', 'L = 64: the left sweep starts on knot 0', two(75, 80), None),
                ('L_65', 'L = 65: the left sweep starts on a centred difference at knot 1', two(76, 81), None),
                ('R_64', 'R + 64 = n - 1: the right sweep starts on the last knot; longer than 64 knots', two(n - 146, n - 86), None),
                ('R_63', 'R + 64 = n - 2: the right sweep starts on a centred difference; longer than 64 knots', two(n - 147, n - 87), None),
                ('long', 'longer than 128 knots: the strided rewrite loop', two(200, 350), None),
                ('one_nan', 'one NaN', [], [(10 * S + 3, nan)]),
                ('two_nan', 'NaN in two segments', [], [(10 * S + 3, nan), (40 * S + 1, nan)]),
                ('plus_inf', '+inf', [], [(12 * S, inf)]),
                ('minus_inf', '-inf', [], [(12 * S + 5, -inf)]),
                ('zero', 'all-zero sequence: first = margin_first', [], 'zero'),
                ('plain', 'no dip', [], 'plain')]
    if name == 'm20_far':      # margins (20, 4 S + 3), offsets (-10, 20): margin_second beyond a segment (and beyond what a NaN spreads over)
        return [('straddle', 'margin_second beyond a segment, second maximum in the straddling segment', two(2 * S + 1, 6 * S + 9), None),
                ('later', 'margin_second beyond a segment, second maximum in a later segment', two(2 * S + 1, 20 * S), None),
                ('on_start', 'second maximum on first + margin_second on a segment start', two(3 * S - 3, 7 * S), None),
                ('one_nan', 'one NaN', [], [(10 * S + 3, nan)]),
                ('two_nan', 'NaN in two segments', [], [(10 * S + 3, nan), (30 * S + 1, nan)]),
                ('two_inf', 'two +inf', [], [(9 * S, inf), (33 * S + 7, inf)]),
                ('minus_inf', '-inf', [], [(12 * S + 5, -inf)]),
                ('plain', 'no dip', [], 'plain')]
    raise ValueError(name)


def settings(n, name):
    S = n // 64
    return {'m0_0': (0, 0, 0, 0), 'm1_0': (1, 0, 0, 0), 'm1_0_wide': (1, 0, 0, n - 3), 'mhalf_0': (n // 2 - 1, 0, 0, 0), 'm20_5': (20, 5, -10, 20),
            'm20_far': (20, 4 * S + 3, -10, 20)}[name]


GROUPS = ['m0_0', 'm1_0', 'm1_0_wide', 'mhalf_0', 'm20_5', 'm20_far']
COPIES = 3      # every case on three base rows
# (n, group, case, copy): the (sequence, box) blocks over CAP x FLOOR, with the level tests/test_wallish_truth_host.py measures (in FLOORs): not sent to the device
OVER_CAP = {(2048, 'm0_0', 'nr_0', 0): 44.3, (2048, 'm0_0', 'end_l1', 0): 50.8, (2048, 'm20_5', 'R_64', 0): 38.7}      # boxes of one knot where the truth nearly cancels; a box of 91


@functools.lru_cache(maxsize=None)
def unit(n):
    """(7,): U of every base row, 8 x the largest |M| of the row without dips."""
    return 8. * np.abs(m_truth(st.gap_rows(n), dtype='f8')).max(axis=-1)


def sequences(n, name, drop_over_cap=True):
    """([(case, copy, edge, finite)], y (rows, n)) of a group."""
    base, U = st.gap_rows(n), unit(n)
    labels, rows = [], []
    for k, (case, edge, dips, other) in enumerate(cases(n, name)):
        for copy in range(1 if other == 'zero' else COPIES):
            if drop_over_cap and (n, name, case, copy) in OVER_CAP:
                continue
            b = (k + 2 * copy) % st.NBASE
            y = np.zeros(n) if other == 'zero' else base[b].copy()
            for knot, weight in dips:
                y[knot] -= weight * U[b]
            finite = True
            if isinstance(other, list):
                finite = False
                for knot, value in other:
                    y[knot] = value
            labels.append((case, copy, edge, finite))
            rows.append(y)
    return labels, np.array(rows)


def _combine(truth, *restatements):
    """Per block (row) the restatement that lies furthest from the truth: ``spline_truth.levels`` of it is the larger of the levels."""
    dist = np.array([np.abs(r.astype(LD) - truth).max(axis=-1) for r in restatements])
    pick = np.argmax(dist, axis=0)
    return np.array([restatements[p][r] for r, p in enumerate(pick)])


@functools.lru_cache(maxsize=None)
def group(n, name, drop_over_cap=True):
    """dict of one launch: margins, offsets, labels, y, finite (rows,), m_ld / m_f8 (truth and the yardstick that lies furthest, finite rows), boxes
    (rows, 2) of the truth with the offsets (finite rows), and per finite row with a valid box: gap_ld[r] / gap_f8[r] / gap_plain[r] (b - a + 1,): the truth, the
    yardstick that lies furthest and the plain float64 solve (cp_gap_spline's yardstick, tests/test_gap_spline_gpu.py)."""
    mf, ms, off0, off1 = settings(n, name)
    labels, y = sequences(n, name, drop_over_cap)
    finite = np.array([lab[3] for lab in labels])
    fy = y[finite]
    m_ld, m_plain = m_truth(fy), m_truth(fy, dtype='f8')
    m_f8 = _combine(m_ld, m_plain, m_recursive(fy)) if n == 2048 else m_plain
    found_ld, found_f8 = box_rule(m_ld, mf, ms), box_rule(m_plain, mf, ms)
    boxes = np.zeros((len(y), 2), dtype='i8')
    boxes[finite] = found_ld + [off0, off1]
    gap_ld, gap_f8, gap_plain = {}, {}, {}
    for r in np.flatnonzero(finite):
        a, b = (int(v) for v in boxes[r])
        if valid_box(a, b, n):
            gap_ld[r] = st.gap_truth(y[r:r + 1], a, b)[0]
            plain = st.gap_truth(y[r:r + 1], a, b, dtype='f8')
            gap_plain[r] = plain[0]
            gap_f8[r] = _combine(gap_ld[r][None], plain, remove_windowed(y[r:r + 1], a, b, composed=True)[:, a:b + 1])[0] if n == 2048 else plain[0]
    index = np.full(len(y), -1)
    index[finite] = np.arange(finite.sum())
    return dict(n=n, name=name, margins=(mf, ms), offsets=(off0, off1), labels=labels, y=y, finite=finite, index=index, m_ld=m_ld, m_f8=m_f8, m_plain=m_plain,
                found_ld=found_ld, found_f8=found_f8, boxes=boxes, gap_ld=gap_ld, gap_f8=gap_f8, gap_plain=gap_plain)


def describe(n, margins, offsets, found):
    """What a finite sequence with the maxima ``found`` = (first, second) exercises: lanes and places in their segments, where the second range starts,
    and the branches of remove_box* its box takes."""
    S = n // 64
    mf, ms = margins
    first, second = (int(v) for v in found)
    lower = first + ms
    a, b = first + offsets[0], second + offsets[1]
    out = dict(first=first, second=second, lane_first=first // S, place_first=first % S, lower=lower, place_lower=lower % S, empty=lower >= n - mf,
               straddling=(not lower >= n - mf) and second // S == lower // S, box=(a, b), valid=valid_box(a, b, n), search='masked_argmax' if n == 2048 else 'elimination')
    if out['valid']:
        L, R = a - 1, b + 1
        i0, i1 = max(L - GAP_WINDOW, 0), min(R + GAP_WINDOW, n - 1)
        out.update(L=L, R=R, i0=i0, i1=i1, nl=L - 1 - i0, nr=i1 - 1 - R, left_trivial=L == i0, right_trivial=R == i1, left_clamped=i0 == 0, right_clamped=i1 == n - 1,
                   length=b - a + 1)
    return out


def assert_rows_within(dev, truth, f64, what):
    """``spline_truth.assert_within`` row for row (dev already in the scale of the truth); returns the fraction of the allowance used."""
    return st.assert_within(np.asarray(dev).astype(LD), np.asarray(truth), np.asarray(f64), what=what)


def allowance(truth, f64):
    """(rows,): ALLOW x level x top of every block."""
    top, level = st.levels(truth, f64)
    return ALLOW * level * top


def judge(g, rows, m=None, boxes=None, rewritten=None):
    """A result for the finite sequences ``rows`` of a group against its truths, by the rule: m (len(rows), n) within the allowance of its block, boxes
    (len(rows), 2) equal, rewritten (len(rows), n) the input bit for bit outside a valid box (everywhere for an invalid one) and within the allowance of the
    (sequence, box) block inside.  Returns (failures [(row, what, figure)], largest fraction of the allowance used by m, by the rewritten knots)."""
    fails, worst_m, worst_gap = [], 0., 0.
    for k, r in enumerate(rows):
        i = g['index'][r]
        assert i >= 0, 'a sequence that is not finite has no truth'
        if m is not None:
            allowed = allowance(g['m_ld'][i:i + 1], g['m_f8'][i:i + 1])[0]
            dist = np.abs(np.asarray(m[k]).astype(LD) - g['m_ld'][i]).max()
            fraction = float(dist / allowed) if allowed > 0 else (0. if dist == 0 else np.inf)
            worst_m = max(worst_m, fraction) if fraction == fraction else np.inf
            if not fraction <= 1.:
                fails.append((r, 'M', fraction))
        if boxes is not None and tuple(int(v) for v in boxes[k]) != tuple(int(v) for v in g['boxes'][r]):
            fails.append((r, 'box', tuple(int(v) for v in boxes[k])))
        if rewritten is not None:
            y, got = g['y'][r], np.asarray(rewritten[k])
            inside = np.zeros(y.size, dtype=bool)
            if r in g['gap_ld']:
                a, b = (int(v) for v in g['boxes'][r])
                inside[a:b + 1] = True
                allowed = allowance(g['gap_ld'][r][None], g['gap_f8'][r][None])[0]
                dist = np.abs(got[inside].astype(LD) - g['gap_ld'][r]).max()
                fraction = float(dist / allowed) if allowed > 0 else (0. if dist == 0 else np.inf)
                worst_gap = max(worst_gap, fraction) if fraction == fraction else np.inf
                if not fraction <= 1.:
                    fails.append((r, 'rewritten', fraction))
            if not np.array_equal(got[~inside], y[~inside]):
                fails.append((r, 'outside the box', int((got[~inside] != y[~inside]).sum())))
    return fails, worst_m, worst_gap
