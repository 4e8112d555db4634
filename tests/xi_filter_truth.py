"""
Extended-precision truth of ``cp_kirkby2013_rows`` (csrc/cp_xi_filter.hip: the kirkby2013 correlation-function BAO filter, a wave per row), and the
separations, windows, fit ranges and rows that tests/test_xi_filter_edges_gpu.py feeds it.  numpy only, no device.

Truth (:func:`truth`), in ``np.longdouble``, per row with rho the ratio of its cosmology, x = s / rho THE FLOAT64 QUOTIENT (the contract: the kernel
forms it "as the reference does"), promoted:
  precision_i = interp(x_i, knots, weights)               on the fit samples [fit_begin, fit_end)
  center_i    = interp(x_i, knots[2:6], 1 - weights[2:6])  on every sample
  p           = the weighted least-squares fit of (s / 128)^(1 - j), j = 0 .. 4: the normal equations, by elimination in longdouble
  xinow_i     = (1 - center_i) xi_i + center_i fit(s_i)
with ``interp`` np.interp(x, xp, fp, left=0, right=0): fp[-1] exactly at the last knot, 0 beyond it, NaN for a NaN x (:func:`interp`).  Nothing is
special-cased: a non-finite fit (a NaN or inf among the fit samples even at weight 0, where 0 x NaN is NaN; a NaN ratio; no weighted sample at all,
where the first pivot is 0 / 0) makes the whole row NaN through 0 x NaN, as in the kernel; the reference raises LinAlgError in the last case.
tests/test_xi_filter_truth_host.py holds the truth to mpmath at 40 digits and to ``oracle.bao.kirkby2013``.

:func:`restated` is the kernel's algorithm in float64 (without its fused multiply-adds): the window's slopes formed on the host, the 9 Hankel moments
sum w t^(2 - m) and the 5 right-hand sides sum w xi t^(1 - j), an LDL^T solve, the fit by Horner in 128 / s.  The 14 sums in two orders: the kernel's
(``order='wave'``: 64 lane-strided partials, lane l taking the fit samples l, l + 64, ..., then the pairwise tree over lane distances 32, 16, ..., 1)
and plain sequential (``order='sequential'``).  Both are bitwise equivariant under a scaling of xi by 2^e.

Tolerance rule (that of tests/spline_truth.py and tests/fftlog_taps_truth.py) with one change: the scale of a row is not its
largest value -- that is xi at the smallest separation, up to 1e7 times the values between the boxes, and hides them -- but the largest |truth| over
its BLENDED samples, those with knots[2] <= x <= knots[5], the only ones the fit reaches.  Per case (one s grid, window, fit range and set of
ratios, over its seven base rows), ``level`` is the largest distance of a restatement (both orders) from the truth over the blended samples of a
row, relative to that row's scale, floored at FLOOR = 1.1e-16; the device is allowed ALLOW = 16 levels times the row's scale on its blended samples.
Every sample whose blend factor is 0 (outside [knots[2], knots[5]], and on those two knots where the weights there are 1) must come back bit for bit:
fma(0, fit, 1 * xi) is exact; NaN exactly where the truth has it.  A row without blended samples has no allowance and needs none.

Rows (:func:`base_rows`): seven per grid, (30 / s)^2 (1 + 0.3 exp(-((s - 105) / 10)^2 / 2)) times (1 + 0.2 N(0, 1)), seeded by the grid's size.  The
noise is essential: a smooth xi leaves the fit a tiny residual, and a fit sample that the kernel dropped would move the result by 4e-8 of the blended
scale instead of 2e-5 or more (``drop_one``, asserted per case in the host test).  Row i of a batch is base row i % 7 times 2**e_i, |e_i| <= 100,
exactly; the filter is linear in xi, so its truth is that of the base row times 2**e_i.
"""
import functools

import numpy as np

LD = np.longdouble
FLOOR = 1.1e-16
ALLOW = 16.
CAP = 1e-10     # the level of every case used on the device stays below (tests/test_xi_filter_truth_host.py)
NBASE = 7
EXPONENT_RANGE = 100
EXPONENTS = np.random.default_rng(20250311).integers(-EXPONENT_RANGE, EXPONENT_RANGE + 1, 8704)
PIVOT = 128.

KNOTS = np.array([49.5, 50., 82., 82.68, 149.32, 150., 190., 191.9])      # the filter's own: boxes (50, 82), (150, 190), ramps of 1 %
WEIGHTS = np.array([0., 1., 1., 0., 0., 1., 1., 0.])
GENERAL = np.array([0.3, 1., 0.8, 0.1, 0.2, 0.7, 1., 0.4])      # steps at knots[0], knots[7] (precision) and at knots[2], knots[5] (blend)
RATIOS = np.array([1., 0.9, 1.1, 0.75, 1.3, 1.0123456789])      # those of test_xi_filter_batch_gpu.py
# for 1022 to 1500 samples: at a ratio of 2 the right box reaches the end of the filter's fit range, whose last samples -- the last, partial pass of
# a wave -- carry no weight at the ratios above (with them, 126 and 127 samples are over the cap: 1.4e-10 and 1.7e-10)
RATIOS_WIDE = np.concatenate([RATIOS, [2., 0.5]])
# the lists of 5 to 16 samples keep all their box samples inside the boxes for ratios in [0.98, 1.02] only, and a box sample that a ratio moves out
# leaves them fewer than five weighted samples, that is no fit: they run at these
NEAR = np.array([1., 0.98, 1.02, 1.0123456789, 0.99])


# ---- the operation ----------------------------------------------------------------------------------------------------------------------------

def interp(x, xp, fp, dtype=LD, slopes=None):
    """np.interp(x, xp, fp, left=0, right=0) in ``dtype``: fp[j] + slope_j (x - xp[j]) on [xp[j], xp[j + 1]), fp[-1] at xp[-1], 0 outside, NaN for NaN."""
    x64 = np.asarray(x, dtype='f8')
    xp64 = np.asarray(xp, dtype='f8')
    n = xp64.size
    x, xp, fp = x64.astype(dtype), xp64.astype(dtype), np.asarray(fp).astype(dtype)
    if slopes is None:
        slopes = np.diff(fp) / np.diff(xp)
    with np.errstate(invalid='ignore'):
        j = (x64[..., None] >= xp64).sum(axis=-1) - 1
    jc = np.clip(j, 0, n - 2)
    v = slopes[jc] * (x - xp[jc]) + fp[jc]
    v = np.where(j < 0, 0, v)
    v = np.where(j == n - 1, np.where(x64 == xp64[-1], fp[-1], 0), v)
    return np.where(x64 != x64, x, v).astype(dtype)


def x_of(s, rho):
    """The float64 quotient s / rho."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.asarray(s, dtype='f8') / np.float64(rho)


def window_of(s, rho, knots, weights, dtype=LD, host_slopes=False):
    """(precision, center) of every sample.  ``host_slopes``: the slopes rounded to float64 as the entry point forms them."""
    knots, weights = np.asarray(knots, dtype='f8'), np.asarray(weights, dtype='f8')
    x = x_of(s, rho)
    ws = cs = None
    cvalue = 1. - weights[2:6]      # (float64: what the reference hands to np.interp)
    if host_slopes:
        ws = ((weights[1:] - weights[:-1]) / (knots[1:] - knots[:-1])).astype(dtype)
        cs = ((cvalue[1:] - cvalue[:-1]) / (knots[3:6] - knots[2:5])).astype(dtype)
    return interp(x, knots, weights, dtype, ws), interp(x, knots[2:6], cvalue, dtype, cs)


def blended_mask(s, rho, knots):
    """The samples the fit reaches: knots[2] <= x <= knots[5]."""
    x = x_of(s, rho)
    with np.errstate(invalid='ignore'):
        return (x >= knots[2]) & (x <= knots[5])


def _solve(M, R):
    """G p = R with G[j][k] = M[..., j + k] (5 x 5 Hankel, symmetric positive definite) by LDL^T without pivoting, in the type of M, vectorised over
    the leading axes: M (..., 9), R (..., 5) -> p (..., 5).  The kernel's ``solve``."""
    L = [[None] * 5 for _ in range(5)]
    D = [None] * 5
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for j in range(5):
            d = M[..., 2 * j]
            for k in range(j):
                d = d - L[j][k] * L[j][k] * D[k]
            D[j] = d
            for i in range(j + 1, 5):
                a = M[..., i + j]
                for k in range(j):
                    a = a - L[i][k] * L[j][k] * D[k]
                L[i][j] = a / d
        y = [None] * 5
        for i in range(5):
            v = R[..., i]
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v
        p = [None] * 5
        for i in range(4, -1, -1):
            v = y[i] / D[i]
            for k in range(i + 1, 5):
                v = v - L[k][i] * p[k]
            p[i] = v
    return np.stack(np.broadcast_arrays(*p), axis=-1)


def _terms(s, xi, w, dtype):
    """The 14 summands of every fit sample: (nfit, 9) moments w t^(2 - m) and (rows, nfit, 5) right-hand sides w xi t^(1 - j), formed as the kernel
    forms them (t = s / 128, u = 128 / s)."""
    s = np.asarray(s, dtype='f8').astype(dtype)
    t, u = s * dtype(1. / PIVOT), dtype(PIVOT) / s
    u2 = u * u
    u3 = u2 * u
    wt, wu = w * t, w * u
    with np.errstate(invalid='ignore', over='ignore'):
        wx = w * xi
        moments = np.stack([wt * t, wt, w, wu, wu * u, wu * u2, wu * u3, (wu * u2) * u2, (w * u3) * u3], axis=-1)
        rhs = np.stack([wx * t, wx, wx * u, wx * u2, wx * u3], axis=-1)
    return moments, rhs


def _sum(a, axis, order):
    """Sum over ``axis``: 'sequential', or 'wave' -- 64 lane-strided sequential partials, then the pairwise tree over lane distances 32 ... 1."""
    a = np.moveaxis(a, axis, 0)
    with np.errstate(invalid='ignore', over='ignore'):
        if order == 'sequential':
            return np.cumsum(a, axis=0)[-1]
        n = a.shape[0]
        passes = -(-n // 64)
        padded = np.zeros((passes * 64,) + a.shape[1:], dtype=a.dtype)
        padded[:n] = a
        lanes = np.cumsum(padded.reshape((passes, 64) + a.shape[1:]), axis=0)[-1]
        while lanes.shape[0] > 1:
            half = lanes.shape[0] // 2
            lanes = lanes[:half] + lanes[half:]
        return lanes[0]


def _filter(s, xi, rho, fit_begin, fit_end, knots, weights, dtype, order, host_slopes):
    s = np.asarray(s, dtype='f8')
    xi = np.asarray(xi, dtype='f8')
    rows = np.atleast_2d(xi).astype(dtype)
    w, c = window_of(s, rho, knots, weights, dtype, host_slopes)
    fit = slice(fit_begin, fit_end)
    moments, rhs = _terms(s[fit], rows[:, fit], w[fit], dtype)
    M, R = _sum(moments, 0, order), _sum(rhs, 1, order)
    p = _solve(M, R)                                                                 # (rows, 5)
    sd = s.astype(dtype)
    t, u = sd * dtype(1. / PIVOT), dtype(PIVOT) / sd
    with np.errstate(invalid='ignore', over='ignore'):
        curve = (p[:, 0:1] * t + p[:, 1:2]) + u * (u * (u * p[:, 4:5] + p[:, 3:4]) + p[:, 2:3])
        out = c * curve + (1 - c) * rows
    return out.reshape(xi.shape)


def truth(s, xi, rho, fit_begin, fit_end, knots=KNOTS, weights=WEIGHTS):
    """xinow of the rows ``xi`` (..., ns) at the ratio rho, in longdouble."""
    return _filter(s, xi, rho, fit_begin, fit_end, knots, weights, LD, 'sequential', False)


def restated(s, xi, rho, fit_begin, fit_end, knots=KNOTS, weights=WEIGHTS, order='wave'):
    """The kernel's algorithm in float64, the 14 sums in the kernel's order ('wave') or one after the other ('sequential')."""
    return _filter(s, xi, rho, fit_begin, fit_end, knots, weights, np.float64, order, True)


ORDERS = ('wave', 'sequential')


# ---- rows ---------------------------------------------------------------------------------------------------------------------------------

def base_rows(s, seed=0):
    """(7, ns) float64: a power law with a bump at the peak, times (1 + 0.2 N(0, 1))."""
    s = np.asarray(s, dtype='f8')
    rng = np.random.default_rng([s.size, seed, 2013])
    return (30. / s)**2 * (1. + 0.3 * np.exp(-0.5 * ((s - 105.) / 10.)**2)) * (1. + 0.2 * rng.standard_normal((NBASE, s.size)))


def exponents(nrows):
    if nrows > EXPONENTS.size:
        raise ValueError('at most {:d} rows'.format(EXPONENTS.size))
    return EXPONENTS[:nrows]


def batch(base, nrows):
    """(nrows, ns): row i = base[i % 7] * 2**e_i, exactly."""
    return base[np.arange(nrows) % NBASE] * np.ldexp(1., exponents(nrows))[:, None]


def unscale(values):
    """The rows of a device result in longdouble with the 2**e_i of ``batch`` taken out again (exact)."""
    values = np.asarray(values)
    return values.astype(LD) * np.ldexp(LD(1), -exponents(len(values)))[:, None]


def ratio_index(nrows, per_cosmology):
    """The ratio row i reads: i // rows_per_cosmology."""
    return np.arange(nrows) // per_cosmology


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------

class Case(object):
    """s (ns,), fit (begin, end), knots, weights, ratios (nr,), base (7, ns) and, per ratio and base row: truth (nr, 7, ns) longdouble, blend
    (nr, ns) bool, zero (nr, ns) bool (blend factor 0), top (nr, 7) the largest |truth| over the blended samples, level (one number)."""

    def expected(self, nrows, per_cosmology=1, ratio_of_cosmology=None):
        """(truth, blend, zero, top) row for row of the unscaled batch: row i is base row i % 7 at ratio ratio_of_cosmology[i // per_cosmology] (an
        index into the case's ratios; default: cosmology j takes ratio j % nr)."""
        cosmo = ratio_index(nrows, per_cosmology)
        which = cosmo % len(self.ratios) if ratio_of_cosmology is None else np.asarray(ratio_of_cosmology)[cosmo]
        b = np.arange(nrows) % NBASE
        return self.truth[which, b], self.blend[which], self.zero[which], self.top[which, b], which


def make_case(s, fit, knots=KNOTS, weights=WEIGHTS, ratios=RATIOS, label='', seed=0):
    case = Case()
    case.s, case.fit, case.knots, case.weights, case.ratios, case.label = np.asarray(s, dtype='f8'), (int(fit[0]), int(fit[1])), knots, weights, np.asarray(ratios, dtype='f8'), label
    case.ns = case.s.size
    case.base = base_rows(case.s, seed)
    case.truth = np.stack([truth(case.s, case.base, rho, fit[0], fit[1], knots, weights) for rho in case.ratios])
    case.blend = np.stack([blended_mask(case.s, rho, knots) for rho in case.ratios])
    case.zero = np.stack([window_of(case.s, rho, knots, weights)[1] == 0 for rho in case.ratios])
    case.top = np.where(case.blend[:, None, :], np.abs(case.truth), 0).max(axis=-1)
    level = FLOOR
    for order in ORDERS:
        for r, rho in enumerate(case.ratios):
            f64 = restated(case.s, case.base, rho, fit[0], fit[1], knots, weights, order).astype(LD)
            dist = np.where(case.blend[r], np.abs(f64 - case.truth[r]), 0).max(axis=-1)
            with np.errstate(divide='ignore', invalid='ignore'):
                level = max(level, float(np.where(case.top[r] > 0, dist / case.top[r], 0).max()))
    case.level = level
    for a in (case.s, case.base, case.truth, case.blend, case.zero, case.top):
        a.flags.writeable = False
    return case


def check(case, got, nrows, per_cosmology=1, ratio_of_cosmology=None, scaled=True, what='', rows=None):
    """The device's rows ``got`` (nrows, ns) against the case: NaN exactly where the truth has it, the blended samples within ALLOW x level x the
    row's blended scale, every sample of blend factor 0 equal to the input bit for bit.  ``rows`` (bool, nrows): the rows to look at (default all).
    Prints and returns the largest fraction of the allowance used."""
    got = np.asarray(got)
    true, blend, zero, top, which = case.expected(nrows, per_cosmology, ratio_of_cosmology)
    assert got.shape == true.shape, (what, got.shape, true.shape)
    sent = batch(case.base, nrows) if scaled else case.base[np.arange(nrows) % NBASE]
    value = unscale(got) if scaled else got.astype(LD)
    if rows is not None:
        got, true, blend, zero, top, sent, value = (a[rows] for a in (got, true, blend, zero, top, sent, value))
    assert np.array_equal(np.isnan(got), np.isnan(true)), '{}: NaN in other places than the truth has them'.format(what)
    assert np.isfinite(got).all(), what
    same = got.view('u8') == sent.view('u8')
    assert same[zero].all(), '{}: {:d} samples of blend factor 0 differ from the input'.format(what, int((~same[zero]).sum()))
    dist = np.where(blend, np.abs(value - true), 0).max(axis=-1)
    allowed = LD(ALLOW) * LD(case.level) * top
    with np.errstate(divide='ignore', invalid='ignore'):
        fraction = np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0)).astype('f8')
    worst = float(fraction.max()) if fraction.size else 0.
    print('%s: largest fraction of the allowance %.3g (level %.3g)' % (what or case.label, worst, case.level))
    assert worst <= 1., '{}: row {} at {:.3g} of its allowance'.format(what, int(np.argmax(fraction)), worst)
    return worst


def drop_one(case):
    """The smallest move of the case's truth, in allowances, when one fit sample of weight >= 0.5 is left out of the fit (its 14 summands taken off the
    sums): over all ratios and such samples, the move being the largest over the seven base rows and their blended samples, each row in its own
    allowance.  (A kernel that loses a sample loses it in every row, and the device tests look at every row; the least move over single rows is that
    of the one sample among thousands that happens to lie on the fitted curve.)  Where one sample less leaves fewer than five weighted samples the
    fit has no solution, which is no small move: not counted.  inf for a case without blended samples."""
    smallest = np.inf
    b, e = case.fit
    sd = case.s.astype(LD)
    t, u = sd * LD(1. / PIVOT), LD(PIVOT) / sd
    for r, rho in enumerate(case.ratios):
        blend = case.blend[r]
        w, c = window_of(case.s, rho, case.knots, case.weights)
        w = w[b:e]
        chosen = np.flatnonzero(w >= 0.5)
        if not blend.any() or (w > 0).sum() < 6 or not chosen.size:
            continue
        moments, rhs = _terms(case.s[b:e], case.base[:, b:e].astype(LD), w, LD)
        M, R = moments.sum(axis=0), rhs.sum(axis=1)
        p = _solve(M - moments[chosen][:, None, :], R[None] - np.moveaxis(rhs[:, chosen], 1, 0)) - _solve(M, R)      # (chosen, rows, 5)
        tb, ub = t[blend], u[blend]
        curve = (p[..., 0:1] * tb + p[..., 1:2]) + ub * (ub * (ub * p[..., 4:5] + p[..., 3:4]) + p[..., 2:3])
        dist = np.abs(c[blend] * curve).max(axis=-1)                                                                # (chosen, rows)
        allowed = LD(ALLOW) * LD(case.level) * case.top[r]
        smallest = min(smallest, float((dist / allowed).max(axis=-1).min()))
    return smallest


# ---- the grids ------------------------------------------------------------------------------------------------------------------------------

# the five: all in the boxes at every ratio of NEAR (nothing is blended, the fit goes through them); 6: and one between the boxes; 8: and one in
# front of the window; 16: and the 8 knots.  LIST_SEED: of the seeds 0 to 7 the first whose rows stay under the cap in all of the lists (the
# fitted curve through five noisy samples is small at some blended sample of seeds 0 to 2, and the level is relative to it)
FIVE = [52., 61., 79., 156., 184.]
LISTS = {5: FIVE, 6: sorted(FIVE + [110.]), 7: sorted(FIVE + [100., 120.]), 8: sorted(FIVE + [40., 105., 115.]),
         15: sorted(list(KNOTS[:-1]) + FIVE + [70., 110., 170.]), 16: sorted(list(KNOTS) + FIVE + [70., 110., 170.])}
LIST_SEED = 3


def grid(ns):
    """(s, fit): from 32 samples on np.geomspace(20, 400, ns) and the filter's own fit range 25 <= s <= 380; below, a fixed list inside [40, 250],
    all of it fitted."""
    if ns < 32:
        s = np.array(LISTS[ns])
        return s, (0, ns)
    s = np.geomspace(20., 400., ns)
    index = np.flatnonzero((s >= 25.) & (s <= 380.))
    return s, (int(index[0]), int(index[-1]) + 1)


STAGED_SIZES = [6, 8, 16, 126, 128, 130, 1022, 1024]
ANY_SIZES = [5, 7, 127, 129, 1023, 1026, 1500]


@functools.lru_cache(maxsize=None)
def size_case(ns, general=False):
    s, fit = grid(ns)
    return make_case(s, fit, KNOTS, GENERAL if general else WEIGHTS, (RATIOS_WIDE if ns >= 1000 else RATIOS) if ns >= 32 else NEAR[:4], 'ns %d%s' % (ns, ' general weights' if general else ''),
                     seed=0 if ns >= 32 else LIST_SEED)


# B. fit ranges of other lengths than the filter picks, on 256 samples.  63 neighbours of np.geomspace(20, 400, 256) span a factor 2.07 in s, on which the
# five powers are too much alike (level 7e-8, found here), and a range that holds the filter's window and little else gives 2e-10 to 1e-9.  Instead: a
# window of the filter's shape with the boxes (40, 80) and (160, 320); the samples of the fit range np.geomspace(36, hi, length), those in front of it
# on [20, 36), those behind it on (hi, 400].  hi = 300: the range cuts through the right box (its last samples, those of the last partial pass of the
# wave, carry weight 1 at most ratios); hi = 154 with the weights RANGE_GENERAL: the range ends between the boxes and leaves 3 to 10 blended samples
# outside (the samples between the boxes carry weight 0.5 to 0.6 there, so that the fit has something to hold on to: with 0.1 to 0.2 the level is
# 1e-10 to 6e-10).
RANGE_NS = 256
RANGE_KNOTS = np.array([39.6, 40., 80., 80.8, 159.2, 160., 320., 323.2])
RANGE_GENERAL = np.array([0.3, 1., 0.8, 0.5, 0.6, 0.7, 1., 0.4])
RANGE_LENGTHS = [63, 64, 65, 127, 128, 129, 193]
RANGE_STARTS = [0, 1, 37]
RANGE_RATIOS = np.array([1., 0.9, 0.95, 1.0123456789, 1.05, 0.85])
RANGES = [(b, n) for n in RANGE_LENGTHS for b in RANGE_STARTS] + [(RANGE_NS - 193, 193), (RANGE_NS - 65, 65)]      # the last two end at ns
RANGES_SHORT = [(37, 129), (0, 65)]


def range_grid(begin, length, hi):
    return np.concatenate([np.geomspace(20., 36., begin + 1)[:-1], np.geomspace(36., hi, length), np.geomspace(hi, 400., RANGE_NS - begin - length + 1)[1:]])


@functools.lru_cache(maxsize=None)
def range_case(begin, length):
    return make_case(range_grid(begin, length, 300.), (begin, begin + length), RANGE_KNOTS, WEIGHTS, RANGE_RATIOS, 'fit range [%d, %d)' % (begin, begin + length))


@functools.lru_cache(maxsize=None)
def range_case_short(begin, length):
    return make_case(range_grid(begin, length, 154.), (begin, begin + length), RANGE_KNOTS, RANGE_GENERAL, RANGE_RATIOS[[0, 3]],
                     'fit range [%d, %d) ending between the boxes' % (begin, begin + length))


# C. separations on the knots.  For rho in (1, 0.5, 2): every knot times rho (exact), its two float64 neighbours times rho, and knots[2] (1 - 5e-13)
# and knots[5] (1 + 5e-13) times rho (inside maybe_center's margin, blend factor 0); with a grid of 60 (61: the any kernel) samples under them.
EDGE_RATIOS = np.array([1., 0.5, 2., 1.0123456789])


def edge_grid(odd=False):
    special = []
    for rho in EDGE_RATIOS[:3]:
        for k in KNOTS:
            special += [np.nextafter(k, -np.inf) * rho, k * rho, np.nextafter(k, np.inf) * rho]
        special += [KNOTS[2] * (1. - 5e-13) * rho, KNOTS[5] * (1. + 5e-13) * rho]
    s = np.unique(np.concatenate([np.geomspace(20., 400., 61 if odd else 60), special]))
    assert s.size == (61 if odd else 60) + 3 * 26 and (s.size % 2 == 1) == odd
    return s


@functools.lru_cache(maxsize=None)
def edge_case(odd=False, general=True):
    s = edge_grid(odd)
    return make_case(s, (0, s.size), KNOTS, GENERAL if general else WEIGHTS, EDGE_RATIOS, 'knot edges, %d samples, %s weights' % (s.size, 'general' if general else 'default'))


# D to F. many rows at a cheap shape: the lists of 16 (staged) and 15 (any) samples, fitted without their first sample
MANY_ROWS = 8197      # one trip of the grid is 2048 workgroups x 4 waves = 8192 rows
MANY_PER_COSMOLOGY = [1, 3, 8197, 10000]


@functools.lru_cache(maxsize=None)
def many_case(ns):
    return make_case(np.array(LISTS[ns]), (1, ns), KNOTS, WEIGHTS, NEAR, '%d rows of %d samples' % (MANY_ROWS, ns), seed=LIST_SEED)


def many_ratios(per_cosmology):
    """The index into NEAR of every cosmology: drawn from the five, seeded by rows_per_cosmology."""
    ncosmo = -(-MANY_ROWS // per_cosmology)
    return np.random.default_rng([per_cosmology, 5]).integers(0, len(NEAR), ncosmo)


def device_cases():
    """Every case the device tests use, for the host test's cap and drop-one conditions."""
    cases = [size_case(ns) for ns in sorted(STAGED_SIZES + ANY_SIZES)] + [size_case(128, True)]
    cases += [range_case(b, n) for b, n in RANGES] + [range_case_short(b, n) for b, n in RANGES_SHORT]
    cases += [edge_case(odd, general) for odd in (False, True) for general in (True, False)]
    cases += [many_case(16), many_case(15)]
    return cases
