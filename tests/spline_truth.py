"""
Extended-precision truth of the three spline kernels that solve their tridiagonal system in pieces -- ``spline_rows_kernel`` (csrc/cp_spline_rows.hip:
a halo of knots in front of every lane's segment, only the window of knots the queries can see), ``column_spline_kernel`` (csrc/cp_spline.hip: up
to 8 parts per column, 32 knots of halo, per-column knots) and ``gap_spline_kernel`` (csrc/cp_spline.hip: two sweeps of at most 64 knots towards a
gap) -- with the knots and rows that tests/test_spline_rows_edges_gpu.py, test_spline_columns_gpu.py and test_gap_spline_gpu.py feed them.  numpy only.

Truth: a Thomas solve in ``np.longdouble`` over ALL knots, vectorised over rows, with no window, no halo and no parts, of the system for the FIRST
derivatives at the knots (scipy's CubicSpline; the rows kernel solves for the second derivatives: truth and kernel are different formulations),
  h_i s_{i-1} + 2 (h_{i-1} + h_i) s_i + h_{i-1} s_{i+1} = 3 (h_i delta_{i-1} + h_{i-1} delta_i),   h_i = x_{i+1} - x_i,  delta_i = (y_{i+1} - y_i) / h_i
closed by the natural (2 s_0 + s_1 = 3 delta_0), clamped (s_0 = 0: zero end slopes, scipy's 'clamped' and the kernels') or not-a-knot (scipy's
rows) condition.  From the slopes: the values at queries (``extrapolate``: the end cubics continued; NaN outside otherwise, and a NaN query
stays NaN) and the second derivatives at the knots.  ``gap_truth`` is wallish2018's step: z = y x^2 on x = 1 .. n, the knots a .. b dropped, a
clamped spline through the others evaluated at a .. b and divided by x^2.
The same functions with ``dtype='f8'`` are the float64 restatement that gives the rounding level of the tolerance rule.

Tolerance rule (that of tests/jacobian_reference.py), :func:`levels` and :func:`assert_within`: a block is one row (one
column of the column kernel); its level is the float64 restatement's largest distance from the truth relative to the block's largest |truth|,
floored at FLOOR = 1.1e-16; the device is allowed ALLOW = 16 levels.

Knots: the families of tests/spline_tables_cases.py (on [1, 5000]) and two more,
  logk_pad   np.linspace(-3, 0, n - 4) with [-7, -5] in front and [1, 2] behind: brieden2022's log10 k knots as ``_pad_log`` extends them
  sigma_r    np.geomspace(1e-2, 1e7, n): the FFTLog output that sigma_r takes to its radii
Rows: seven base rows per (family, n), a smooth positive function of the knots times uniform(0.5, 1.5) noise; row i of a batch is base row i % 7
times 2**e_i, |e_i| <= 100 (``batch``, the device of tests/transform_truth.py: the product is exact and the spline linear, so the truth of row i
is the truth of its base row times 2**e_i, and ``scale`` and the root of the rows kernel stay finite).
"""
import functools

import numpy as np

import spline_tables_cases as stc

LD = np.longdouble
FLOOR = 1.1e-16
ALLOW = 16.
CAP = 32.      # a case whose level exceeds CAP x FLOOR is not used on the device (tests/test_spline_truth_host.py)
NBASE = 7
EXPONENT_RANGE = 100
EXPONENTS = np.random.default_rng(20240923).integers(-EXPONENT_RANGE, EXPONENT_RANGE + 1, 8704)
BCS = ['natural', 'clamped', 'not-a-knot']
FAMILIES = ['uniform', 'geom1.05', 'saw1.5x16', 'saw2x40', 'alt1e3', 'jitter100', 'logk_pad', 'sigma_r']


def knots(name, n):
    if name == 'logk_pad':
        if n < 6:
            raise ValueError('logk_pad needs at least 6 knots')
        return np.concatenate([[-7., -5.], np.linspace(-3., 0., n - 4), [1., 2.]])
    if name == 'sigma_r':
        return np.geomspace(1e-2, 1e7, n)
    return stc.knots(name, n)


def families(n):
    return [name for name in FAMILIES if not (name == 'logk_pad' and n < 6)]


def base_rows(name, n):
    """(7, n) float64: (1 + 40 u)^-1.5 of the knots mapped onto u in [0, 1] ((1 + x / 50)^-1.5 on sigma_r's grid, the rows of test_spline_rows) times
    uniform(0.5, 1.5) noise."""
    x = knots(name, n)
    rng = np.random.default_rng(104729 * n + FAMILIES.index(name))
    u = x / 2000. if name == 'sigma_r' else (x - x[0]) / (x[-1] - x[0])
    return rng.uniform(0.5, 1.5, (NBASE, n)) * (1. + 40. * u)**-1.5


def exponents(nrows):
    if nrows > EXPONENTS.size:
        raise ValueError('at most {:d} rows'.format(EXPONENTS.size))
    return EXPONENTS[:nrows]


def batch(base, nrows):
    """(nrows, ...): row i = base[i % 7] * 2**e_i, exactly."""
    return base[np.arange(nrows) % NBASE] * np.ldexp(1., exponents(nrows))[:, None]


def unscale(values):
    """The rows of a device result as longdouble with the 2**e_i of ``batch`` taken out again (exact)."""
    values = np.asarray(values)
    return values.astype(LD) * np.ldexp(LD(1), -exponents(len(values)))[(slice(None),) + (None,) * (values.ndim - 1)]


def _thomas(lower, diag, upper, rhs):
    """Rows of tridiagonal systems (..., n) by elimination without pivoting, in the type of the arguments."""
    n = rhs.shape[-1]
    c = np.empty(np.broadcast_shapes(diag.shape, rhs.shape), dtype=rhs.dtype)
    d = np.empty_like(c)
    c[..., 0] = upper[..., 0] / diag[..., 0]
    d[..., 0] = rhs[..., 0] / diag[..., 0]
    for i in range(1, n):
        den = diag[..., i] - lower[..., i] * c[..., i - 1]
        c[..., i] = upper[..., i] / den
        d[..., i] = (rhs[..., i] - lower[..., i] * d[..., i - 1]) / den
    for i in range(n - 2, -1, -1):
        d[..., i] = d[..., i] - c[..., i] * d[..., i + 1]
    return d


def slopes(x, y, bc='natural', dtype=LD):
    """The first derivatives of the spline at its knots, (rows, n): x (n,) or (rows, n), y (rows, n)."""
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    n = x.shape[-1]
    if bc == 'clamped' and n == 2:      # one cubic between two knots with zero slopes
        return np.zeros(y.shape, dtype=dtype)
    if n < 3 or (bc == 'not-a-knot' and n < 4):
        raise ValueError('{} spline through {:d} knots'.format(bc, n))
    h = np.diff(x, axis=-1)
    delta = np.diff(y, axis=-1) / h
    lower, diag, upper = (np.zeros(x.shape, dtype=dtype) for _ in range(3))
    rhs = np.zeros(y.shape, dtype=dtype)
    lower[..., 1:-1] = h[..., 1:]
    diag[..., 1:-1] = 2 * (h[..., :-1] + h[..., 1:])
    upper[..., 1:-1] = h[..., :-1]
    rhs[..., 1:-1] = 3 * (h[..., 1:] * delta[..., :-1] + h[..., :-1] * delta[..., 1:])
    if bc == 'natural':
        diag[..., 0], upper[..., 0], rhs[..., 0] = 2, 1, 3 * delta[..., 0]
        lower[..., -1], diag[..., -1], rhs[..., -1] = 1, 2, 3 * delta[..., -1]
    elif bc == 'clamped':
        diag[..., 0] = diag[..., -1] = 1
    elif bc == 'not-a-knot':
        d = x[..., 2] - x[..., 0]
        diag[..., 0], upper[..., 0] = h[..., 1], d
        rhs[..., 0] = ((h[..., 0] + 2 * d) * h[..., 1] * delta[..., 0] + h[..., 0]**2 * delta[..., 1]) / d
        d = x[..., -1] - x[..., -3]
        lower[..., -1], diag[..., -1] = d, h[..., -2]
        rhs[..., -1] = (h[..., -1]**2 * delta[..., -2] + (2 * d + h[..., -1]) * h[..., -2] * delta[..., -1]) / d
    else:
        raise ValueError('unknown end condition {}'.format(bc))
    return _thomas(lower, diag, upper, rhs)


def second_derivatives(x, y, s, side='knots'):
    """The second derivatives of the piecewise cubic with slopes s: 'left' / 'right' (rows, n - 1), at the lower / upper end of every interval;
    'knots' (rows, n): the lower ends and the upper end of the last interval."""
    dtype = s.dtype
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    h = np.diff(x, axis=-1)
    delta = np.diff(y, axis=-1) / h
    left = (6 * delta - 4 * s[..., :-1] - 2 * s[..., 1:]) / h
    right = (2 * s[..., :-1] + 4 * s[..., 1:] - 6 * delta) / h
    if side == 'left':
        return left
    if side == 'right':
        return right
    return np.concatenate([left, right[..., -1:]], axis=-1)


def third_derivatives(x, y, s):
    """(rows, n - 1): the third derivative on every interval."""
    dtype = s.dtype
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    h = np.diff(x, axis=-1)
    delta = np.diff(y, axis=-1) / h
    return 6 * (s[..., :-1] + s[..., 1:] - 2 * delta) / h**2


def evaluate(x, y, s, xq, extrapolate=False, nu=0):
    """The piecewise cubic (nu = 1, 2: its first, second derivative) at the shared queries xq (nq,): (rows, nq).  x (n,) or (rows, n).  Outside the
    knots NaN, or the end cubics continued.  A query on an interior knot belongs to the interval that begins there, the last knot to the last interval."""
    dtype = s.dtype
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    xq64 = np.asarray(xq, dtype='f8')
    if x.ndim == 2:
        return np.stack([evaluate(x[r], y[r:r + 1], s[r:r + 1], xq64, extrapolate, nu)[0] for r in range(len(x))])
    n = x.size
    q = xq64.astype(dtype)
    j = np.clip(np.searchsorted(x, q, side='right') - 1, 0, n - 2)
    j = np.where(xq64 != xq64, 0, j)
    h = x[j + 1] - x[j]
    delta = (y[..., j + 1] - y[..., j]) / h
    s0, s1 = s[..., j], s[..., j + 1]
    c2 = (3 * delta - 2 * s0 - s1) / h
    c3 = (s0 + s1 - 2 * delta) / h**2
    t = q - x[j]
    if nu == 0:
        v = y[..., j] + t * (s0 + t * (c2 + t * c3))
    elif nu == 1:
        v = s0 + t * (2 * c2 + 3 * t * c3)
    elif nu == 2:
        v = 2 * c2 + 6 * t * c3
    else:
        raise ValueError('derivative order {}'.format(nu))
    outside = (xq64 != xq64) if extrapolate else ~((xq64 >= float(x[0])) & (xq64 <= float(x[-1])))
    v[..., outside] = np.nan
    return v


def spline(x, y, xq, bc='natural', extrapolate=False, dtype=LD, nu=0):
    return evaluate(x, y, slopes(x, y, bc, dtype), xq, extrapolate, nu)


def knot_second_derivatives(x, y, bc='natural', dtype=LD):
    return second_derivatives(x, y, slopes(x, y, bc, dtype))


def gap_truth(y, a, b, dtype=LD):
    """(rows, b - a + 1): the clamped spline through z = y x^2 at x = 1 .. n without the knots a .. b (indices), at those knots, over x^2."""
    y = np.asarray(y).astype(dtype)
    n = y.shape[-1]
    if not (1 <= a <= b <= n - 2):
        raise ValueError('box ({}, {}) of {} knots'.format(a, b, n))
    x = np.arange(1, n + 1)
    keep = np.concatenate([np.arange(a), np.arange(b + 1, n)])
    xk, zk = x[keep].astype(dtype), y[..., keep] * x[keep].astype(dtype)**2
    xq = x[a:b + 1].astype('f8')
    return spline(xk, zk, xq, 'clamped', dtype=dtype) / xq.astype(dtype)**2


def levels(truth, f64):
    """(top, level), each (rows,): per block (row) the largest |truth| and the rounding level of the float64 restatement.  NaN entries (queries
    outside the knots) must agree and do not count."""
    truth, f64 = np.asarray(truth), np.asarray(f64).astype(LD)
    assert np.array_equal(np.isnan(truth), np.isnan(f64))
    nan = np.isnan(truth)
    top = np.where(nan, 0, np.abs(truth)).max(axis=-1)
    dist = np.where(nan, 0, np.abs(f64 - truth)).max(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        level = np.where(top > 0, dist / top, 0)
    return top, np.maximum(np.asarray(level, dtype='f8'), FLOOR)


def assert_within(dev, truth, f64, what='', scaled=False):
    """Every row of the device's result within ALLOW x its level of the truth, NaN exactly where the truth has NaN; prints and returns the largest
    fraction of the allowance used.  truth, f64: (7, m) with dev (nrows, m) row i belonging to base row i % 7 (``scaled``: times 2**e_i), or row
    for row."""
    dev = np.asarray(dev)
    top, level = levels(truth, f64)
    got = unscale(dev) if scaled else dev.astype(LD)
    if len(dev) != len(truth) or scaled:
        index = np.arange(len(dev)) % NBASE
        truth, top, level = np.asarray(truth)[index], top[index], level[index]
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert np.array_equal(np.isnan(got), np.isnan(truth)), '{}: NaN in other places than the truth has them'.format(what)
    assert np.isfinite(got[~np.isnan(truth)]).all(), what
    dist = np.where(np.isnan(truth), 0, np.abs(got - truth)).max(axis=-1)
    allowed = ALLOW * level * top
    with np.errstate(divide='ignore', invalid='ignore'):
        fraction = np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0))
    worst = float(fraction.max())
    print('%s: largest fraction of the allowance %.3g (level at most %.3g FLOOR)' % (what, worst, float(level.max() / FLOOR)))
    assert worst <= 1., '{}: row {} at {:.3g} of its allowance'.format(what, int(np.argmax(fraction)), worst)
    return worst


# ---- the cases of the rows kernel, shared by the host and the device tests (computed once per process) -------------------------------------------

def rows_halo(x, bc):
    """The halo ``cp_spline_rows_plan_create`` chooses: the smallest multiple of 8 after which 1e-18 of a sweep's start is left (or the first one
    >= n); None beyond 128, where the plan is refused."""
    x = np.asarray(x, dtype='f8')
    n = x.size
    h = np.append(np.diff(x), x[-1] - x[-2])
    sub, diag, sup = np.zeros(n), np.zeros(n), np.zeros(n)
    sub[1:-1], diag[1:-1], sup[1:-1] = h[:-2], 2. * (h[:-2] + h[1:-1]), h[1:-1]
    diag[0], sup[0] = 2. * h[0], h[0]
    sub[-1], diag[-1] = h[-2], 2. * h[-2]
    open_ends = bc != 'clamped'
    if bc == 'not-a-knot':
        fix = [1. + h[0] / h[1], -h[0] / h[1], 1. + h[n - 2] / h[n - 3], -h[n - 2] / h[n - 3]]
        diag[1] += h[0] * fix[0]; sup[1] += h[0] * fix[1]; sub[1] = 0.      # noqa: E702
        diag[n - 2] += h[n - 2] * fix[2]; sub[n - 2] += h[n - 2] * fix[3]; sup[n - 2] = 0.      # noqa: E702
    inv, c, q = np.zeros(n), np.zeros(n), np.zeros(n)
    inv[0] = 0. if open_ends else 1. / diag[0]
    c[0] = sup[0] * inv[0]
    for i in range(1, n):
        inv[i] = 0. if (open_ends and i == n - 1) else 1. / (diag[i] - sub[i] * c[i - 1])
        c[i], q[i] = sup[i] * inv[i], sub[i] * inv[i]
    q, c = np.abs(q), np.abs(c)
    halo = 8
    while True:
        if halo > 128:
            return None
        if halo >= n:
            return halo
        f, b = np.ones(n - halo), np.ones(n - halo)
        for t in range(halo):
            f *= q[halo - t:n - t]
            b *= c[halo - t - 1:n - t - 1]
        if max(f.max(), b.max()) < 1e-18:
            return halo
        halo += 8


def rows_layout(nw, halo):
    """(R, S, lds_bytes) of a window of nw knots: ``cp_spline_rows_plan_create``'s formulas.  R follows the window's length (4 up to 16 x 27 knots,
    2 up to 32 x 59) and is halved while the 4 R row buffers of a workgroup and the factor table exceed 160 KiB."""
    R = 4 if nw <= 16 * 27 else (2 if nw <= 32 * 59 else 1)
    while True:
        lpr = 64 // R
        S = ((nw + lpr - 1) // lpr) | 1
        pad = halo + 1
        nslots = lpr * S + pad
        rstride = lpr * S + 2 * pad + 1
        lds = (((4 * R * rstride + 3) & ~3) + 4 * nslots) * 8
        if lds <= 160 * 1024 or R == 1:
            return R, S, lds
        R //= 2


ROWS_LARGEST_FAMILIES = ['uniform', 'sigma_r']


def rows_largest(halo=32):
    """(n, uniform knots): the largest all-knots window that fits the 160 KiB of LDS with this halo."""
    n = max(nw for nw in range(1889, 4097) if rows_layout(nw, halo)[2] <= 160 * 1024)
    return n, knots('uniform', n)


@functools.lru_cache(maxsize=None)
def rows_case(name, n, bc):
    """dict of one (family, n, end condition): x, y (7, n) and, for all-knots queries, values / second derivatives in longdouble and in float64."""
    x, y = knots(name, n), base_rows(name, n)
    case = dict(x=x, y=y)
    for key, dtype in (('ld', LD), ('f8', 'f8')):
        s = slopes(x, y, bc, dtype)
        case['s_' + key] = s
        case['m_' + key] = second_derivatives(x, y, s)
    return case


def rows_values(case, xq, extrapolate=False):
    """(truth, float64 restatement) of a case at the queries xq."""
    return tuple(evaluate(case['x'], case['y'], case['s_' + key], xq, extrapolate) for key in ('ld', 'f8'))


# S = 1; R: 4 -> 2 between 432 and 433 knots; 2 -> 1 between 1632 and 1633 (halo 32: two rows per wave no longer fit the LDS); 1888 and 1889, the end of
# R = 2 by the length of its lanes, which no halo lets it reach
ROWS_SIZES = [5, 8, 9, 432, 433, 1632, 1633, 1888, 1889]
ROWS_R = {5: 4, 8: 4, 9: 4, 432: 4, 433: 2, 1632: 2, 1633: 1, 1888: 1, 1889: 1}      # with a halo of 32
ROWS_TRIPS = [('sigma_r', 2000, 1034, 22), ('uniform', 432, 8203, 13)]      # (family, n, rows, group): more rows than one trip of the grid, R = 1 and R = 4
ROWS_EDGES = [(1000, 300, 400), (1000, 0, 50), (1000, 949, 999), (2000, 700, 1400)]      # (n, first, last knot the queries reach): R = 4, 4, 4, 2
ROWS_EXTRAPOLATED = [433, 9]
# (family, n, end condition, output), '*' for all: over the cap of CAP x FLOOR in the float64 restatement and therefore not used on the device, with the
# level measured by tests/test_spline_truth_host.py (in FLOORs).  The restatement forms second derivatives as (6 delta - 4 s_i - 2 s_{i+1}) / h, which
# cancels where spacings of 1 and 1e-3 alternate; the not-a-knot condition carries that into the values of the end intervals; np.geomspace(1e-2, 1e7, n)
# with n < 10 has neighbouring knots a factor 10 to 178 apart, which no sigma_r grid has.  saw2x40, expected to be the family over the cap, is not.
ROWS_OVER_CAP = {('alt1e3', '*', '*', 'm'): '1565 to 5682', ('alt1e3', '*', 'not-a-knot', 'values'): '1352 to 3343',
                 ('sigma_r', 5, '*', '*'): 'up to 1822', ('sigma_r', 8, '*', '*'): 'up to 177', ('sigma_r', 9, '*', '*'): 'up to 93',
                 ('saw1.5x16', 9, 'not-a-knot', 'm'): 85.6, ('saw2x40', 5, 'not-a-knot', 'm'): 38.6, ('saw2x40', 432, 'not-a-knot', 'm'): 91.1,
                 ('jitter100', 1889, 'not-a-knot', 'm'): 32.8}


def rows_used(name, n, bc, what):
    """Whether the device tests use (family, n, end condition) for ``what`` = 'values' or 'm' (second derivatives)."""
    if n < 6 and name == 'logk_pad':
        return False
    return not any(all(k in ('*', v) for k, v in zip(key, (name, n, bc, what))) for key in ROWS_OVER_CAP)


def rows_queries(x, first=0, last=None, seed=0):
    """Queries that reach the knots first .. last and no others: those knots themselves, the midpoints of their intervals and a random point in
    each."""
    x = np.asarray(x)
    last = x.size - 1 if last is None else last
    lo, hi = x[first:last], x[first + 1:last + 1]
    inside = lo + np.random.default_rng(seed).uniform(0., 1., lo.size) * (hi - lo)
    return np.unique(np.clip(np.concatenate([x[first:last + 1], 0.5 * (lo + hi), inside]), x[first], x[last]))


def rows_beyond(x):
    """Queries for ``extrapolate=True``: beyond both ends by a quarter, a half and one of the end intervals, a NaN, the end knots, and inside."""
    h0, h1 = x[1] - x[0], x[-1] - x[-2]
    inside = rows_queries(x)[::3]
    return np.concatenate([x[0] - np.array([1., 0.5, 0.25]) * h0, inside[:inside.size // 2], [np.nan], inside[inside.size // 2:], x[-1] + np.array([0.25, 0.5, 1.]) * h1])


# ---- the column kernel -------------------------------------------------------------------------------------------------------------------------

COLUMN_SIZES = [3, 4, 81, 160, 161, 162, 241, 641, 642, 721, 1000]
COLUMN_PARTS = [1, 1, 1, 1, 2, 2, 3, 8, 8, 8, 8]      # min(max((n - 1) // 80, 1), 8)
COLUMN_COUNTS = [1, 63, 64, 65, 130]
COLUMN_FAMILIES = ['uniform', 'geom1.05', 'saw2x40', 'logk_pad', 'sigma_r']
# alt1e3 (up to 34 FLOOR at n = 642, 1000), jitter100 (36.3 at n = 241) and saw1.5x16 (32.9 at n = 641) are over the cap at one size or more: not used
COLUMN_HALO = 32
COLUMN_RANGE = (0., 1120.)      # every column's knots lie inside


def column_run(n, parts):
    return (n - 1 + parts - 1) // parts


def column_knots(n, ncol=max(COLUMN_COUNTS)):
    """(ncol, n): column c holds family c % 5 mapped onto [0, 1000], stretched by its own factor in [0.9, 1.1] and shifted by up to 20: the knots at
    which one part of a column ends and the next begins differ from column to column.  Column c does not depend on ncol."""
    rng = np.random.default_rng(977 * n)
    factor, shift = rng.uniform(0.9, 1.1, max(COLUMN_COUNTS)), rng.uniform(0., 20., max(COLUMN_COUNTS))
    x = np.empty((ncol, n))
    for c in range(ncol):
        name = COLUMN_FAMILIES[c % len(COLUMN_FAMILIES)]
        if name == 'logk_pad' and n < 6:
            name = 'uniform'
        k = knots(name, n)
        x[c] = shift[c] + factor[c] * 1000. * (k - k[0]) / (k[-1] - k[0])
    assert (np.diff(x, axis=-1) > 0.).all() and x.min() >= COLUMN_RANGE[0] and x.max() <= COLUMN_RANGE[1]
    return x


def column_values(n, ncol=max(COLUMN_COUNTS)):
    x = column_knots(n)
    rng = np.random.default_rng(977 * n + 1)
    return (rng.uniform(0.5, 1.5, x.shape) * (1. + x / 25.)**-1.5)[:ncol]


def column_queries(n):
    """The shared ascending queries of size n: random ones over the range of all columns (so above the last knot of some), without those that fall into
    a run of intervals of column 0; for column 0 its first and last knot and every knot at which a part begins, exactly; 24 queries in one of its
    intervals; two below and two above every column."""
    x = column_knots(n, 1)[0]
    parts = COLUMN_PARTS[COLUMN_SIZES.index(n)]
    run = column_run(n, parts)
    rng = np.random.default_rng(977 * n + 2)
    q = rng.uniform(COLUMN_RANGE[0], COLUMN_RANGE[1], 160)
    exact = [x[0], x[-1]] + [x[part * run] for part in range(1, parts) if part * run < n - 1]
    if n >= 81:
        empty = (n // 3, n // 3 + 5)      # no query between these knots of column 0 ...
        q = q[(q < x[empty[0]]) | (q > x[empty[1]])]
        crowded = n // 2 + 1      # ... and 24 in this interval
        q = np.concatenate([q, x[crowded] + rng.uniform(0., 1., 24) * (x[crowded + 1] - x[crowded])])
    return np.unique(np.concatenate([q, exact, [-50., -10., 5000., 1e4]]))


@functools.lru_cache(maxsize=None)
def column_case(n):
    """x, y (130, n), xq and (truth, float64 restatement) (130, nq) of the natural splines of size n."""
    x, y, xq = column_knots(n), column_values(n), column_queries(n)
    return dict(x=x, y=y, xq=xq, ld=spline(x, y, xq, 'natural'), f8=spline(x, y, xq, 'natural', dtype='f8'))


# ---- the gap spline --------------------------------------------------------------------------------------------------------------------------

GAP_BOXES = {300: [(1, 1), (1, 298), (65, 70), (66, 70), (150, 150), (100, 234), (100, 233)], 4: [(1, 1), (1, 2), (2, 2)]}
GAP_INVALID = {300: [(0, 5), (5, 299), (7, 6)], 4: [(0, 1), (2, 3), (2, 1)]}
GAP_COUNTS = [1, 37]


def gap_rows(n):
    """(7, n): DST-like decaying rows with a bump, those of test_wallish_dd_box; four knots: positive decaying rows (a box of one knot is a block of one
    value, which has no scale where rows of both signs make it cancel)."""
    rng = np.random.default_rng(31 * n)
    x = 1. + np.arange(n)
    if n == 4:
        return rng.uniform(0.5, 1.5, size=(NBASE, n)) / x**1.5
    return rng.normal(size=(NBASE, n)) / x**1.5 + 3e-3 * np.exp(-0.5 * ((x - 0.35 * n) / 12.)**2) * rng.uniform(0.5, 2., size=(NBASE, 1))


@functools.lru_cache(maxsize=None)
def gap_case(n, a, b):
    """(truth, float64 restatement), each (7, b - a + 1)."""
    y = gap_rows(n)
    return gap_truth(y, a, b), gap_truth(y, a, b, dtype='f8')
