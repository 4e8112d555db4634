"""Extended-precision truth of the two (k, z) table-row kernels of csrc/cp_spline.hip -- ``tables_rows_kernel`` (cp_tables_rows: both spline operators on
the matrix cores) and ``tables_rows_direct_kernel`` (cp_tables_rows_direct: the k spline evaluated from the tables' second derivatives, the z operator on
the matrix cores) -- and the cases that put them on their launch, tile and route edges.  numpy only; shared by tests/test_tables_truth_host.py and
tests/test_tables_truth_gpu.py.

Truth          out[b, zq, q] = f(scale sum_zi Wz[zq, zi] S_k(T[b, zi])(k_q)) entirely in longdouble: S_k the not-a-knot spline of spline_truth (the Thomas
               solve over all knots, the cubic of the query's interval, NaN outside the knots), Wz the spline operator of linop_truth.operator_truth
               (the spline of the unit rows: not-a-knot, natural with 2 or 3 knots where a line / a natural spline is all there is; ``extrapolate``
               continues the end cubics, without it a redshift outside the knots is a NaN row), f the identity, the root or 10^x (linop_truth.exp10_truth).
               For the direct kernel the device is handed the second derivatives the library computes (SplineRows.second_derivatives); its truth is
               this one, the truth of the spline, not that of those float64 M.
Restatement    the same formula in float64 numpy: the float64 Thomas solve, the float64 operator of the unit rows, numpy's product.
Rule           DESIGN.md section 5: a block is one table's output; distances against the table's largest |argument|; the level the restatement's distance
               floored at FLOOR = 1.1e-16; ALLOW = 16 levels; a case is used while its level is at most CAP = 32 floors (tests/test_tables_truth_host.py).
               The level is always that of the ARGUMENT of f.  Roots are held squared with SQRT_EXTRA = 3 FLOOR of the value added; behind 10^x the
               relative distance from the longdouble 10^x is at most ln 10 times the argument's allowance + EXP10_EXTRA (linop_truth).  Where 10^x is
               subnormal the allowance is absolute: that relative part of the truth + SUBNORMAL_UNITS = 2 units of 2^-1074 (one rounding of ldexp on top
               of the form's own); where it rounds to 0 or leaves the doubles the answer is 0 / Inf exactly, and either answer counts inside the allowance
               around the two thresholds.
Tables         (1 + 40 u)^-1.5 along k (spline_truth's rows) times 1 + 0.2 cos along z times uniform(0.9, 1.1) noise per entry, times an amplitude
               per table: arguments of order one.  'signed': the same minus 0.05, negative in the tail of every row (roots of negative elements).
               'bump' (the exponent route): 1 + 0.15 exp(-((u - u0) / 0.025)^2) on uniform knots, u0 the middle of ONE tile of 16 wavenumbers, times
               1 + 0.002 cos along z: with ``scale`` = target / (the largest truth of that tile) the tile's largest |argument| is the target and every other
               tile stays below 299 (the host test holds every case to the side of 300 / 308.25 / -323.3 it claims, in longdouble).
"""
import functools

import numpy as np

import linop_truth as lt
import spline_truth as st
from spline_truth import LD, FLOOR, ALLOW, CAP

POST = {None: 0, 'sqrt': 1, 'exp10': 2}      # CP_SPLINE_POST_*
SUBNORMAL_UNITS = 2.
TINY = LD(2) ** -1074
DBL_MIN, DBL_MAX = LD(2.2250738585072014e-308), LD(1.7976931348623157e308)
K_BC = 'not-a-knot'

BASE = dict(nb=3, nzin=5, n=40, nzq=7, nq=70)
NQ = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513]
NZQ = [1, 15, 16, 17, 63, 64]
NZQ_NQ = [64, 80]
NZIN = [2, 3, 4, 15, 16, 17, 31, 32]
N_KNOTS = [4, 5, 16, 17, 100, 504]
TINY_TABLES = dict(nzin=4, n=8, nzq=3)
DIRECT_BATCHES = {256: [2047, 2048, 2049], 513: [682, 683, 1365]}      # nq -> tables: around the 2048 workgroups (one tile per row), the grid of 2046 (three)
ROWS_BATCHES = {256: [511, 512, 513, 1025], 300: [255, 256, 257, 513]}  # nq -> tables: 511 ... 1025 items of one tile, 510 ... 1026 items of two tiles per row
SCALES = [1., -0.5, 2. ** -3]
EXPONENT_TARGETS = {'299.9': 299.9, '300-': float(np.nextafter(300., 0.)), '300': 300., '300.1': 300.1, 'inf': 308.29, 'subnormal': 322.9, 'zero': 331.}
BUMP_TILE = {64: 1, 128: 6}      # nq -> the tile of 16 wavenumbers that holds the bump


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return case


def z_bc(nzin):
    return 'not-a-knot' if nzin >= 4 else 'natural'


def k_queries(x, nq, kind='inside', seed=0):
    """nq ascending wavenumbers that span the knots (the first and the last knot among them, three interior knots from nq = 8 on); 'outside': two below
    the first knot and two above the last (NaN columns, first and last of the row); 'half': the lower half of the knots only (a plan that does not
    span them); 'even': evenly spaced; one query: inside the middle interval."""
    n = x.size
    rng = np.random.default_rng([nq, n, seed, 3])
    if nq == 1:
        return np.array([0.7 * x[n // 2 - 1] + 0.3 * x[n // 2]])
    if kind == 'even':
        return np.linspace(x[0], x[-1], nq)
    hi = x[n // 2] if kind == 'half' else x[-1]
    q = rng.uniform(x[0], hi, nq)
    if nq >= 8:
        q[2:5] = x[[1, n // 4, (n // 2 - 1) if kind == 'half' else n - 2]]
    q = np.sort(q)
    if kind == 'outside':
        assert nq >= 8
        span = x[-1] - x[0]
        q[:3] = [x[0] - 0.01 * span, x[0] - 1e-9 * span, x[0]]
        q[-3:] = [x[-1], x[-1] + 1e-9 * span, x[-1] + 0.02 * span]
    else:
        q[0], q[-1] = x[0], hi
    return q


def z_queries(zk, nzq, kind='beyond', seed=0):
    """nzq ascending redshifts: 'inside' the knots (both ends among them from two on); 'beyond' / 'nan_z': the first below and the last above the knots
    (from three on) -- the end cubics continued, or NaN rows for a plan built without extrapolation."""
    rng = np.random.default_rng([nzq, zk.size, seed, 5])
    span = zk[-1] - zk[0]
    if nzq == 1:
        return np.array([zk[0] + 0.37 * span])
    q = np.sort(rng.uniform(zk[0], zk[-1], nzq))
    q[0], q[-1] = zk[0], zk[-1]
    if kind != 'inside' and nzq >= 3:
        q[0], q[-1] = zk[0] - 0.03 * span, zk[-1] + 0.02 * span
        if nzq >= 5:
            q[1], q[-2] = zk[0], zk[-1]
    if nzq >= 8:
        q[3] = zk[min(1, zk.size - 1)]
        q = np.sort(q)
    return q


def z_operator(nzin, zq, extrapolate, dtype=LD):
    """(nzq, nzin): the spline operator along z on the knots spline_truth.knots('uniform', nzin); two knots: the line through them."""
    zk = st.knots('uniform', nzin)
    if nzin == 2:
        z0, z1 = zk.astype(dtype)
        t = (np.asarray(zq).astype(dtype) - z0) / (z1 - z0)
        w = np.stack([1 - t, t], axis=1)
        if not extrapolate:
            w[(zq < zk[0]) | (zq > zk[1])] = np.nan
        return w
    if dtype is LD:
        return lt.operator_truth('uniform', nzin, z_bc(nzin), 0, zq, extrapolate)
    return np.ascontiguousarray(st.evaluate(zk, np.eye(nzin), st.slopes(zk, np.eye(nzin), z_bc(nzin), dtype), zq, extrapolate).T)


def tables(nb, nzin, n, kind='plain', seed=0, family='geom1.05', u0=0.5):
    """(x (n,), T (nb, nzin, n)): see the module's text."""
    x = st.knots('uniform' if kind == 'bump' else family, n)
    u = (x - x[0]) / (x[-1] - x[0])
    v = np.linspace(0., 1., nzin)
    rng = np.random.default_rng([nzin, n, seed, 11])
    if kind == 'bump':
        shape = 1. + 0.15 * np.exp(-((u - u0) / 0.025) ** 2)
        t = shape[None, None, :] * (1. + 0.002 * np.cos(3. * v)[None, :, None]) * np.ones((nb, 1, 1))
        return x, t
    draws = rng.uniform(0., 1., (nb, 1 + nzin * n))      # (table by table: a longer batch begins with the tables of a shorter one)
    amp = 0.5 + draws[:, :1, None]
    noise = 0.9 + 0.2 * draws[:, 1:].reshape(nb, nzin, n)
    t = amp * noise * ((1. + 40. * u) ** -1.5)[None, None, :] * (1. + 0.2 * np.cos(3. * v[None, :, None] + np.arange(nb)[:, None, None]))
    if kind == 'signed':
        t = t - 0.05 * amp
    return x, t


def arguments(x, t, xq, wz, scale, dtype=LD):
    """(nb, nzq, nq): scale Wz (k spline of T[b]) in ``dtype``; NaN columns for wavenumbers outside the knots, NaN rows for NaN rows of Wz."""
    nb, nzin, n = t.shape
    rows = t.reshape(nb * nzin, n)
    low = st.evaluate(x, rows, st.slopes(x, rows, K_BC, dtype), xq, False).reshape(nb, nzin, xq.size)
    nanz = np.isnan(wz[:, 0])
    nanq = np.isnan(low[0, 0])
    wz0, low0 = np.where(nanz[:, None], 0, wz), np.where(nanq[None, None, :], 0, low)
    if dtype is LD:
        out = np.einsum('zi,biq->bzq', wz0, low0) * LD(scale)
    else:
        out = np.matmul(wz0[None], low0) * scale
    out[:, nanz, :] = np.nan
    out[:, :, nanq] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def case(nb=3, nzin=5, n=40, nzq=7, nq=70, scale=1., kq='inside', zq='beyond', kind='plain', seed=0, u0=0.5, tsign=1.):
    """One case: knots, tables, queries, the truth and the restatement of the ARGUMENT, the level per table (in FLOORs: ``level_floors``)."""
    x, t = tables(nb, nzin, n, kind, seed, u0=u0)
    t = t * tsign
    zk = st.knots('uniform', nzin)
    xq = k_queries(x, nq, kq, seed)
    zqv = z_queries(zk, nzq, zq, seed)
    extrapolate = zq != 'nan_z'
    truth = arguments(x, t, xq, z_operator(nzin, zqv, extrapolate), scale)
    f64 = arguments(x, t, xq, z_operator(nzin, zqv, extrapolate, 'f8'), scale, 'f8')
    top, level = levels(truth, f64)
    return _freeze(dict(x=x, zk=zk, t=t, xq=xq, zq=zqv, extrapolate=extrapolate, scale=scale, truth=truth, f64=f64, top=top, level=level,
                        zbc=z_bc(nzin), level_floors=float(level.max() / FLOOR), shape=(nb, nzin, n, nzq, nq)))


def levels(truth, f64):
    """(top, level), each (nb,): spline_truth.levels with a table's whole output as the block."""
    nb = truth.shape[0]
    return st.levels(truth.reshape(nb, -1), np.asarray(f64).reshape(nb, -1))


def fraction(got, c, post=None, what='', tables_from=0):
    """The largest fraction of its allowance an element of ``got`` (nb, nzq, nq) uses against case ``c``; NaN, 0 and Inf exactly where the truth has them."""
    got64 = np.asarray(got, dtype='f8')
    got = got64.astype(LD)
    nb = got.shape[0]
    arg = c['truth'][tables_from:tables_from + nb]
    assert got.shape == arg.shape, (what, got.shape, arg.shape)
    allowed = (ALLOW * c['level'] * c['top'])[tables_from:tables_from + nb, None, None] * np.ones(arg.shape[1:])
    nan = np.isnan(arg)
    either = np.zeros(arg.shape, dtype=bool)      # elements where two answers count
    if post == 'sqrt':
        near = ~nan & (np.abs(arg) <= allowed)      # the sign of an argument inside its allowance of zero is not the kernel's to know
        nan = nan | (~near & (arg < 0))
        either = near
        err = np.abs(got * got - arg)
        allowed = allowed + lt.SQRT_EXTRA * np.abs(np.where(nan, 0, arg))
    elif post == 'exp10':
        rel = lt.LN10 * allowed + lt.EXP10_EXTRA
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            true = lt.exp10_truth(arg)
            lo, hi = true * (1 - rel), true * (1 + rel)
            must_inf, may_inf = lo > DBL_MAX, hi > DBL_MAX
            must_zero, may_zero = hi < TINY / 2, lo - SUBNORMAL_UNITS * TINY <= 0
            allowed = rel * true + np.where(true < DBL_MIN, SUBNORMAL_UNITS * TINY, 0)
            assert np.array_equal(np.isinf(got64) & ~nan, (may_inf & np.isinf(got64)) & ~nan) and (np.isinf(got64) | ~must_inf | nan).all(), '{}: Inf in other places than the truth'.format(what)
            assert ((got64 == 0) | ~must_zero | nan).all() and (~(got64 == 0) | may_zero | nan).all(), '{}: 0 in other places than the truth'.format(what)
            exact = np.isinf(got64) | (may_inf & ~must_inf) | must_zero
            err = np.where(exact, 0, np.abs(got - true))
    else:
        err = np.abs(got - arg)
    assert np.array_equal(np.isnan(got64) & ~either, nan & ~either), '{}: NaN in other places than the truth has them'.format(what)
    with np.errstate(invalid='ignore', divide='ignore'):
        used = np.asarray(np.where(nan | (either & np.isnan(got64)), 0, err / allowed), dtype='f8')
    worst = float(used.max()) if used.size else 0.
    print('%s: largest fraction of the allowance %.3g (level at most %.3g FLOOR)' % (what, worst, c['level_floors']))
    return worst


# ---- the exponent route ------------------------------------------------------------------------------------------------------------------------------
EXPONENT_SHAPE = dict(nb=2, nzin=12, n=61, nzq=64)


@functools.lru_cache(maxsize=None)
def exponent_case(name, nq, negative_scale=False):
    """Two tables of 12 x 61 uniform knots, 64 redshifts, nq evenly spaced wavenumbers, 10^x: the largest |argument| of ONE tile of 16 wavenumbers
    (BUMP_TILE) is EXPONENT_TARGETS[name] to the rounding of the scale, every other tile stays below 299.  'subnormal' and 'zero': negative arguments.
    negative_scale: the tables negated under the negated scale -- the same arguments."""
    tile = BUMP_TILE[nq]
    u0 = (16 * tile + 7.6) / (nq - 1)
    unit = case(nq=nq, scale=1., kq='even', zq='inside', kind='bump', u0=u0, **EXPONENT_SHAPE)
    peak = np.abs(unit['truth'][:, :, 16 * tile:16 * tile + 16]).max()
    target = EXPONENT_TARGETS[name]
    scale = float(LD(target) / peak)
    while LD(scale) * peak < LD(target):      # the smallest scale that puts the peak AT the target or above it ...
        scale = float(np.nextafter(scale, np.inf))
    while LD(np.nextafter(scale, 0.)) * peak >= LD(target):
        scale = float(np.nextafter(scale, 0.))
    if name == '300-':                        # ... and the largest that leaves it below
        scale = float(np.nextafter(scale, 0.))
    sign = -1. if name in ('subnormal', 'zero') else 1.
    ssign = -1. if negative_scale else 1.
    c = dict(case(nq=nq, scale=ssign * scale, kq='even', zq='inside', kind='bump', u0=u0, tsign=sign * ssign, **EXPONENT_SHAPE))
    c['tile'], c['target'], c['sign'] = tile, target, sign
    return c


def tile_extremes(c):
    """(largest |argument| of the bump's tile, largest of every other tile) in longdouble."""
    a = np.abs(c['truth'])
    lo = 16 * c['tile']
    return a[:, :, lo:lo + 16].max(), np.delete(a, np.arange(lo, lo + 16), axis=2).max()


# ---- 2^20 wavenumbers --------------------------------------------------------------------------------------------------------------------------------
WIDE_NQ = [1 << 20, (1 << 20) + 16]      # the last row length the table-driven 10^x takes, and the first it does not
WIDE_SHAPE = dict(nb=1, nzin=4, n=8, nzq=64)


@functools.lru_cache(maxsize=None)
def wide_case(nq):
    """One tiny table, 64 redshifts inside the knots, nq wavenumbers (0.5 GB of output): the truth of the first and the last 512 columns and of 4096 seeded
    ones (``cols``); the block is the sampled part of the table."""
    x, t = tables(1, 4, 8)
    zk = st.knots('uniform', 4)
    xq = k_queries(x, nq)
    zqv = z_queries(zk, 64, 'inside')
    cols = np.unique(np.concatenate([np.arange(512), np.arange(nq - 512, nq), np.random.default_rng([nq, 17]).integers(0, nq, 4096)]))
    truth = arguments(x, t, xq[cols], z_operator(4, zqv, True), 1.)
    f64 = arguments(x, t, xq[cols], z_operator(4, zqv, True, 'f8'), 1., 'f8')
    top, level = levels(truth, f64)
    return _freeze(dict(x=x, zk=zk, t=t, xq=xq, zq=zqv, extrapolate=True, scale=1., truth=truth, f64=f64, top=top, level=level, zbc=z_bc(4), cols=cols,
                        level_floors=float(level.max() / FLOOR), shape=(1, 4, 8, 64, nq), direct_only=True))
