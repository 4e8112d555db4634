"""
Extended-precision truth of the spliced clamped spline ``cp_splice_apply`` (wallish2018, reference bao_filter.py:415-431) behind both of its kernels --
``splice_uniform_kernel<S>`` (csrc/cp_splice_uniform.h, scheme 1: two recursions per lane on a uniform stretch, junction corrections from host-built
windows) and ``splice_kernel`` (csrc/cp_bao.hip, scheme 0: elimination in LDS with a run-in of ``halo`` knots per lane, any knots) -- with the cases
that tests/test_splice_edges_gpu.py feeds them.  numpy only (the tables of scheme 1 come from the plan builder itself, compiled for the host:
tests/test_splice_host.build).

Truth: the clamped spline through the gathered knots at the queries, ``spline_truth.spline(..., bc='clamped')`` in ``np.longdouble`` (a Thomas solve for
the FIRST derivatives over all knots: both kernels solve for the second), NaN outside the knots; with ``tophat`` p / ((p / v - 1) t + 1) in longdouble.

Tolerance: the rule of tests/spline_truth.py per BLOCK -- one row's queries in the interval in front of the stretch, on the stretch, in the interval
behind it; the whole row for knots without a stretch.  A block's level is the larger distance from the truth of (a) the plain float64 solve and (b) the
float64 restatement of the scheme that runs (scheme 1: tests/test_splice_host.run; scheme 0: :func:`eliminate`), floored at FLOOR; the device gets
ALLOW = 16 levels.  Stretch cases must stay within STRETCH_CAP = 8 FLOOR in every block under both restatements (a condition on the inputs: the
intervals that border the stretch are 2.5 h and 3.5 h long -- second derivatives weigh (H / h)^2 in an interval of length H),
irregular ones within spline_truth.CAP = 32.

Stretch cases: nl knots from array 0, nm uniform knots from columns 3 .. 3 + nm of array 1 (3 spare columns in front, 5 behind), nr knots from array 0;
the outside knots step away geometrically (ratio 1.3) from gaps of 2.5 h in front and 3.5 h behind.  Array 0's grid is [outside-left knots | interior
queries | outside-right knots] and the queries are that grid (nq == n0: the tophat step applies).  Rows: seven base rows, a smooth positive function
times 1 + eps uniform(-1, 1), eps = 0, 0, 1e-6, 1e-6, 1e-3, 1e-3, 1e-3; batches by ``spline_truth.batch`` (the operation is homogeneous of degree 1
with and without tophat).
"""
import functools

import numpy as np

import spline_truth as st
import spline_tables_cases as stc
from test_splice_host import build as uniform_tables, run as uniform_run

LD = st.LD
STRETCH_CAP = 8.
H = 2.**-10      # the spacing of the stretch: every knot of it exactly representable
U0 = 1.
EPS = [0., 0., 1e-6, 1e-6, 1e-3, 1e-3, 1e-3]
SPARE = (3, 5)

# name -> (nm, nl, nr, interior queries)
STRETCH = {}
for _nm in [256, 1320, 1321, 2112, 2113, 2368, 2369, 2624, 2625, 2880, 2881, 3136, 3137, 3392, 3393, 3648]:
    STRETCH['nm%d' % _nm] = (_nm, 50, 30, 400)
for _nl, _nr in [(10, 5), (1, 1), (2, 44), (45, 2), (0, 30), (50, 0), (0, 0)]:
    STRETCH['nm300_%d_%d' % (_nl, _nr)] = (300, _nl, _nr, 400)
STRETCH['gb0'] = (300, 70, 30, 400)          # the first block of 64 queries holds no spline query, the first spline query sits inside a block
STRETCH['generic512'] = (300, 64, 30, 512)   # eight whole blocks of spline queries
STRETCH['generic60'] = (300, 2, 3, 60)       # one block
for _nm in [257, 258, 400]:                  # either side of the constant slot of scheme 0 (more than 256 equal spacings)
    STRETCH['nm%d' % _nm] = (_nm, 50, 30, 400)
# the uniform-stretch scheme does not fit: too many knots for S = 57, too few, nine blocks of spline queries
ELIMINATION_ONLY = {'nm3649': (3649, 50, 30, 400), 'nm255': (255, 50, 30, 400), 'generic513': (300, 64, 30, 513)}
UNIFORM_S = {33: (2112, 1320, 1321, 256), 37: (2368, 2113), 41: (2624, 2369), 45: (2880, 2625), 49: (3136, 2881), 53: (3392, 3137), 57: (3648, 3393)}
BATCH_ROWS = [1, 3, 4, 5]      # and 4 x CUs + 5
# (gap in front, gap behind) in units of h where not (2.5, 3.5).  One knot in front of the stretch: the factor of scheme 0 has come within 2e-11 of its
# constant -- the plan's own threshold -- at knot 10 with 1.7e-11 to spare, and the rows with 1e-3 noise see that as 13.6 FLOOR in the interval there, over
# the cap; with a gap of 1.5 h it is 6e-12 off at the same knot
GAPS = {'nm300_1_1': (1.5, 3.5)}

IRREGULAR_SIZES = [4, 5, 63, 64, 65, 128, 129, 192, 193, 700]
IRREGULAR_FAMILIES = stc.FAMILIES
# (family, n): over CAP x FLOOR in the float64 restatement, not used on the device; the level measured by tests/test_splice_truth_host.py.  alt1e3 (spacings
# of 1 and 1e-3 alternating) cancels in the second derivatives; uniform at 700 knots is the constant slot of the stretch again: the factor is taken as
# converged at knot 10, 2e-11 off, and these rows carry noise of half their size; at 3840 knots the one h0 stands for spacings that differ by the rounding of
# the knots, 4e-13 of h (2699 uniform knots sit at 16 FLOOR)
IRREGULAR_OVER_CAP = {('alt1e3', 65): 37.0, ('alt1e3', 192): 33.6, ('uniform', 700): 45.4, ('uniform', 3840): 2203.}
PIECES = {'two': [(1, 2, 100), (0, 5, 93)], 'three': [(1, 2, 60), (0, 5, 70), (1, 80, 63)]}      # 193 knots of jitter100 from two arrays


# ---- what cp_splice_plan_create chooses, restated ----------------------------------------------------------------------------------------------------

def factors(x):
    """(h, inv, c): spacings (the last one repeated), elimination factors and super-diagonal ratios of the clamped system for the second derivatives."""
    x = np.asarray(x, dtype='f8')
    n = x.size
    h = np.append(np.diff(x), x[-1] - x[-2])
    inv, c = np.empty(n), np.empty(n)
    inv[0] = 1. / (2. * h[0])
    c[0] = h[0] * inv[0]
    for i in range(1, n):
        diag = 2. * (h[i - 1] + h[i]) if i < n - 1 else 2. * h[n - 2]
        inv[i] = 1. / (diag - h[i - 1] * c[i - 1])
        c[i] = h[i] * inv[i]
    return h, inv, c


def longest_run(h, n):
    best = (0, 0)
    lo = 0
    while lo < n - 1:
        hi = lo + 1
        while hi < n - 1 and abs(h[hi] - h[lo]) <= 2e-11 * h[lo]:
            hi += 1
        if hi - lo > best[1] - best[0]:
            best = (lo, hi)
        lo = hi
    return best


def elimination_plan(x):
    """dict(S, halo, ntab_left, uniform_end, lds_bytes, h0, inv0, ...) as ``cp_splice_plan_create`` chooses them; None where it answers CP_EUNSUPPORTED."""
    x = np.asarray(x, dtype='f8')
    n = x.size
    h, inv, c = factors(x)
    qf, qb = np.abs(np.append(0., h[:-1] * inv[1:])), np.abs(c)      # qf[i] = |h[i-1] inv[i]|
    halo = 8
    while True:
        if halo > 128:
            return None
        if halo >= n:
            break
        f, b = np.ones(n - halo), np.ones(n - halo)
        for t in range(halo):
            f *= qf[halo - t:n - t]
            b *= qb[halo - t - 1:n - t - 1]
        if max(f.max(), b.max()) < 1e-18:
            break
        halo += 8
    lo, hi = best = longest_run(h, n)
    L = U = n
    h0 = inv0 = 1.
    if hi - lo > 256:
        mid = (lo + hi) // 2
        h0, inv0 = h[mid], inv[mid]
        a = lo + 1
        while a < hi and abs(inv[a] - inv0) > 2e-11 * inv0:
            a += 1
        b = hi
        while b > a and abs(inv[b - 1] - inv0) > 2e-11 * inv0:
            b -= 1
        if b - a > 128:
            L, U = a, b
    if n > 64 * 60:
        return None
    S = ((n + 63) // 64) | 1
    pad = halo + 1
    nslots = L + 1 + (64 * S + pad - U)
    lds = (4 * (64 * S + 2 * pad + (halo & 1)) + 4 * nslots) * 8
    if lds > 160 * 1024:
        return None
    return dict(n=n, S=S, halo=halo, ntab_left=L, uniform_end=U, lds_bytes=lds, h0=h0, inv0=inv0, h=h, inv=inv, c=c, run=best)


def layout_of(plan):
    return {key: plan[key] for key in ('S', 'halo', 'ntab_left', 'uniform_end', 'lds_bytes')}


def eliminate(x, y, plan, xq, mistake=None):
    """``splice_kernel`` restated in float64: y (rows, n) gathered knot values -> the spline at xq (rows, nq), NaN outside the knots.  A lane per S knots,
    both sweeps started ``halo`` knots outside its segment from zero, the plan's factors -- the constants h0, inv0 where the plan uses its one slot for the
    stretch --, the A / B weights of the queries as the plan forms them.
    ``mistake`` (tests/test_splice_truth_host.py; never made in the library): 'halo8', the run-ins cut to 8 knots; 'slot_early', the stretch's slot used
    from one knot too early."""
    assert mistake in (None, 'halo8', 'slot_early')
    x, y = np.asarray(x, dtype='f8'), np.asarray(y, dtype='f8')
    n, S, halo = plan['n'], plan['S'], plan['halo']
    L, U = plan['ntab_left'], plan['uniform_end']
    h, inv, c = plan['h'], plan['inv'], plan['c']
    pad = halo + 1
    run_in = 8 if mistake == 'halo8' else halo
    if mistake == 'slot_early':
        L = L - 1
    index = np.arange(-pad, 64 * S + pad)      # buf[i] = ext[i + pad]
    at = np.clip(index, 0, n - 1)
    on_stretch = (index >= L) & (index < U)
    cx = np.where(on_stretch, 6. / plan['h0'], 6. * (1. / h)[at])
    cy = np.where(on_stretch, plan['inv0'], inv[at])
    cz = np.where(on_stretch, plan['h0'] * plan['inv0'], np.where(at > 0, h[np.maximum(at - 1, 0)] * inv[at], 0.))
    cw = np.where(on_stretch, plan['h0'] * plan['inv0'], c[at])
    Y = y[:, at]
    own = S * np.arange(64)
    g = lambda a, i: a[..., i + pad]      # noqa: E731
    # forward sweep
    start = own - run_in
    y0 = g(Y, start)
    d = np.zeros_like(y0)
    sigma_m = (y0 - g(Y, start - 1)) * g(cx, start - 1)
    D = Y.copy()      # (beyond the segments the buffer still holds knot values)
    for t in range(run_in + S):
        i = start + t
        yp = g(Y, i + 1)
        sigma = (yp - y0) * g(cx, i)
        d = -g(cz, i) * d + g(cy, i) * (sigma - sigma_m)
        if t >= run_in:
            D[:, i + pad] = d
        sigma_m, y0 = sigma, yp
    # backward sweep
    M = np.zeros((len(y), 64 * S))
    m = np.zeros_like(d)
    for t in range(run_in + S):
        i = own + S + run_in - 1 - t
        dd = g(D, i)
        m = np.where(i >= n - 1, dd, -g(cw, i) * m + dd)
        if t >= run_in:
            M[:, i] = m
    M = M[:, :n]
    # evaluation
    xq = np.asarray(xq, dtype='f8')
    inside = (xq >= x[0]) & (xq <= x[-1])
    j = np.where(inside, np.clip(np.searchsorted(x, np.where(inside, xq, x[0]), side='right') - 1, 0, n - 2), 0)
    a, b = (x[j + 1] - xq) / h[j], (xq - x[j]) / h[j]
    wz, ww = (a * a * a - a) * (h[j] * h[j]) / 6., (b * b * b - b) * (h[j] * h[j]) / 6.
    v = a * y[:, j] + b * y[:, j + 1] + (wz * M[:, j] + ww * M[:, j + 1])
    v[:, ~inside] = np.nan
    return v


# ---- stretch cases ---------------------------------------------------------------------------------------------------------------------------------

def stretch_knots(nm, nl, nr, gaps=(2.5, 3.5)):
    u = U0 + H * np.arange(nm)
    left = u[0] - np.cumsum(gaps[0] * H * 1.3**np.arange(nl))[::-1]
    right = u[-1] + np.cumsum(gaps[1] * H * 1.3**np.arange(nr))
    return left, u, right


def interior_queries(nm, nl, nr, ni, S, seed, gaps=(2.5, 3.5)):
    """ni ascending queries inside the interval in front of the stretch (six or more, where there is one), the stretch and the interval behind it: the
    end knots of the stretch, knots at multiples of S with ``nextafter`` on either side, random points."""
    left, u, right = stretch_knots(nm, nl, nr, gaps)
    rng = np.random.default_rng(seed)
    q = [u[0], u[-1], np.nextafter(u[0], np.inf), np.nextafter(u[-1], -np.inf)]
    if nl:
        q += list(left[-1] + rng.uniform(0.02, 0.98, 7) * (u[0] - left[-1])) + [np.nextafter(u[0], -np.inf)]
    if nr:
        q += list(u[-1] + rng.uniform(0.02, 0.98, 7) * (right[0] - u[-1])) + [np.nextafter(u[-1], np.inf)]
    edges = [k for k in (1, S - 1, S, S + 1, 2 * S, 36, 37, 40, 41, (nm - 1) // S * S - 1, (nm - 1) // S * S, nm - 41, nm - 40, nm - 2) if 0 < k < nm - 1]
    for k in sorted(set(edges))[:(ni - len(q)) // 3]:
        q += [u[k], np.nextafter(u[k], -np.inf), np.nextafter(u[k], np.inf)]
    q = np.array(q)
    assert q.size <= ni, (q.size, ni)
    k = rng.integers(0, nm - 1, ni - q.size)
    q = np.unique(np.concatenate([q, u[k] + rng.uniform(0.01, 0.99, k.size) * H]))
    assert q.size == ni
    return q


def smooth(x, nm):
    """Positive and smooth on every scale of the knots: 1 + a bump as wide as a third of the stretch, centred on it."""
    centre, width = U0 + 0.5 * H * (nm - 1), H * nm / 3.
    return 1. + 0.5 / (1. + ((x - centre) / width)**2)


def pick_S(nm):
    return next((S for S in range(33, 58, 4) if 64 * S >= nm), 0)


@functools.lru_cache(maxsize=None)
def stretch_inputs(name):
    """dict: knots, pieces, queries (= the grid of array 0), base rows of both arrays (7, n0) / (7, n1), tophat, blocks, plan of scheme 0, tables of scheme 1."""
    nm, nl, nr, ni = {**STRETCH, **ELIMINATION_ONLY}[name]
    gaps = GAPS.get(name, (2.5, 3.5))
    left, u, right = stretch_knots(nm, nl, nr, gaps)
    seed = 7 * nm + 1000 * nl + nr + ni
    xq = np.concatenate([left, interior_queries(nm, nl, nr, ni, pick_S(nm) or 57, seed, gaps), right])
    knots = np.concatenate([left, u, right])
    assert (np.diff(knots) > 0).all() and (np.diff(xq) > 0).all()
    pieces = [(0, 0, nl), (1, SPARE[0], nm), (0, nl + ni, nr)]
    rng = np.random.default_rng(seed + 1)
    n0, n1 = xq.size, nm + sum(SPARE)
    grid1 = U0 + H * (np.arange(n1) - SPARE[0])
    eps = np.array(EPS)[:, None]
    rows0 = smooth(xq, nm) * (1. + eps * rng.uniform(-1., 1., (st.NBASE, n0)))
    rows1 = smooth(grid1, nm) * (1. + eps * rng.uniform(-1., 1., (st.NBASE, n1)))
    tophat = rng.uniform(0., 1., n0)
    tophat[::3], tophat[1::3] = 0., 1.
    interior = np.arange(nl, nl + ni)
    blocks = {'front': interior[xq[interior] < u[0]], 'stretch': interior[(xq[interior] >= u[0]) & (xq[interior] <= u[-1])], 'behind': interior[xq[interior] > u[-1]]}
    blocks = {key: index for key, index in blocks.items() if index.size}
    return dict(name=name, nm=nm, nl=nl, nr=nr, ni=ni, gaps=gaps, knots=knots, pieces=pieces, xq=xq, rows0=rows0, rows1=rows1, tophat=tophat, blocks=blocks, interior=interior,
                plan=elimination_plan(knots), tables=uniform_tables(knots, pieces, xq))


def gather(case, rows0, rows1):
    return np.concatenate([(rows1 if src else rows0)[..., start:start + count] for src, start, count in case['pieces']], axis=-1)


def damp(p, v, t):
    return p / ((p / v - 1) * t + 1)


def restate(case, scheme, mistake=None):
    """The float64 restatement of a scheme at all queries (7, nq), without tophat."""
    if scheme == 1:
        return np.array([uniform_run(case['tables'], (r0, r1), mistake=mistake) for r0, r1 in zip(case['rows0'], case['rows1'])])
    return eliminate(case['knots'], gather(case, case['rows0'], case['rows1']), case['plan'], case['xq'], mistake=mistake)


@functools.lru_cache(maxsize=None)
def stretch_case(name):
    """The inputs and, per scheme that fits, truth and the float64 result the level comes from: case['spline'] / case['damped'] -> (truth, {scheme: f8})."""
    case = dict(stretch_inputs(name))
    y = gather(case, case['rows0'], case['rows1'])
    truth = st.spline(case['knots'], y, case['xq'], 'clamped')
    plain = st.spline(case['knots'], y, case['xq'], 'clamped', dtype='f8')
    p_ld, t_ld = case['rows0'].astype(LD), case['tophat'].astype(LD)
    interior = case['interior']
    assert (truth[:, interior] > 0).all()
    case['truth'] = {'spline': truth, 'damped': damp(p_ld, truth, t_ld)}
    case['plain'] = {'spline': plain, 'damped': damp(case['rows0'], plain, case['tophat'])}
    case['scheme'] = {}
    for scheme in ([0, 1] if case['tables'] is not None else [0]):
        v = restate(case, scheme)
        case['scheme'][scheme] = {'spline': v, 'damped': damp(case['rows0'], v, case['tophat'])}
    return case


def block_levels(case, scheme, what):
    """{block: (columns, top (7,), level (7,))}: per block and base row the larger of the two float64 distances from the truth, floored."""
    truth = case['truth'][what]
    out = {}
    for key, columns in case['blocks'].items():
        levels = [st.levels(truth[:, columns], f[:, columns]) for f in (case['plain'][what], case['scheme'][scheme][what])]
        out[key] = (columns, levels[0][0], np.maximum(levels[0][1], levels[1][1]))
    return out


def fraction_used(case, scheme, what, result):
    """{block: (7,)}: the fraction of the device's allowance that a float64 result (7, nq) uses."""
    truth = case['truth'][what]
    return {key: np.asarray(np.abs(result[:, columns].astype(LD) - truth[:, columns]).max(axis=-1) / (st.ALLOW * level * top), dtype='f8')
            for key, (columns, top, level) in block_levels(case, scheme, what).items()}


def assert_blocks(dev, case, scheme, what, label, scaled=True):
    """A device result (nrows, nq), row i = base row i % 7 (times 2**e_i), within ALLOW levels of the truth in every block; the outside knots' own queries
    bit for bit.  Prints and returns the largest fraction of the allowance used."""
    dev = np.asarray(dev)
    got = st.unscale(dev) if scaled else dev.astype(LD)
    index = np.arange(len(dev)) % st.NBASE
    truth = case['truth'][what][index]
    worst, top_level = 0., 0.
    for key, (columns, top, level) in block_levels(case, scheme, what).items():
        assert np.isfinite(got[:, columns].astype('f8')).all(), (label, key)
        dist = np.abs(got[:, columns] - truth[:, columns]).max(axis=-1)
        fraction = np.asarray(dist / (st.ALLOW * level[index] * top[index]), dtype='f8')
        worst, top_level = max(worst, float(fraction.max())), max(top_level, float(level.max() / st.FLOOR))
        assert fraction.max() <= 1., '{}: block {} of row {} at {:.3g} of its allowance'.format(label, key, int(np.argmax(fraction)), fraction.max())
    outside = np.setdiff1d(np.arange(case['xq'].size), case['interior'])
    assert np.array_equal(got[:, outside].astype('f8'), case['rows0'][index][:, outside]), label      # a knot of its own column: that value
    print('%s: largest fraction of the allowance %.3g (level at most %.3g FLOOR)' % (label, worst, top_level))
    return worst


# ---- irregular cases ---------------------------------------------------------------------------------------------------------------------------------

def irregular_queries(x, S, seed):
    """Both end knots, every knot at a multiple of S with its two neighbours, ``nextafter`` either side of a few knots, the midpoints of the first and
    last two intervals, random points; two queries outside the knots and one NaN (positions 0, 1 and 2 of the result)."""
    n = x.size
    rng = np.random.default_rng(seed)
    q = [x[0], x[-1]]
    for k in range(0, n, S * max(1, n // (40 * S))):
        q += [x[j] for j in (k - 1, k, k + 1) if 0 <= j < n]
    for k in sorted(set(j for j in (1, S, 2 * S, n // 3, n // 2, n - 1 - S, n - 2) if 0 < j < n - 1)):
        q += [np.nextafter(x[k], -np.inf), np.nextafter(x[k], np.inf)]
    for k in sorted(set(j for j in (0, 1, n - 3, n - 2) if 0 <= j < n - 1)):
        q.append(0.5 * (x[k] + x[k + 1]))
    k = rng.integers(0, n - 1, 120)
    q = np.concatenate([q, x[k] + rng.uniform(0., 1., 120) * (x[k + 1] - x[k])])
    q = np.clip(q, x[0], x[-1])
    return np.concatenate([[x[0] - 0.5 * (x[1] - x[0]), np.nan, x[-1] + 1.], q])


@functools.lru_cache(maxsize=None)
def largest_irregular(name):
    """The largest n of the family that ``cp_splice_plan_create`` takes: the LDS of the plan grows with n (a table slot per knot outside a uniform
    stretch, 64 doubles per buffer and step of S), so by bisection; 64 x 60 knots, the kernel's own bound, where the LDS never fills (one slot for
    nearly all knots: uniform, and geom1.05, whose spacings stay equal from knot 600 on)."""
    lo, hi = 2200, 64 * 60 + 1      # fits, does not
    assert elimination_plan(stc.knots(name, lo)) is not None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if elimination_plan(stc.knots(name, mid)) is not None:
            lo = mid
        else:
            hi = mid
    return lo


@functools.lru_cache(maxsize=None)
def irregular_case(name, n, pieces=None):
    """One array, one piece (or PIECES[pieces]: the knots' values spread over two arrays): x, y (7, n), queries, plan, truth, the float64 result of the level."""
    x = stc.knots(name, n)
    y = st.base_rows(name, n)
    plan = elimination_plan(x)
    xq = irregular_queries(x, plan['S'], 31 * n + IRREGULAR_FAMILIES.index(name))
    truth = st.spline(x, y, xq, 'clamped')
    plain = st.spline(x, y, xq, 'clamped', dtype='f8')
    scheme = eliminate(x, y, plan, xq)
    assert np.isnan(truth[:, :3].astype('f8')).all() and np.isfinite(truth[:, 3:].astype('f8')).all()
    dist = [np.nanmax(np.abs(f.astype(LD) - truth), axis=-1) for f in (plain, scheme)]
    case = dict(name=name, n=n, x=x, y=y, xq=xq, plan=plan, truth=truth, plain=plain, scheme=scheme, f8=np.where((dist[1] > dist[0])[:, None], scheme, plain))
    if pieces is not None:
        case['pieces'] = PIECES[pieces]
        assert sum(p[2] for p in case['pieces']) == n
        width = [max([p[1] + p[2] for p in case['pieces'] if p[0] == src] + [1]) + 2 for src in (0, 1)]
        rows = [np.random.default_rng(n + src).uniform(0.5, 1.5, (st.NBASE, width[src])) for src in (0, 1)]
        first = 0
        for src, start, count in case['pieces']:
            rows[src][:, start:start + count] = y[:, first:first + count]
            first += count
        case['rows'] = rows
    else:
        case['pieces'], case['rows'] = [(0, 0, n)], [y, None]
    return case


# ---- wallish2018's own grids -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def production_case():
    """The grids of test_spliced_clamped_spline: 3 051 of 3 666 knots on np.linspace(1e-7, 2, 4096), intervals of 19 h in front of and about 1000 h behind
    the stretch.  Levels from the restatements, no cap."""
    k = np.geomspace(1e-7, 1e2, 1024)
    klin = np.linspace(1e-7, 2., 4096)
    mask, left, right = (klin > 1e-2) & (klin < 1.5), k < 5e-4, k > 2.
    knots = np.concatenate([k[left], klin[mask], k[right]])
    pieces = [(0, 0, int(left.sum())), (1, int(np.flatnonzero(mask)[0]), int(mask.sum())), (0, int(np.flatnonzero(right)[0]), int(right.sum()))]
    rng = np.random.default_rng(2)
    shape = lambda x: x / (1. + (x / 0.02)**2.6)      # noqa: E731
    eps = np.array(EPS)[:, None]
    rows0 = shape(k) * (1. + 0.05 * np.sin(k / 0.01) * np.exp(-(k / 0.3)**2)) * rng.uniform(0.5, 2., (st.NBASE, 1))
    rows1 = shape(klin) * (1. + eps * rng.uniform(-1., 1., (st.NBASE, klin.size))) * (rows0[:, :1] / shape(k)[0])
    tophat = np.ones_like(k)
    tophat[k > 1.] *= np.exp(-20.**2 * (k[k > 1.] - 1.)**2)
    u = klin[mask]
    interior = np.flatnonzero(~left & ~right)
    blocks = {'front': interior[k[interior] < u[0]], 'stretch': interior[(k[interior] >= u[0]) & (k[interior] <= u[-1])], 'behind': interior[k[interior] > u[-1]]}
    case = dict(name='wallish2018', nm=u.size, nl=int(left.sum()), nr=int(right.sum()), knots=knots, pieces=pieces, xq=k, rows0=rows0, rows1=rows1, tophat=tophat,
                blocks=blocks, interior=interior, plan=elimination_plan(knots), tables=uniform_tables(knots, pieces, k))
    y = gather(case, rows0, rows1)
    truth = st.spline(knots, y, k, 'clamped')
    plain = st.spline(knots, y, k, 'clamped', dtype='f8')
    case['truth'] = {'spline': truth, 'damped': damp(rows0.astype(LD), truth, tophat.astype(LD))}
    case['plain'] = {'spline': plain, 'damped': damp(rows0, plain, tophat)}
    case['scheme'] = {}
    for scheme in (0, 1):
        v = restate(case, scheme)
        case['scheme'][scheme] = {'spline': v, 'damped': damp(rows0, v, tophat)}
    return case
