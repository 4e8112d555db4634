"""
Truth, launch plan and cases of the point-interpolation kernels of csrc/cp_interp.hip -- ``interp_linear_kernel``, ``flag_outside_kernel``,
``interp_table_kernel<1 | 2, double | float>``, ``spline_points_kernel`` / ``spline_points_lds_kernel`` and ``spline_rows_at_queries_kernel`` -- shared by
tests/test_interp_truth_host.py (the plan and the cap of every case, the emulated four-in-flight loop, the mutations the cases catch) and
tests/test_interp_truth_gpu.py (the kernels through the C ABI).  numpy only.

The launch plan restated: what the entry points compute from their sizes, with the constants of cp_interp.hip named once (``linear_plan``, ``table_plan``,
``flag_plan``, ``points_plan``, ``rows_plan``).  A trip is one pass of a kernel's grid-stride loop; a thread of ``interp_table_kernel`` holds U = 4 samples
in the slots i + u * stride of one trip.

Truths
  piecewise linear   ``numpy.interp`` itself (the contract is bit identity); float32 samples are widened, interpolated and rounded once; samples outside the
                     table and NaN samples give NaN (``interp``)
  cp_spline_points   ``spline_truth.evaluate`` in longdouble on the float64 (xk, y, s) exactly as the kernel gets them: the kernel is a Hermite evaluator
                     of whatever slopes it is given, and so is the truth (``points_values``)
  cp_spline_rows_at_queries   a y_j + b y_j+1 + ((a^3 - a) M_j + (b^3 - b) M_j+1) h^2 / 6 in longdouble from the float64 (xk, y, M) as given, the interval
                     numpy's searchsorted(side='right') - 1 clipped to [0, n - 2] (the end cubics continued), NaN for a NaN query (``rows_values``).
                     An infinite query gives NaN as well, in the truth as in the kernel: a^3 - a is inf - inf.
Both spline truths with ``dtype='f8'`` are the float64 restatement that sets the tolerance (``spline_truth.levels``, ``assert_within``: 16 levels per
column / row, a case is used only while its level stays under ``spline_truth.CAP``).
"""
import functools

import numpy as np

import spline_tables_cases as stc
import spline_truth as st

LD = np.longdouble

# ---- the constants of cp_interp.hip ------------------------------------------------------------------------------------------------------------------
BLOCK = 256
LINEAR_GRID = 256 * 8        # cp_interp_linear, spline_points_kernel
TABLE_GRID = 256 * 16        # interp_table_kernel
TABLE_U = 4                  # samples of a thread in flight
FLAG_GRID = 1024             # flag_outside_kernel
LDS_GRID = 256 * 4           # spline_points_lds_kernel
LDS_KNOTS = 2048             # SPLINE_LDS_KNOTS
LDS_MIN_NQ = 65536
ROWS_GRID = 256 * 16         # spline_rows_at_queries_kernel
COARSE_STRIDE = 32
COARSE_MAX = 4096            # coarse knots in LDS (32 KB)


def _ceil(a, b):
    return -(-a // b)


def coarse(n, fixed_stride=False):
    """(stride, ncoarse) of the coarse knots in LDS."""
    stride = COARSE_STRIDE
    while not fixed_stride and _ceil(n, stride) > COARSE_MAX:
        stride *= 2
    return stride, _ceil(n, stride)


def last_block_knots(n):
    """How many knots the last coarse block holds (the fine bisection's ``hi`` is clipped at n - 1 when this is not stride + 1 ... )."""
    stride, ncoarse = coarse(n)
    return n - (ncoarse - 1) * stride


def _grid(count, most):
    return min(_ceil(count, BLOCK), most)


def linear_plan(n, nx):
    stride, ncoarse = coarse(n)
    grid = _grid(nx, LINEAR_GRID)
    return dict(stride=stride, ncoarse=ncoarse, grid=grid, trips=_ceil(nx, grid * BLOCK), lds=ncoarse * 8)


def table_plan(nx):
    """grid, stride (threads of the grid), trips of a thread's loop (each U * stride samples) and the number of live samples per slot u."""
    grid = _grid(nx, TABLE_GRID)
    stride = grid * BLOCK
    chunk = np.arange(_ceil(nx, stride))      # chunk c holds the samples c * stride ... and is slot c % U of trip c // U
    size = np.minimum(stride, nx - chunk * stride)
    live = [int(size[chunk % TABLE_U == u].sum()) for u in range(TABLE_U)]
    return dict(grid=grid, stride=stride, trips=_ceil(nx, TABLE_U * stride), live=live)


def flag_plan(nx):
    return dict(grid=FLAG_GRID, trips=_ceil(nx, FLAG_GRID * BLOCK))


def points_plan(n, ncol, nq):
    if ncol == 1 and n <= LDS_KNOTS and nq >= LDS_MIN_NQ:
        grid = _grid(nq, LDS_GRID)
        return dict(kernel='spline_points_lds_kernel', stride=None, ncoarse=None, grid=grid, trips=_ceil(nq, grid * BLOCK), lds=(n + 4 * (n - 1)) * 8)
    stride, ncoarse = coarse(n)
    grid = _grid(nq, LINEAR_GRID)
    return dict(kernel='spline_points_kernel', stride=stride, ncoarse=ncoarse, grid=grid, trips=_ceil(nq, grid * BLOCK), lds=ncoarse * 8)


def rows_plan(nrows, nq):
    grid = _grid(nrows * nq, ROWS_GRID)
    return dict(grid=grid, trips=_ceil(nrows * nq, grid * BLOCK))


def slot_of(j, nx):
    """(trip, slot u) in which interp_table_kernel handles sample j of nx."""
    stride = table_plan(nx)['stride']
    return (j // stride) // TABLE_U, (j // stride) % TABLE_U


# ---- piecewise linear: tables, samples, truth ----------------------------------------------------------------------------------------------------------
def interp(q, x, f):
    """numpy.interp, NaN outside the table and for NaN; float32 samples widened, the result rounded once."""
    q = np.asarray(q)
    q64 = q.astype('f8')
    with np.errstate(invalid='ignore'):
        r = np.interp(q64, x, f)
    r[~((q64 >= x[0]) & (q64 <= x[-1]))] = np.nan
    return r.astype(q.dtype)


def is_outside(q, x):
    q64 = np.asarray(q).astype('f8')
    return ~((q64 >= x[0]) & (q64 <= x[-1]))


def values(x):
    """The table values of tests/test_interp_table_host.py: of both signs, growing."""
    return np.cos(3. * np.arange(x.size)) * np.sqrt(1. + np.arange(x.size))


# name: (knots, law, first knot of the law): those that tests/test_interp_table_host.py has as well are the same there
TABLES = {'uniform': (lambda: np.linspace(-2., 5., 3001), 1, 0),      # law 1
          'desi': (lambda: np.concatenate([[0.], np.logspace(-8, 2, 40001)]), 2, 1),      # law 2 behind one leading knot: the reference's data/desi.dat
          'geometric': (lambda: np.geomspace(3e-4, 7e5, 777), 2, 0),      # law 2 from the first knot on
          'three rows': (lambda: np.array([1., 2., 3.]), 1, 0),      # the smallest table with a law: the walk's clamp n - 2 is 1
          'three leading knots': (lambda: np.concatenate([[-1., 0., 1e-12], np.geomspace(1e-6, 10., 500)]), 2, 3),      # bisection among the leading knots
          'off by a fifth of a step': (lambda: np.linspace(0., 1., 200) + np.r_[0., 0.2 / 199 * np.sin(np.arange(1, 199)), 0.], 1, 0),      # law 1 at the edge of acceptance: the walk steps
          'huge range': (lambda: np.geomspace(1e-300, 1e300, 1201), 2, 0),      # the exponent part of log2_guess over all of its range
          'nine leading knots': (lambda: np.concatenate([-np.arange(9., 0., -1.), np.geomspace(1e-6, 10., 500)]), 0, 0),      # one leading knot too many: bisection
          'repeated knots': (lambda: np.repeat(np.linspace(0., 1., 50), 2), 0, 0),
          'irregular': (lambda: np.sort(np.random.default_rng(11).uniform(0., 10., 5000)), 0, 0),
          'two rows': (lambda: np.array([1., 2.]), 0, 0),
          'one row': (lambda: np.array([3.]), 0, 0),
          'subnormal knots': (lambda: np.geomspace(1e-320, 1e-310, 400), 2, 0)}      # frexp of a subnormal: the exponent below -1022
LARGE_TABLES = ['uniform', 'desi']
SMALL_TABLES = [name for name in TABLES if name not in LARGE_TABLES]
SMALL_NX = 20000


@functools.lru_cache(maxsize=None)
def table(name):
    """(x, f) of a table; the subnormal table has subnormal values as well (a finite slope)."""
    x = TABLES[name][0]()
    f = x * (1.5 + np.cos(3. * np.arange(x.size))) if name == 'subnormal knots' else values(x)
    return x, f


def infinite_values(f):
    """+inf at one knot, -inf at two neighbours, equal infinities at two neighbours: numpy's retry from the right knot and its common-value rule."""
    f = f.copy()
    n = f.size
    f[n // 5], f[2 * n // 5:2 * n // 5 + 2], f[3 * n // 5:3 * n // 5 + 2] = np.inf, -np.inf, np.inf
    return f


def pool(x, size, seed=0):
    """``size`` samples inside the table in a fixed random order, so that every prefix is a mix: every knot, one ulp either side of every knot, the two ends,
    and for the rest uniform and (from the first positive knot on) log-uniform samples.
    Samples 1 ... 6 are the ends, their neighbours and the last interval."""
    rng = np.random.default_rng(1000 + seed)
    parts = [x, np.nextafter(x[1:], -np.inf), np.nextafter(x[:-1], np.inf), x[[0, -1]]]
    rest = max(size - sum(p.size for p in parts), 16)
    positive = x[x > 0.]
    if positive.size >= 2 and x[-1] > x[0]:
        parts.append(np.exp(rng.uniform(np.log(positive[0]), np.log(x[-1]), rest // 2)))
        rest -= rest // 2
    parts.append(rng.uniform(0., 1., rest) * (x[-1] - x[0]) + x[0] if np.isfinite(x[-1] - x[0]) else rng.uniform(x[0], x[-1], rest))
    q = np.clip(np.concatenate(parts), x[0], x[-1])
    q = np.ascontiguousarray(q[rng.permutation(q.size)][:size])
    if size >= 8 and x.size >= 2:      # in every call of eight samples or more: the ends and the last interval (the last coarse block of the bisection)
        q[1:7] = x[0], x[-1], np.nextafter(x[-1], -np.inf), x[-2], 0.5 * (x[-2] + x[-1]), np.nextafter(x[0], np.inf)
    return q


# nx of cp_interp_table_apply with a law, and the edge each is there for (stride = grid * 256, a trip is 4 strides)
TABLE_NX = {1: 'one thread of one block',
            255: 'one block, its last thread idle',
            256: 'one block, full',
            257: 'a second block of one thread',
            1048575: 'the full grid of 4096 blocks, the last thread idle: the largest nx with slot 0 alone',
            1048576: 'the full grid, every thread one sample in slot 0',
            1048577: 'exactly one live sample in slot 1, none in slots 2 and 3',
            2 * 1048576 + 1: 'slot 1 full, one live sample in slot 2',
            4194303: 'all four slots, the last thread of the last block idle in slot 3',
            4194304: 'one trip exactly full',
            4194305: 'a second trip of one sample',
            5242880 + 257: 'a second trip with slot 0 full and 257 live samples in slot 1'}
POOL_SIZE = max(TABLE_NX)

# (n, nx) of the bisection kernel: coarse strides 32 / 64 / 128 / 256, the last coarse block clipped to one and two knots; trips of 524 288 samples
BISECT_N = {1: 'one row: every sample is the last knot', 2: 'one interval', 33: 'two coarse knots, the second alone in its block',
            131072: 'stride 32 with all 4096 coarse knots', 131073: 'stride 64, the last block the last knot alone', 262145: 'stride 128, the last block one knot',
            262146: 'stride 128, the last block clipped to two knots', 524289: 'stride 256, the last block one knot'}
BISECT_NX = {1: 'one thread', 524287: 'one trip, the last thread idle', 524288: 'one trip exactly', 524289: 'a second trip of one sample',
             1048576 + 3: 'a third trip of three samples'}
BISECT_LARGEST_AT = (33, 262146)      # the n that get the largest nx


def bisect_cases():
    return [(n, nx) for n in BISECT_N for nx in BISECT_NX if nx != max(BISECT_NX) or n in BISECT_LARGEST_AT]


@functools.lru_cache(maxsize=None)
def bisect_table(n):
    """n irregular knots (jittered spacings, so that no law fits) and their values."""
    rng = np.random.default_rng(7 * n)
    x = np.concatenate([[0.], np.cumsum(rng.uniform(0.2, 1.8, n - 1))]) if n > 1 else np.array([3.])
    return x, values(x)


# where the flag test puts its one bad sample: (label, nx, index)
def flag_places():
    s = TABLE_GRID * BLOCK
    nx = 7 * s + 4099      # the second trip reaches into slot 3
    places = [('first', nx, 0), ('last', nx, nx - 1)]
    places += [('trip %d slot %d' % (t, u), nx, (TABLE_U * t + u) * s + 1000 * u + 13) for t in (0, 1) for u in range(TABLE_U)]
    places += [('the last thread of the last block, slot %d' % u, nx, (u + 1) * s - 1) for u in (0, 3)]
    places.append(('the last thread of the last block of a partial grid', 70001, 70000))
    return places


FLAG_IRREGULAR_NX = FLAG_GRID * BLOCK + 1000      # flag_outside_kernel: a second trip
FLAG_IRREGULAR_AT = [0, FLAG_GRID * BLOCK - 1, FLAG_GRID * BLOCK, FLAG_GRID * BLOCK + 999]


# ---- cp_spline_points ----------------------------------------------------------------------------------------------------------------------------------
POINT_FAMILIES = ['uniform', 'geom1.05', 'jitter100', 'sigma_r', 'logk_pad']
POINT_SIZES = [119, 2048, 2049]      # the distance tables; the LDS kernel's largest spline; one knot more
POINT_NCOL = [1, 2, 3, 64]
POINT_NQ = {1: 'one thread', 257: 'a second block', 65535: 'the last nq of the general kernel at ncol = 1', 65536: 'the first nq of the LDS kernel',
            262144: 'one trip of the LDS kernel exactly', 262145: 'a second trip of the LDS kernel', 524288: 'one trip of the general kernel exactly',
            524289: 'a second trip of the general kernel'}
POINT_COUNT_CASES = [('jitter100', 2048), ('uniform', 2049), ('sigma_r', 119)]      # the (family, n) that run through every nq
POINT_BASE = 8209      # distinct queries of a case; query i of a call is base query i % 8209
# cases over the cap, with their level in FLOORs as tests/test_interp_truth_host.py measures it: (family, n, nu, extrapolate) -- filled from the measurement
POINTS_OVER_CAP = {}


def points_used(name, n, nu, extrapolate):
    return not any(all(k in ('*', v) for k, v in zip(key, (name, n, nu, extrapolate))) for key in POINTS_OVER_CAP)


@functools.lru_cache(maxsize=None)
def points_case(name, n):
    """x, y (7, n) and the float64 slopes s (7, n) of the natural splines (the longdouble solve, rounded: what a caller hands the kernel)."""
    x, y = st.knots(name, n), st.base_rows(name, n)
    return dict(x=x, y=y, s=st.slopes(x, y, 'natural', LD).astype('f8'))


@functools.lru_cache(maxsize=None)
def tiny_case(n):
    """n = 2, 3 with independent slopes (collinear values with their own slope make the cubic degenerate and its second derivative all rounding)."""
    x = np.array([1., 3.5, 4.25][:n])
    y = np.array([[0.7, -1.1, 0.4], [2., 2.5, 1.75]])[:, :n]
    s = np.array([[1.3, 0.2, -0.9], [-0.6, 0.8, 1.1]])[:, :n]
    return dict(x=x, y=y, s=s)


@functools.lru_cache(maxsize=None)
def stride64_case():
    """131 073 uniform knots (coarse stride 64) a unit apart, the samples and slopes those of 2 + sin x: a Hermite cubic per interval like any other (with
    knots 3e-4 apart the second derivative is all cancellation: 27 783 FLOOR in the float64 restatement)."""
    x = np.linspace(0., 131072., 131073)
    return dict(x=x, y=(2. + np.sin(x))[None, :], s=np.cos(x)[None, :])


def points_base(x, extrapolate, seed=0, size=POINT_BASE):
    """The distinct queries of a case: every knot, one ulp below every knot, the midpoints (thinned to fit), random points inside; ``extrapolate``: up to one
    end interval beyond either end; otherwise one ulp outside either end (NaN there)."""
    rng = np.random.default_rng(31 + seed)
    fixed = [x, np.nextafter(x[1:], -np.inf), 0.5 * (x[1:] + x[:-1])]
    step = _ceil(sum(p.size for p in fixed), size - 64)
    fixed = np.concatenate([x[[0, -1]], np.concatenate(fixed)[::step]]) if step > 1 else np.concatenate(fixed)
    h0, h1 = x[1] - x[0], x[-1] - x[-2]
    if extrapolate:
        beyond = np.concatenate([x[0] - np.array([1., 0.5, 0.25, 1e-3]) * h0, x[-1] + np.array([1e-3, 0.25, 0.5, 1.]) * h1, x[0] - rng.uniform(0., 1., 12) * h0,
                                 x[-1] + rng.uniform(0., 1., 12) * h1])
    else:
        beyond = np.array([np.nextafter(x[0], -np.inf), np.nextafter(x[-1], np.inf)])
    k = rng.integers(0, x.size - 1, size - fixed.size - beyond.size)
    inside = np.clip(x[k] + rng.uniform(0., 1., k.size) * (x[k + 1] - x[k]), x[0], x[-1])
    q = np.concatenate([fixed, beyond, inside])
    assert q.size == size
    return q[rng.permutation(size)]


def points_index(nq, size=POINT_BASE):
    """(index into the base queries, positions that hold NaN instead) of a call with nq queries: NaN first, last and inside from 257 queries on."""
    nan = np.array([0, nq // 2, nq - 1]) if nq >= 257 else np.array([], dtype='i8')
    return np.arange(nq) % size, nan


def points_queries(base, nq):
    index, nan = points_index(nq, base.size)
    q = base[index]
    q[nan] = np.nan
    return q


def points_values(case, base, nu, extrapolate, rows=slice(None)):
    """(truth, float64 restatement) at the base queries, (rows, size)."""
    return tuple(st.evaluate(case['x'], case['y'][rows], case['s'][rows].astype(dtype), base, bool(extrapolate), nu) for dtype in (LD, 'f8'))


def points_expand(v, nq):
    """The values at the base queries taken to the nq queries of a call."""
    index, nan = points_index(nq, v.shape[-1])
    v = v[..., index]
    v[..., nan] = np.nan
    return v


# ---- cp_spline_rows_at_queries ---------------------------------------------------------------------------------------------------------------------------
ROWS_SHAPES = {(1, 2, 1): 'one thread, one interval', (7, 300, 41): "the batched filter's shape", (64, 300, 65): 'whole rows do not end with a block',
               (257, 300, 4081): '1 048 817 elements: a second trip of 241', (1025, 119, 1024): '1 049 600 elements: a second trip of four blocks'}
ROWS_KNOTS = ['log10', 'jitter100']      # the BAO filter's knots (uniform to rounding: the first guess is right); uneven knots: the walk takes steps both ways
ROWS_OVER_CAP = {}


def rows_knots(name, n):
    return np.log10(np.geomspace(1e-5, 1e2, n)) if name == 'log10' else stc.knots('jitter100', n)


@functools.lru_cache(maxsize=None)
def rows_case(name, shape):
    """x (n,), y, m (nrows, n) and xq (nrows, nq): smooth noisy rows with the float64 second derivatives of their natural splines; per row queries inside, on
    the knots (every third element in turn), up to one end interval beyond either end; from 20 elements on +inf, -inf and NaN (first row) and a NaN in the
    last element."""
    nrows, n, nq = shape
    x = rows_knots(name, n)
    rng = np.random.default_rng(97 * n + nrows + (name == 'log10'))
    u = (x - x[0]) / (x[-1] - x[0])
    y = rng.uniform(0.5, 1.5, (nrows, n)) * (1. + 40. * u)**-1.5
    if n >= 3:
        m = st.knot_second_derivatives(x, y, 'natural', LD).astype('f8')
    else:
        m = np.array([[0.3, -0.2]]) * y / (x[1] - x[0])**2
    h0, h1 = x[1] - x[0], x[-1] - x[-2]
    k = rng.integers(0, n - 1, (nrows, nq))
    xq = np.clip(x[k] + rng.uniform(0., 1., k.shape) * (x[k + 1] - x[k]), x[0], x[-1])
    flat = xq.reshape(-1)
    at = np.arange(0, flat.size, 3)
    flat[at] = x[(at // 3) % n]
    if flat.size >= 20:
        at = np.arange(7, flat.size, 11)
        flat[at] = np.where(at % 2, x[0] - rng.uniform(0., 1., at.size) * h0, x[-1] + rng.uniform(0., 1., at.size) * h1)
        flat[[1, 2, 4, flat.size - 1]] = np.inf, -np.inf, np.nan, np.nan
        flat[[5, 8]] = x[0] - h0, x[-1] + h1
    return dict(x=x, y=y, m=m, xq=xq)


def rows_values(x, y, m, xq, dtype=LD):
    """(nrows, nq): the four-term formula in ``dtype`` at the queries xq (nrows, nq) of the rows."""
    xq = np.asarray(xq, dtype='f8')
    n = x.size
    j = np.clip(np.searchsorted(x, xq.reshape(-1), side='right').reshape(xq.shape) - 1, 0, n - 2)
    j = np.where(xq != xq, 0, j)
    xx, q = x.astype(dtype), xq.astype(dtype)
    yy, mm = np.asarray(y).astype(dtype), np.asarray(m).astype(dtype)
    h = xx[j + 1] - xx[j]
    with np.errstate(invalid='ignore'):
        a, b = (xx[j + 1] - q) / h, (q - xx[j]) / h
        take = lambda t, k: np.take_along_axis(t, k, axis=1)      # noqa: E731
        v = a * take(yy, j) + b * take(yy, j + 1) + ((a * a * a - a) * take(mm, j) + (b * b * b - b) * take(mm, j + 1)) * (h * h) / 6
    v[xq != xq] = np.nan
    return v


def worst_level(truth, f64):
    """The largest level of a case in FLOORs."""
    return float(st.levels(truth, f64)[1].max() / st.FLOOR)
