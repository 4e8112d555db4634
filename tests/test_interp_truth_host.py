"""CPU: what tests/test_interp_truth_gpu.py rests on (tests/interp_truth.py).

  * the four-in-flight loop of ``interp_table_kernel`` with ``cpit::interp_samples<LAW, 4>`` under it, compiled with g++ (tests/host_emu/emu_interp.cpp) and run
    for a grid of T = 8 threads: the bits of ``numpy.interp`` for double and float samples on every table with a law, with infinite values in the table and
    with subnormal knots, at every nx where a slot or a trip begins or ends; the flag raised if and only if a sample is outside, with the one outside sample
    in every position, so in every (trip, slot) class;
  * the restated launch plan of every device case hits the edge the case is listed for;
  * the float64 restatement of every spline case used on the device stays under ``spline_truth.CAP`` (cases over it are listed with their level in
    ``interp_truth.POINTS_OVER_CAP`` / ``ROWS_OVER_CAP`` and are not used);
  * nine mutations of the emulated loop, of the restated search and of the float64 restatement are each caught by at least one listed case; the four of the
    loop run on an index model of it (7 M samples per device case), which at T = 8 is held to the emulated C++ loop on real samples, mutated and not.
"""
import ctypes
import functools

import numpy as np
import pytest

import interp_truth as it
import spline_truth as st
import test_interp_table_host as ith
from sigma_device import CANARY

LD = np.longdouble
T = 8
CANARY32 = np.float32(-1.2345679e37)
HOST_NX = [1, T - 1, T, T + 1, 2 * T + 1, 4 * T - 1, 4 * T, 4 * T + 1, 5 * T + 3, 8 * T + 1]


def loop(x, f, law, q):
    """(out with one guard element behind it, flag): the emulated kernel loop into canaries."""
    single = q.dtype == np.float32
    out = np.full(q.size + 1, CANARY32 if single else CANARY, dtype=q.dtype)
    ptr = ctypes.POINTER(ctypes.c_float if single else ctypes.c_double)
    entry = ith._lib().emu_interp_samples_f32 if single else ith._lib().emu_interp_samples
    flag = entry(ctypes.c_longlong(x.size), ith.as_p(x), ith.as_p(f), law[0], ctypes.c_longlong(law[1]), ctypes.c_double(law[2]), ctypes.c_double(law[3]),
                 ctypes.c_longlong(q.size), q.ctypes.data_as(ptr), out.ctypes.data_as(ptr), ctypes.c_longlong(T))
    return out, flag


def test_shared_tables_are_the_host_tests_tables():
    shared = [name for name in it.TABLES if name in ith.TABLES]
    # every table of the host test that has a law is here, and so goes through the four-in-flight loop below
    assert sorted(name for name in ith.TABLES if ith.TABLES[name][1]) == sorted(name for name in shared if it.TABLES[name][1])
    assert set(ith.TABLES) - set(shared) == {'off by a third of a step'}      # (no law: one more irregular table)
    for name in shared:
        assert np.array_equal(it.table(name)[0], ith.TABLES[name][0](np.random.default_rng(11))) and it.TABLES[name][1:] == ith.TABLES[name][1:], name


LOOP_TABLES = [name for name in it.TABLES if it.TABLES[name][1]] + ['uniform, infinite values', 'desi, infinite values']


@pytest.mark.parametrize('name', LOOP_TABLES)
def test_emulated_loop_gives_numpys_bits(name):
    base = name.split(',')[0]
    x, f = it.table(base)
    if name != base:
        f = it.infinite_values(f)
    law = ith.find_law(x)
    assert law[:2] == it.TABLES[base][1:], law
    whole = it.pool(x, 40000, seed=len(name))
    for dtype in ('f8', 'f4'):
        with np.errstate(over='ignore'):
            clean = whole.astype(dtype)
        clean = clean[~it.is_outside(clean, x)]
        if clean.size < 2000:      # (the subnormal knots: no float32 sample lies inside)
            assert dtype == 'f4' and base == 'subnormal knots'
            continue
        with np.errstate(over='ignore'):
            ends = np.array([x[0], x[-1]]).astype(dtype)
        bads = [b for b in (np.nextafter(ends[0], ends.dtype.type(-np.inf)), np.nextafter(ends[1], ends.dtype.type(np.inf)), ends.dtype.type(np.nan)) if it.is_outside(b, x)]
        for k, nx in enumerate(HOST_NX):
            q = np.ascontiguousarray(clean[97 * k:97 * k + nx])
            ref = it.interp(q, x, f)
            out, flag = loop(x, f, law, q)
            assert flag == 0 and out[-1] == out.dtype.type(CANARY32 if dtype == 'f4' else CANARY), (name, dtype, nx)
            assert np.array_equal(out[:-1], ref, equal_nan=True), (name, dtype, nx)
            assert name != base or not np.isnan(ref).any()
            classes = set()
            for j in range(nx):      # the one outside sample in every position: every (trip, slot) class that this nx has
                bad = q.copy()
                bad[j] = bads[j % len(bads)]
                out, flag = loop(x, f, law, bad)
                assert flag == 1 and np.isnan(out[j]), (name, dtype, nx, j)
                keep = np.arange(nx) != j
                assert np.array_equal(out[:-1][keep], ref[keep], equal_nan=True), (name, dtype, nx, j)
                classes.add(((j // T) // 4, (j // T) % 4))
            assert len(classes) == -(-nx // T)


def test_emulated_loop_with_infinite_values_reaches_numpys_retries():
    """The infinite values are met: samples in the intervals next to them give infinities of both signs as numpy does (asserted above) -- through the retry from
    the right knot (behind the +inf knot: -inf x dx + inf is NaN at first) and the common-value rule (between two equal infinities the slope is NaN) -- never NaN."""
    x, f = it.table('uniform')
    ref = it.interp(it.pool(x, 40000, seed=len('uniform, infinite values')), x, it.infinite_values(f))
    assert np.isposinf(ref).sum() > 10 and np.isneginf(ref).sum() > 10 and not np.isnan(ref).any()


# ---- the plans of the device cases -------------------------------------------------------------------------------------------------------------------
def test_table_plans_hit_their_edges():
    s = it.TABLE_GRID * it.BLOCK
    assert s == 1048576
    expect = {1: (1, 1, [1, 0, 0, 0]), 255: (1, 1, [255, 0, 0, 0]), 256: (1, 1, [256, 0, 0, 0]), 257: (2, 1, [257, 0, 0, 0]),
              1048575: (4096, 1, [s - 1, 0, 0, 0]), 1048576: (4096, 1, [s, 0, 0, 0]), 1048577: (4096, 1, [s, 1, 0, 0]), 2 * 1048576 + 1: (4096, 1, [s, s, 1, 0]),
              4194303: (4096, 1, [s, s, s, s - 1]), 4194304: (4096, 1, [s, s, s, s]), 4194305: (4096, 2, [s + 1, s, s, s]), 5242880 + 257: (4096, 2, [2 * s, s + 257, s, s])}
    assert sorted(expect) == sorted(it.TABLE_NX)
    for nx, (grid, trips, live) in expect.items():
        plan = it.table_plan(nx)
        assert (plan['grid'], plan['trips'], plan['live']) == (grid, trips, live) and sum(live) == nx and plan['stride'] == grid * 256, (nx, plan)
    # for every nx <= 1 048 576 the stride is at least nx: slot 0 alone
    assert all(it.table_plan(nx)['stride'] >= nx for nx in (1, 257, 70001, 260000, 1048576))
    seen = {}
    for label, nx, j in it.flag_places():
        assert 0 <= j < nx
        seen[label] = it.slot_of(j, nx)
    assert [seen['trip %d slot %d' % (t, u)] for t in (0, 1) for u in range(4)] == [(t, u) for t in (0, 1) for u in range(4)]
    assert seen['first'] == (0, 0) and seen['last'] == (1, 3)
    nx = it.flag_places()[0][1]
    assert nx <= 7500000 and it.table_plan(nx)['trips'] == 2 and min(it.table_plan(nx)['live']) > s
    for u in (0, 3):
        j = [p[2] for p in it.flag_places() if p[0].endswith('last block, slot %d' % u)][0]
        assert j % s == s - 1 and it.slot_of(j, nx) == (0, u)      # thread 255 of block 4095
    label, nx, j = it.flag_places()[-1]
    assert j == nx - 1 and it.table_plan(nx)['grid'] == -(-nx // 256) < it.TABLE_GRID and nx % 256 != 0
    assert it.flag_plan(it.FLAG_IRREGULAR_NX)['trips'] == 2 and it.flag_plan(262144)['trips'] == 1
    assert [j // (it.FLAG_GRID * it.BLOCK) for j in it.FLAG_IRREGULAR_AT] == [0, 0, 1, 1] and it.FLAG_IRREGULAR_AT[-1] == it.FLAG_IRREGULAR_NX - 1


BISECT_EXPECT = {1: (32, 1, 1), 2: (32, 1, 2), 33: (32, 2, 1), 131072: (32, 4096, 32), 131073: (64, 2049, 1), 262145: (128, 2049, 1), 262146: (128, 2049, 2), 524289: (256, 2049, 1)}


def test_bisection_plans_hit_their_edges():
    assert sorted(BISECT_EXPECT) == sorted(it.BISECT_N)
    for n, (stride, ncoarse, last) in BISECT_EXPECT.items():
        assert it.coarse(n) == (stride, ncoarse) and it.last_block_knots(n) == last and ncoarse <= it.COARSE_MAX, n
        x = it.bisect_table(n)[0]
        assert x.size == n and (n < 3 or ith.find_law(x)[0] == 0), n      # irregular: cp_interp_table takes the bisection
    trips = {nx: it.linear_plan(33, nx)['trips'] for nx in it.BISECT_NX}
    assert trips == {1: 1, 524287: 1, 524288: 1, 524289: 2, 1048579: 3} and it.linear_plan(33, 524288)['grid'] == 2048 == it.LINEAR_GRID
    cases = it.bisect_cases()
    assert len(cases) == 8 * 4 + 2 and sorted(n for n, nx in cases if nx == 1048579) == [33, 262146]


def test_points_plans_hit_their_edges():
    lds, general = 'spline_points_lds_kernel', 'spline_points_kernel'
    assert it.points_plan(2048, 1, 65535)['kernel'] == general and it.points_plan(2048, 1, 65536)['kernel'] == lds
    assert it.points_plan(2049, 1, 65536)['kernel'] == general and it.points_plan(2048, 2, 65536)['kernel'] == general
    assert it.points_plan(2048, 1, 65536)['lds'] == 81888 and it.points_plan(119, 1, 65536)['lds'] == (119 + 4 * 118) * 8
    assert [it.points_plan(2048, 1, nq)['trips'] for nq in (65536, 262144, 262145, 524289)] == [1, 1, 2, 3]
    assert [it.points_plan(2048, 2, nq)['trips'] for nq in (1, 257, 262145, 524288, 524289)] == [1, 1, 1, 1, 2]
    assert [it.points_plan(2048, 2, nq)['grid'] for nq in (1, 257, 524288)] == [1, 2, 2048]
    plan = it.points_plan(131073, 1, 257)
    assert (plan['kernel'], plan['stride'], plan['ncoarse']) == (general, 64, 2049) and it.stride64_case()['x'].size == 131073
    assert set(n for _, n in it.POINT_COUNT_CASES) == set(it.POINT_SIZES)


def test_rows_plans_hit_their_edges():
    expect = {(1, 2, 1): (1, 1), (7, 300, 41): (2, 1), (64, 300, 65): (17, 1), (257, 300, 4081): (4096, 2), (1025, 119, 1024): (4096, 2)}
    assert sorted(expect) == sorted(it.ROWS_SHAPES)
    for (nrows, n, nq), (grid, trips) in expect.items():
        plan = it.rows_plan(nrows, nq)
        assert (plan['grid'], plan['trips']) == (grid, trips)
    assert 257 * 4081 == 1048817 and 1025 * 1024 == 1049600 and (64 * 65) % 256 != 0
    for name in it.ROWS_KNOTS:
        for shape in it.ROWS_SHAPES:
            case = it.rows_case(name, shape)
            x, xq = case['x'], case['xq']
            flat = xq.reshape(-1)
            if flat.size >= 20:
                assert np.isposinf(flat[1]) and np.isneginf(flat[2]) and np.isnan(flat[[4, -1]]).all() and flat[5] == x[0] - (x[1] - x[0]) and flat[8] == x[-1] + (x[-1] - x[-2])
            finite = flat[np.isfinite(flat)]
            assert finite.min() >= x[0] - (x[1] - x[0]) and finite.max() <= x[-1] + (x[-1] - x[-2])      # within one end interval
            if flat.size >= 3 * x.size:
                assert np.isin(x, flat).all()      # every knot is a query
    # uneven knots: the uniform first guess is off by many intervals, in both directions
    x = it.rows_knots('jitter100', 300)
    guess = np.clip(((x[:-1] - x[0]) * (299 / (x[-1] - x[0]))).astype(int), 0, 298)
    assert (guess - np.arange(299)).max() >= 5 and (guess - np.arange(299)).min() <= -5
    x = it.rows_knots('log10', 300)
    guess = np.clip(((0.5 * (x[:-1] + x[1:]) - x[0]) * (299 / (x[-1] - x[0]))).astype(int), 0, 298)
    assert np.array_equal(guess, np.arange(299))


# ---- the cap of every spline case used on the device ------------------------------------------------------------------------------------------------------
def point_levels(case, name, n):
    out = {}
    for extrapolate in (0, 1):
        base = it.points_base(case['x'], extrapolate, seed=n)
        for nu in (0, 1, 2):
            truth, f64 = it.points_values(case, base, nu, extrapolate)
            out[(name, n, nu, extrapolate)] = it.worst_level(truth, f64)
    return out


@pytest.mark.parametrize('n', it.POINT_SIZES)
def test_points_cases_stay_under_the_cap(n):
    for name in it.POINT_FAMILIES:
        for key, level in point_levels(it.points_case(name, n), name, n).items():
            print('LEVEL cp_spline_points %-40s %.1f FLOOR' % (key, level))
            if it.points_used(*key):
                assert level <= st.CAP, (key, level)
            else:
                assert level > st.CAP, (key, level, 'is listed as over the cap and is not')


def test_tiny_and_stride64_points_cases_stay_under_the_cap():
    for name, case in (('n = 2', it.tiny_case(2)), ('n = 3', it.tiny_case(3)), ('stride 64', it.stride64_case())):
        for key, level in point_levels(case, name, case['x'].size).items():
            print('LEVEL cp_spline_points %-40s %.1f FLOOR' % (key, level))
            assert level <= st.CAP, (key, level)


@pytest.mark.parametrize('name', it.ROWS_KNOTS)
def test_rows_cases_stay_under_the_cap(name):
    for shape in it.ROWS_SHAPES:
        case = it.rows_case(name, shape)
        truth, f64 = (it.rows_values(case['x'], case['y'], case['m'], case['xq'], dtype) for dtype in (LD, 'f8'))
        level = it.worst_level(truth, f64)
        print('LEVEL cp_spline_rows_at_queries %-10s %-18s %.1f FLOOR' % (name, shape, level))
        # an infinite query gives NaN (a^3 - a is inf - inf), as a NaN query does; everything else is finite
        assert np.array_equal(np.isnan(truth), ~np.isfinite(case['xq']))
        if (name, shape) in it.ROWS_OVER_CAP:
            assert level > st.CAP
        else:
            assert level <= st.CAP, (name, shape, level)


def test_a_query_on_a_knot_is_the_sample_in_the_restatements():
    case = it.rows_case('jitter100', (7, 300, 41))
    f64 = it.rows_values(case['x'], case['y'], case['m'], case['xq'], 'f8')
    on = np.isin(case['xq'], case['x'])
    at = np.searchsorted(case['x'], case['xq'][on])
    assert on.sum() > 80 and np.array_equal(f64[on], case['y'][np.nonzero(on)[0], at])


# ---- mutations ---------------------------------------------------------------------------------------------------------------------------------------------
def loop_model(nx, threads, mutation=None):
    """The kernel's loop as index arithmetic: (src, flagged) -- src[k] the sample whose result ends in out[k] (-1: not written; k = nx is the element behind the
    output), flagged[j] whether an outside sample j raises the flag."""
    j = np.arange(nx, dtype='i4')
    chunk = j // np.int32(threads)
    u, trip = chunk % it.TABLE_U, chunk // it.TABLE_U
    done = np.ones(nx, dtype=bool)
    if mutation == 'live computed against nx - 1':
        done &= j < nx - 1
    if mutation == 'the second trip skipped':
        done &= trip == 0
    dest = j - u * threads if mutation == 'slot u stores to i' else j
    src = np.full(nx + 1, -1, dtype='i4')
    for slot in range(it.TABLE_U):
        sel = done & (u == slot)
        src[dest[sel]] = j[sel]
    flagged = done & (u == it.TABLE_U - 1) if mutation == 'flag taken from the last slot only' else done
    return src, flagged


@functools.lru_cache(maxsize=None)
def loop_outcome(nx, threads, mutation):
    """(every output is the result of its own sample and nothing else is written -- results of different samples differ --, flagged)."""
    src, flagged = loop_model(nx, threads, mutation)
    return np.array_equal(src[:-1], np.arange(nx)) and src[-1] == -1, flagged


def loop_case_passes(nx, threads, bad, mutation):
    """Whether a device case (nx samples, ``bad`` the indices of the outside ones) passes on a kernel with this mutation: the outputs and the flag as they
    should be."""
    right, flagged = loop_outcome(nx, threads, mutation)
    return right and bool(flagged[bad].any()) == bool(len(bad))


def device_loop_cases():
    for nx in it.TABLE_NX:
        yield 'nx = %d' % nx, nx, []
    for label, nx, j in it.flag_places():
        yield 'flag: ' + label, nx, [j]


LOOP_MUTATIONS = ['slot u stores to i', 'live computed against nx - 1', 'flag taken from the last slot only', 'the second trip skipped']


def test_loop_mutations_are_caught():
    cases = list(device_loop_cases())
    for label, nx, bad in cases:
        assert loop_case_passes(nx, it.table_plan(nx)['stride'], bad, None), label
    for mutation in LOOP_MUTATIONS:
        caught = [label for label, nx, bad in cases if not loop_case_passes(nx, it.table_plan(nx)['stride'], bad, mutation)]
        print('MUTATION %-40s caught by %s' % (mutation, caught))
        assert caught, mutation
        # and by the host cases with T = 8
        host = [nx for nx in HOST_NX if not all(loop_case_passes(nx, T, [j], mutation) for j in range(nx))]
        assert host, mutation
    # none of today's cases with nx <= 1 048 576 would catch a fault of the slots
    assert all(loop_case_passes(nx, it.table_plan(nx)['stride'], [0], 'slot u stores to i') for nx in (1000, 260000))


def loop_on_samples(x, f, q, mutation):
    """(out with its guard element, flag) of the index model with T = 8 on real samples: what a kernel with this mutation leaves in a buffer of canaries."""
    src, flagged = loop_model(q.size, T, mutation)
    out = np.full(q.size + 1, CANARY)
    out[src >= 0] = it.interp(q, x, f)[src[src >= 0]]
    return out, int((it.is_outside(q, x) & flagged).any())


def test_loop_mutations_are_caught_on_samples():
    """The same four mutations at T = 8 on samples of the DESI table: without a mutation the model leaves what the emulated C++ loop leaves, bit for bit,
    so the model is the loop; with one, some host case differs from it in a value, an unwritten element or the flag."""
    x, f = it.table('desi')
    law = ith.find_law(x)
    clean = it.pool(x, 4000, seed=1)
    for mutation in [None] + LOOP_MUTATIONS:
        caught = []
        for k, nx in enumerate(HOST_NX):
            for j in range(-1, nx):      # -1: clean samples; else the one outside sample at j
                q = np.ascontiguousarray(clean[97 * k:97 * k + nx])
                if j >= 0:
                    q[j] = np.nan
                out, flag = loop(x, f, law, q)
                got, raised = loop_on_samples(x, f, q, mutation)
                if not (np.array_equal(out, got, equal_nan=True) and flag == raised):
                    caught.append((nx, j))
        print('MUTATION on samples %-40s caught by %d host cases, the first %s' % (mutation, len(caught), caught[:1]))
        assert bool(caught) == (mutation is not None), (mutation, caught[:3])


def search_model(x, v, mutation=None):
    """(lo, highest knot index read) of the coarse-then-fine bisection of interp_linear_kernel / spline_points_kernel for samples x[0] <= v; a knot read
    behind the table reads NaN."""
    n = x.size
    stride, ncoarse = it.coarse(n, fixed_stride=mutation == 'coarse stride fixed at 32')
    padded = np.concatenate([x, np.full(2 * stride + 2, np.nan)])
    top = 0
    lo = np.zeros(v.size, dtype='i8')
    last = v >= x[-1]
    lo[last] = n - 1 if mutation == 'lo = n - 1 at the last knot' else n - 2
    w = v[~last]
    clo, chi = np.zeros(w.size, dtype='i8'), np.full(w.size, ncoarse)
    while (chi - clo > 1).any():
        mid = (clo + chi) >> 1
        go = chi - clo > 1
        up = go & (padded[np.minimum(mid * stride, padded.size - 1)] <= w)
        clo, chi = np.where(up, mid, clo), np.where(go & ~up, mid, chi)
    l = clo * stride
    h = l + stride if mutation == 'hi of the fine bisection not clipped at n - 1' else np.minimum(l + stride, n - 1)
    while (h - l > 1).any():
        mid = (l + h) >> 1
        go = h - l > 1
        top = max(top, int(mid[go].max()))
        up = go & (padded[mid] <= w)
        l, h = np.where(up, mid, l), np.where(go & ~up, mid, h)
    lo[~last] = l
    top = max(top, int(lo.max()) + 1)      # the interval's upper knot
    return lo, top, (stride, ncoarse)


SEARCH_MUTATIONS = ['hi of the fine bisection not clipped at n - 1', 'coarse stride fixed at 32', 'lo = n - 1 at the last knot']


def search_case_passes(n, mutation):
    x = it.bisect_table(n)[0]
    if n < 2:
        return True
    v = it.pool(x, 3000, seed=n)
    lo, top, plan = search_model(x, v, mutation)
    return plan == BISECT_EXPECT[n][:2] and top <= n - 1 and np.array_equal(lo, np.clip(np.searchsorted(x, v, side='right') - 1, 0, n - 2))


def test_search_mutations_are_caught():
    for n in it.BISECT_N:
        assert search_case_passes(n, None), n
    for mutation in SEARCH_MUTATIONS:
        caught = [n for n in it.BISECT_N if not search_case_passes(n, mutation)]
        print('MUTATION %-48s caught by n = %s' % (mutation, caught))
        assert caught, mutation
    assert 262146 in [n for n in it.BISECT_N if not search_case_passes(n, SEARCH_MUTATIONS[0])]
    assert [n for n in it.BISECT_N if not search_case_passes(n, SEARCH_MUTATIONS[1])] == [131073, 262145, 262146, 524289]


def mutated_rows(case, mutation):
    """The float64 restatement of the rows formula with a and b exchanged, or with xq read as if it were stored query-major."""
    x, y, m, xq = case['x'], case['y'], case['m'], case['xq']
    nrows, nq = xq.shape
    if mutation == 'xq read with the transposed index':
        xq = xq.reshape(-1)[(np.arange(nq)[None, :] * nrows + np.arange(nrows)[:, None]) % xq.size]
    j = np.clip(np.searchsorted(x, xq.reshape(-1), side='right').reshape(xq.shape) - 1, 0, x.size - 2)
    j = np.where(xq != xq, 0, j)
    h = x[j + 1] - x[j]
    with np.errstate(invalid='ignore'):
        a, b = (x[j + 1] - xq) / h, (xq - x[j]) / h
        if mutation == 'a and b swapped in the rows formula':
            a, b = b, a
        take = lambda t, k: np.take_along_axis(t, k, axis=1)      # noqa: E731
        return a * take(y, j) + b * take(y, j + 1) + ((a * a * a - a) * take(m, j) + (b * b * b - b) * take(m, j + 1)) * (h * h) / 6


def rows_case_passes(name, shape, mutation):
    case = it.rows_case(name, shape)
    truth, f64 = (it.rows_values(case['x'], case['y'], case['m'], case['xq'], dtype) for dtype in (LD, 'f8'))
    got = f64 if mutation is None else mutated_rows(case, mutation)
    try:
        st.assert_within(got, truth, f64, '%s %s %s' % (name, shape, mutation))
    except AssertionError:
        return False
    return True


def test_rows_mutations_are_caught():
    shapes = [(1, 2, 1), (7, 300, 41), (64, 300, 65)]
    for shape in shapes:
        assert rows_case_passes('log10', shape, None)
    for mutation in ('a and b swapped in the rows formula', 'xq read with the transposed index'):
        caught = [shape for shape in shapes if not rows_case_passes('log10', shape, mutation)]
        print('MUTATION %-40s caught by %s' % (mutation, caught))
        assert caught, mutation
