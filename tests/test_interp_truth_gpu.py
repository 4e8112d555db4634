"""GPU: the point-interpolation kernels of csrc/cp_interp.hip -- interp_linear_kernel, flag_outside_kernel, interp_table_kernel<1 | 2, double | float>,
spline_points_kernel / spline_points_lds_kernel and spline_rows_at_queries_kernel -- at their launch edges, through the C ABI (cp_interp_linear,
cp_interp_table_*, cp_spline_points, cp_spline_rows_at_queries) into buffers of canaries: every output element written, the one behind the output untouched.
tests/interp_truth.py holds the restated launch plan, the cases with the edge each is there for, and the truths; tests/test_interp_truth_host.py holds the plan
of every case, the cap of every spline case, the emulated four-in-flight loop and the mutations these cases catch.

  piecewise linear   bit for bit numpy.interp (compared as integers: signed zeros and infinities included; NaN for NaN).  Law 1 and law 2 (the DESI shape), double and float samples, nx from 1 to 5 243 137: slots 1, 2, 3 of a thread
                     with one live sample, full, and a second trip; the small tables (leading knots, the edge of acceptance, 1e-300 ... 1e300, subnormal
                     knots, no law); the bisection at coarse strides 32 / 64 / 128 / 256 with last blocks of one and two knots and up to three trips, directly
                     and through an irregular table; infinite table values on all three kernels; the range flag with the one bad sample first, last, in
                     the last thread of the last block and in every slot of both trips (7 344 131 samples), in the second trip of flag_outside_kernel, with
                     and without asking; float samples on an irregular table refused with nothing written
  cp_spline_points   16 levels of the float64 restatement per column against the longdouble Hermite evaluation of the float64 (xk, y, s) as given:
                     five knot families x n = 119, 2048, 2049 x ncol 1, 2, 3, 64 x nu 0, 1, 2 x extrapolate 0, 1; nq from 1 to 524 289 (both sides of the
                     LDS kernel's threshold, second trips of both kernels); n = 2, 3; 131 073 knots (stride 64); NaN queries first, last and inside; NaN one
                     ulp outside without extrapolation; a query on a knot (nu = 0), the last knot too, returns the sample bit for bit
                     (which of the two kernels a call takes is named from the restated plan; the launch itself is not observed)
  cp_spline_rows_at_queries   the same rule per row, both layouts (the transposed output the exact transpose), (nrows, n, nq) from (1, 2, 1) to (1025, 119, 1024)
                     on the filter's log10 knots and on uneven knots; queries on the knots return y bit for bit; +-inf and NaN queries give NaN (a^3 - a is
                     inf - inf), in the truth as on the device

Largest fraction of the allowance measured on the MI355X (1 is the limit; 1 / 16 = 0.0625 is a float64 restatement's own distance): spline_points_kernel 0.486
(the float64 restatement of the kernel's own arithmetic gives the same figure: the file is compiled without contraction), spline_points_lds_kernel 0.076,
spline_rows_at_queries_kernel 0.137.  Every piecewise-linear result has numpy's bits.  No case was dropped for the cap (levels 1 to 29 FLOOR,
tests/test_interp_truth_host.py prints them); the 131 073 knots are a unit apart, because with knots 3e-4 apart the second derivative stands at 27 783 FLOOR.

Found and fixed: a query on the LAST knot with nu = 0 did not return the last sample.  Both spline-point kernels served it from the far end of the last
interval, c0 + h (c1 + h (c2 + h c3)), which rounds: on the MI355X 13 of the 15 (family, n) cases of test_points_families failed there, and in the float64
restatement of that arithmetic 49 of their 105 base columns are off by one to 150 ulp (3.3e-14 of the sample on logk_pad, whose last interval is 1 wide under
samples that fall by a factor of 3).  spline_points_kernel and spline_points_lds_kernel now return y[n - 1] there, as they return y[k] on every other knot
(u = 0).  Smallest failing case: ('uniform', 119), ncol 3, nq 8209, nu 0.
"""
import ctypes
import functools

import numpy as np
import pytest

import interp_truth as it
import spline_truth as st
from sigma_device import CANARY, synchronized

pytestmark = pytest.mark.gpu

LD = np.longdouble
CANARY32 = float(np.float32(-1.2345679e37))
WORST = {}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


def note(variant, fraction):
    WORST[variant] = max(WORST.get(variant, 0.), fraction)
    print('MEASURED %-36s largest fraction of the allowance so far %.3f' % (variant, WORST[variant]))
    return fraction


def guarded(env, count, single=False):
    torch = env[0]
    return torch.full((count + 1,), CANARY32 if single else CANARY, dtype=torch.float32 if single else torch.float64, device=env[3])


def collect(env, out):
    host = synchronized(env[0], out)
    canary = host.dtype.type(CANARY32 if host.dtype == np.float32 else CANARY)
    assert host[-1] == canary, 'the element behind the output was written'
    assert not (host[:-1] == canary).any(), '{:d} output elements were not written'.format(int((host[:-1] == canary).sum()))
    return host[:-1]


def on_device(env, a):
    return env[0].as_tensor(np.ascontiguousarray(a), device=env[3])


def same_bits(torch, a, b):
    """Elementwise: the same bits (signed zeros and infinities included), or both NaN."""
    as_int = torch.int32 if a.dtype == torch.float32 else torch.int64
    return (a.view(as_int) == b.view(as_int)) | (torch.isnan(a) & torch.isnan(b))


def same_on_device(env, out, ref, skip=()):
    """out (with its guard element) against ref, compared on the device: the guard intact, every element equal to ref's (NaN where ref has NaN) but those of
    ``skip``, which are NaN."""
    torch = env[0]
    nx = ref.numel()
    canary = CANARY32 if out.dtype == torch.float32 else CANARY
    got = out[:nx]
    equal = same_bits(torch, got, ref)
    wrong = int(synchronized(torch, (~equal).sum()))
    guard, nans = synchronized(torch, out[nx:]), synchronized(torch, torch.isnan(got[list(skip)])) if len(skip) else np.ones(0, dtype=bool)
    assert guard.size == 1 and guard[0] == np.asarray(canary, dtype=guard.dtype), 'the element behind the output was written'
    assert nans.all(), 'a sample outside the table did not give NaN'
    assert wrong == len(skip), '{:d} elements differ from numpy.interp ({:d} expected: the samples outside)'.format(wrong, len(skip))


class Table(object):
    """A cp_interp_table through the C ABI, destroyed on the way out."""

    def __init__(self, env, x, f):
        self.env, self.x, self.f, self.handle = env, np.ascontiguousarray(x), np.ascontiguousarray(f), ctypes.c_void_p()

    def __enter__(self):
        torch, _lib, lib, dev, stream = self.env
        _lib.check(lib.cp_interp_table_create(ctypes.byref(self.handle), self.x.size, _lib.as_double_p(self.x), _lib.as_double_p(self.f), dev.index))
        return self

    def __exit__(self, *exc):
        handle, self.handle = self.handle, ctypes.c_void_p()
        self.env[2].cp_interp_table_destroy(handle)
        return False

    def law(self):
        law, first = ctypes.c_int(), ctypes.c_longlong()
        self.env[1].check(self.env[2].cp_interp_table_law(self.handle, ctypes.byref(law), ctypes.byref(first)))
        return law.value, first.value

    def apply(self, tq, nx, ask=True):
        """(status, out with its guard element, flag): nx samples of tq into canaries; ``ask`` False: outside == NULL."""
        torch, _lib, lib, dev, stream = self.env
        single = tq.dtype == torch.float32
        out = guarded(self.env, nx, single)
        flag = ctypes.c_int(-7)
        entry = lib.cp_interp_table_apply_f32 if single else lib.cp_interp_table_apply
        status = entry(self.handle, tq.data_ptr(), out.data_ptr(), nx, ctypes.byref(flag) if ask else None, stream)
        return status, out, flag.value

    def clean(self, tq, nx, ref):
        status, out, flag = self.apply(tq, nx)
        assert status == 0 and flag == 0, (status, flag)
        same_on_device(self.env, out, ref[:nx])


def linear(env, tx, tf, n, tq, nx):
    torch, _lib, lib, dev, stream = env
    out = guarded(env, nx)
    _lib.check(lib.cp_interp_linear(tx.data_ptr(), tf.data_ptr(), n, tq.data_ptr(), out.data_ptr(), nx, dev.index, stream))
    return out


@functools.lru_cache(maxsize=None)
def large_pool64(name):
    return it.pool(it.table(name)[0], it.POOL_SIZE, seed=it.LARGE_TABLES.index(name))


@functools.lru_cache(maxsize=None)
def large_pool(name, dtype):
    x, f = it.table(name)
    q = large_pool64(name).astype(dtype)
    assert not it.is_outside(q, x).any()
    return q, it.interp(q, x, f)


# ---- piecewise linear --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['f8', 'f4'])
@pytest.mark.parametrize('name', it.LARGE_TABLES)
def test_table_kernel_slots_and_trips(env, name, dtype):
    """interp_table_kernel<1 | 2, double | float> at every nx of TABLE_NX: numpy's bits in every slot of both trips."""
    x, f = it.table(name)
    q, ref = large_pool(name, dtype)
    tq, tref = on_device(env, q), on_device(env, ref)
    with Table(env, x, f) as table:
        assert table.law() == it.TABLES[name][1:]
        for nx in it.TABLE_NX:
            table.clean(tq, nx, tref)
    assert np.array_equal(ref[:1000], it.interp(q[:1000], x, f)) and ref.dtype == q.dtype == np.dtype(dtype)


@pytest.mark.parametrize('name', it.SMALL_TABLES)
def test_small_tables(env, name):
    x, f = it.table(name)
    q = it.pool(x, it.SMALL_NX, seed=len(name))
    with Table(env, x, f) as table:
        assert table.law() == it.TABLES[name][1:], (name, table.law())
        table.clean(on_device(env, q), q.size, on_device(env, it.interp(q, x, f)))
        with np.errstate(over='ignore'):
            q32 = q.astype('f4')
        q32 = q32[~it.is_outside(q32, x)]
        if table.law()[0] and q32.size:      # (no float sample lies among the subnormal knots)
            table.clean(on_device(env, q32), q32.size, on_device(env, it.interp(q32, x, f)))
        else:
            assert name == 'subnormal knots' or not table.law()[0]
    assert not np.isnan(it.interp(q, x, f)).any()


@pytest.mark.parametrize('n', list(it.BISECT_N))
def test_bisection_strides_and_trips(env, n):
    """interp_linear_kernel, directly and through an irregular cp_interp_table."""
    x, f = it.bisect_table(n)
    sizes = [nx for m, nx in it.bisect_cases() if m == n]
    q = it.pool(x, max(sizes), seed=n)
    tx, tf, tq, tref = (on_device(env, a) for a in (x, f, q, it.interp(q, x, f)))
    with Table(env, x, f) as table:
        assert table.law() == (0, 0)
        for nx in sizes:
            same_on_device(env, linear(env, tx, tf, n, tq, nx), tref[:nx])
            table.clean(tq, nx, tref)


@pytest.mark.parametrize('name', ['uniform', 'desi', 'irregular'])
def test_infinite_table_values(env, name):
    """+inf at one knot, -inf at two neighbours, equal infinities at two neighbours: numpy's retry from the right knot and its common-value rule on all three
    kernels; NaN for a NaN sample."""
    x, f = it.table(name)
    f = it.infinite_values(f)
    q = it.pool(x, 3 * x.size + 20000, seed=3)
    q[-1] = np.nan
    ref = it.interp(q, x, f)
    assert np.isposinf(ref).sum() >= 8 and np.isneginf(ref).sum() >= 4 and np.isnan(ref).sum() == 1
    tq, tref = on_device(env, q), on_device(env, ref)
    with Table(env, x, f) as table:
        assert table.law() == it.TABLES[name][1:]
        status, out, flag = table.apply(tq, q.size)
        assert status == 0 and flag == 1
        same_on_device(env, out, tref)
        host = collect(env, out)
        assert np.array_equal(host[:-1].view('i8'), ref[:-1].view('i8')) and np.isnan(host[-1])      # the infinities with their signs
    if name == 'irregular':
        same_on_device(env, linear(env, on_device(env, x), on_device(env, f), x.size, tq, q.size), tref)


def flag_round(env, table, tq, tref, nx, j, bad):
    """One bad sample at j and nothing else outside: outside == 1 and NaN exactly there; the next asking call on clean samples returns 0; a call that does not
    ask returns the same values and leaves the following asking call at 0."""
    torch = env[0]
    keep = tq[j].clone()
    tq[j] = bad
    try:
        status, out, flag = table.apply(tq, nx)
        assert status == 0 and flag == 1, (status, flag)
        same_on_device(env, out, tref[:nx], skip=[j])
        status, silent, flag = table.apply(tq, nx, ask=False)
        assert status == 0 and flag == -7      # (not touched)
        assert bool(synchronized(torch, same_bits(torch, out, silent).all()))
    finally:
        tq[j] = keep
    table.clean(tq, min(nx, 1000), tref)


@pytest.mark.parametrize('name,dtype', [('uniform', 'f8'), ('desi', 'f8'), ('uniform', 'f4')])
def test_range_flag_in_every_slot(env, name, dtype):
    x, f = it.table(name)
    places = it.flag_places()
    size = max(nx for _, nx, _ in places)
    q, ref = large_pool(name, dtype)
    q, ref = np.resize(q, size), np.resize(ref, size)
    tq, tref = on_device(env, q), on_device(env, ref)
    ends = np.array([x[0], x[-1]]).astype(dtype)
    bads = [b for b in (np.nextafter(ends[0], ends.dtype.type(-np.inf)), np.nextafter(ends[1], ends.dtype.type(np.inf)), ends.dtype.type(np.nan)) if it.is_outside(b, x)]
    assert len(bads) == 3
    with Table(env, x, f) as table:
        table.clean(tq, size, tref)
        for k, (label, nx, j) in enumerate(places):
            flag_round(env, table, tq, tref, nx, j, float(bads[k % 3]))


def test_range_flag_of_the_irregular_table(env):
    """flag_outside_kernel past its first trip of 262 144 samples."""
    x, f = it.table('irregular')
    nx = it.FLAG_IRREGULAR_NX
    q = it.pool(x, nx, seed=5)
    tq, tref = on_device(env, q), on_device(env, it.interp(q, x, f))
    bads = [np.nextafter(x[0], -np.inf), np.nextafter(x[-1], np.inf), np.nan]
    with Table(env, x, f) as table:
        assert table.law() == (0, 0)
        table.clean(tq, nx, tref)
        for k, j in enumerate(it.FLAG_IRREGULAR_AT):
            flag_round(env, table, tq, tref, nx, j, float(bads[k % 3]))


def test_float_samples_on_an_irregular_table_are_refused(env):
    torch, _lib = env[0], env[1]
    x, f = it.table('irregular')
    tq = on_device(env, it.pool(x, 1000).astype('f4'))
    with Table(env, x, f) as table:
        status, out, flag = table.apply(tq, 1000)
        assert status == _lib.CP_EUNSUPPORTED
        assert (synchronized(torch, out) == np.float32(CANARY32)).all(), 'a refused call wrote to its output'
        status, out, flag = table.apply(tq, 1000, ask=False)
        assert status == _lib.CP_EUNSUPPORTED and (synchronized(torch, out) == np.float32(CANARY32)).all()


# ---- cp_spline_points ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_truth(name, n, nu, extrapolate):
    case = it.points_case(name, n)
    base = it.points_base(case['x'], extrapolate, seed=n)
    return (base,) + it.points_values(case, base, nu, extrapolate)


def points(env, tx, ty, ts, n, ncol, tq, nq, nu, extrapolate):
    torch, _lib, lib, dev, stream = env
    out = guarded(env, ncol * nq)
    _lib.check(lib.cp_spline_points(tx.data_ptr(), ty.data_ptr(), ts.data_ptr(), n, ncol, tq.data_ptr(), out.data_ptr(), nq, nu, extrapolate, dev.index, stream))
    return collect(env, out).reshape(ncol, nq)


def on_knots_exact(got, x, rows, q, what):
    """nu = 0: a query on a knot, the last one too, returns the sample bit for bit."""
    on = np.isin(q, x)
    at = np.searchsorted(x, q[on])
    assert (on.any() or q.size < it.POINT_BASE) and np.array_equal(got[:, on], rows[:, at]), '%s: a query on a knot does not return the sample' % what
    return set(at)


def within(got, truth, f64, nq, what):
    """``assert_within`` of a call whose query i is base query i % m.  From four periods on: every period bit for bit the second one (equal queries, equal
    arithmetic; NaN where the call has its NaN queries), and the first two periods against the truth."""
    m = truth.shape[-1]
    if nq < 4 * m:
        return st.assert_within(got, it.points_expand(truth, nq), it.points_expand(f64, nq), what, scaled=True)
    index, nan = it.points_index(nq, m)
    periodic = got[:, m:2 * m][:, index]
    periodic[:, nan] = np.nan
    assert np.array_equal(got, periodic, equal_nan=True), '%s: equal queries with different results' % what
    head = []
    for v in (truth, f64):
        v = np.concatenate([v, v], axis=-1)
        v[..., 0] = np.nan
        head.append(v)
    return st.assert_within(got[:, :2 * m], head[0], head[1], what, scaled=True)


def family_call(env, name, n, ncol, nq, combos, device_cache):
    """The calls of one (family, n, ncol, nq) judged; columns c = base column c % 7 times 2**e_c (exact: samples and slopes alike)."""
    case = it.points_case(name, n)
    x = case['x']
    rows, slopes = st.batch(case['y'], ncol), st.batch(case['s'], ncol)
    tx, ty, ts = (on_device(env, a) for a in (x, rows, slopes))
    plan = it.points_plan(n, ncol, nq)
    assert plan['kernel'] == ('spline_points_lds_kernel' if ncol == 1 and n <= 2048 and nq >= 65536 else 'spline_points_kernel')
    for nu, extrapolate in combos:
        assert it.points_used(name, n, nu, extrapolate)
        base, truth, f64 = point_truth(name, n, nu, extrapolate)
        q = it.points_queries(base, nq)
        key = (name, n, nq, extrapolate)
        if key not in device_cache:
            device_cache[key] = on_device(env, q)
        got = points(env, tx, ty, ts, n, ncol, device_cache[key], nq, nu, extrapolate)
        k = min(ncol, st.NBASE)
        what = '%s n %d ncol %d nq %d nu %d extrapolate %d (%s)' % (name, n, ncol, nq, nu, extrapolate, plan['kernel'])
        assert note(plan['kernel'], within(got, truth[:k], f64[:k], nq, what)) <= 1.
        if nq >= 257:
            assert np.isnan(got[:, [0, nq // 2, nq - 1]]).all()
        if nu == 0:
            hit = on_knots_exact(got, x, rows, q, what)
            assert nq < it.POINT_BASE or n - 1 in hit
        if not extrapolate and nq >= it.POINT_BASE:
            outside = (q < x[0]) | (q > x[-1])
            assert outside.sum() >= 2 and np.isnan(got[:, outside]).all()


ALL_COMBOS = [(nu, extrapolate) for nu in (0, 1, 2) for extrapolate in (0, 1)]


@pytest.mark.parametrize('n', it.POINT_SIZES)
@pytest.mark.parametrize('name', it.POINT_FAMILIES)
def test_points_families(env, name, n):
    cache = {}
    for ncol in it.POINT_NCOL:
        for nq in (1, 257, it.POINT_BASE):
            family_call(env, name, n, ncol, nq, ALL_COMBOS, cache)


@pytest.mark.parametrize('nq', list(it.POINT_NQ))
def test_points_counts(env, nq):
    """Both sides of the LDS kernel's threshold, one trip exactly and a second trip of either kernel, every (nu, extrapolate) at every ncol.  The kernel of a
    call is named from the restated plan (tests/interp_truth.py, held to the launch code's conditions by tests/test_interp_truth_host.py): the launch itself is
    not observed."""
    cache = {}
    taken = set()
    for name, n in it.POINT_COUNT_CASES:
        for ncol in (1, 2, 3, 64):
            if ncol > 2 and nq > 65536:      # the largest nq at ncol = 1 and 2 only
                continue
            family_call(env, name, n, ncol, nq, ALL_COMBOS, cache)
            taken.add(it.points_plan(n, ncol, nq)['kernel'])
    assert taken == ({'spline_points_kernel', 'spline_points_lds_kernel'} if nq >= 65536 else {'spline_points_kernel'})


def test_points_of_two_and_three_knots_and_stride_64(env):
    for label, case, counts in (('n = 2', it.tiny_case(2), (1, 257)), ('n = 3', it.tiny_case(3), (1, 257)), ('stride 64', it.stride64_case(), (257, 65536))):
        x, n, ncol = case['x'], case['x'].size, len(case['y'])
        tx, ty, ts = (on_device(env, case[key]) for key in ('x', 'y', 's'))
        for nq in counts:
            plan = it.points_plan(n, ncol, nq)
            assert plan['kernel'] == 'spline_points_kernel' and plan['stride'] == (64 if n > 3 else 32)
            for nu, extrapolate in ALL_COMBOS:
                base = it.points_base(x, extrapolate, seed=n)
                truth, f64 = it.points_values(case, base, nu, extrapolate)
                q = it.points_queries(base, nq)
                got = points(env, tx, ty, ts, n, ncol, on_device(env, q), nq, nu, extrapolate)
                what = '%s nq %d nu %d extrapolate %d' % (label, nq, nu, extrapolate)
                assert note(plan['kernel'], st.assert_within(got, it.points_expand(truth, nq), it.points_expand(f64, nq), what)) <= 1.
                if nu == 0 and nq > 1:
                    on_knots_exact(got, x, case['y'], q, what)


# ---- cp_spline_rows_at_queries ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', list(it.ROWS_SHAPES), ids=lambda shape: '%dx%dx%d' % shape)
@pytest.mark.parametrize('name', it.ROWS_KNOTS)
def test_rows_at_their_own_queries(env, name, shape):
    torch, _lib, lib, dev, stream = env
    nrows, n, nq = shape
    assert (name, shape) not in it.ROWS_OVER_CAP
    case = it.rows_case(name, shape)
    x, y, xq = case['x'], case['y'], case['xq']
    tx, ty, tm, tq = (on_device(env, case[key]) for key in ('x', 'y', 'm', 'xq'))
    got = {}
    for transposed in (0, 1):
        out = guarded(env, nrows * nq)
        _lib.check(lib.cp_spline_rows_at_queries(tx.data_ptr(), ty.data_ptr(), tm.data_ptr(), nrows, n, tq.data_ptr(), nq, out.data_ptr(), transposed, dev.index, stream))
        got[transposed] = collect(env, out).reshape((nq, nrows) if transposed else (nrows, nq))
    assert np.array_equal(got[1].T, got[0], equal_nan=True), 'the transposed output is not the transpose of the plain one'
    truth, f64 = (it.rows_values(x, y, case['m'], xq, dtype) for dtype in (LD, 'f8'))
    # NaN for a NaN query and for an infinite one (a^3 - a is inf - inf), on the device as in the truth: assert_within wants NaN exactly where the truth has it
    assert np.array_equal(np.isnan(truth), ~np.isfinite(xq))
    assert note('spline_rows_at_queries_kernel', st.assert_within(got[0], truth, f64, '%s %s' % (name, shape))) <= 1.
    on = np.isin(xq, x)      # on a knot a = 1, b = 0 (the last knot: a = 0, b = 1) exactly: y bit for bit
    at = np.searchsorted(x, xq[on])
    assert on.sum() >= nrows * nq // 4 and np.array_equal(got[0][on], y[np.nonzero(on)[0], at])


def test_every_variant_was_reached():
    for name in sorted(WORST):
        print('MEASURED %-36s %.3f' % (name, WORST[name]))
    assert sorted(WORST) == ['spline_points_kernel', 'spline_points_lds_kernel', 'spline_rows_at_queries_kernel']
