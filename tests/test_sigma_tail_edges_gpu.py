"""GPU: the row kernels of csrc/cp_sigma.hip -- fftlog_spline_kernel (cp_fftlog_spline_execute) and fftlog_geospline_kernel<false>, <true, 4>, <true, 8>
(cp_fftlog_geospline_execute, CU solve and prefiltered) -- against the longdouble truth of tests/sigma_truth.py, through the C ABI: cp_fftlog_plan_create with
five-tap u tables (the transform is then a sparse circular correlation, exact in longdouble), LinearOperator.dense with weights of the test's making,
cp_geospline_plan_create / _create_prefiltered on the geometric grid.  tests/test_sigma_truth_host.py holds the truths, the cap of every case used here and
the mutations these cases catch.  Allowance: ALLOW = 16 levels of the float64 restatements per (row, 64 radii) block, against the local scale of the truth
(the module's docstring); + 1e-16 behind the root; a row packed with a larger partner that the front end leaves unscaled (exponents within
CP_ROW_SCALE_SPREAD = 4) is allowed the ratio of the two, as cp_fftlog_body.h states and tests/test_sigma_truth_host.py measures on the float64 packed
transform.  Every test prints the largest fraction of its allowance that was used.

  band operator   nq 1 ... 513 at bw = 44; bw 1, 7, 8, 9, 16, 17, 1024 at nq = 257 (chunks of 8 and their tails, a full row); bands from knot 0 and to knot
                  1023, one padded beyond knot 1023 (the clamp); NaN queries and rows of zeros first, last and in both slots of a thread; both post ops;
                  a real natural-spline operator (bandwidth 64 at the 1e-18 threshold); 1, 2, 3 rows and a second trip of the grid with an odd count; a
                  NaN sample in row 2j and in row 2j + 1; 2^+-300 inside a pair; more than 512 MiB of rows (stream_rows); 8055 queries, the LDS bound, and
                  8056 refused
  CU solve        S = 4 ... 8 at need = 64 S and one more than 64 (S - 1); ws = 2 and ws + ne = n - 2; radii on knots, repeated, unsorted, outside the
                  grid in every block of 64; nq 1 ... 512; the root and its NaN; batches as above; groups of 2, 10, 64 with fewer tables than XCDs, 9 tables
                  and a second round
  prefiltered     the same radii and batches; 256 / 257 radii (QS = 4 / 8); ne + 2 = 373, 374, 512; the last pair of a workgroup without a second row

Largest fraction of the allowance measured on the MI355X (1 is the limit; 1 / 16 = 0.0625 is the float64 restatement's own distance): fftlog_spline_kernel 0.27 at the
full row of 1024 weights, 0.06 to 0.20 otherwise; CU solve 0.16 at one radius whose level sits at one floor, 0.06 to 0.11 otherwise; prefiltered 0.077 (QS = 4) and
0.098 (QS = 8).  Without the factor of the unscaled pairs the second trip stood at 0.54 and the 65 539 rows beyond 512 MiB at 1.9 (two queries: a level near its
floor): pairs of random exponents within 2^4 of each other turn up in every long batch, and their smaller row rounds relative to the larger.
"""
import ctypes

import numpy as np
import pytest

import sigma_truth as sg
from sigma_device import CANARY, LDS_FFT, FftPlan, GeoPlan, synchronized

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


@pytest.fixture(scope='module')
def basis(env):
    torch, _lib, lib, dev, stream = env
    out = np.zeros(16)
    _lib.check(lib.cp_geospline_basis(ctypes.c_double(sg.RHO), _lib.as_double_p(out)))
    return out.reshape(4, 4)


def note(kernel, fraction):
    WORST[kernel] = max(WORST.get(kernel, 0.), fraction)
    print('MEASURED %-28s largest fraction of the allowance so far %.3f' % (kernel, WORST[kernel]))
    return fraction


def guarded(env, count):
    """count doubles of canaries and one more behind them."""
    torch, _lib, lib, dev, stream = env
    return torch.full((count + 1,), CANARY, dtype=torch.float64, device=dev)


def collect(env, out, shape):
    host = synchronized(env[0], out)
    assert host[-1] == CANARY, 'the element behind the output was written'
    got = host[:-1].reshape(shape)
    assert not (got == CANARY).any(), '{:d} output elements were not written'.format(int((got == CANARY).sum()))
    return got


def band_execute(env, fft, op, rows, post):
    torch, _lib, lib, dev, stream = env
    tin = rows if torch.is_tensor(rows) else torch.as_tensor(np.ascontiguousarray(rows, dtype='f8'), device=dev)
    out = guarded(env, tin.shape[0] * op.nq)
    _lib.check(lib.cp_fftlog_spline_execute(fft.handle, op._handle, tin.data_ptr(), out.data_ptr(), tin.shape[0], int(post), stream))
    return collect(env, out, (tin.shape[0], op.nq))


def geo_execute(env, fft, plan, rows, post, group=0):
    """(nbatch, nq), the grouped layout (tables, nq, group) brought back to rows."""
    torch, _lib, lib, dev, stream = env
    tin = torch.as_tensor(np.ascontiguousarray(rows, dtype='f8'), device=dev)
    nbatch, nq = tin.shape[0], plan.r.size
    out = guarded(env, nbatch * nq)
    _lib.check(lib.cp_fftlog_geospline_execute(None if fft is None else fft.handle, plan.handle, tin.data_ptr(), out.data_ptr(), nbatch, int(group), int(post), stream))
    if group:
        return collect(env, out, (nbatch // group, nq, group)).transpose(0, 2, 1).reshape(nbatch, nq)
    return collect(env, out, (nbatch, nq))


def held(case, got, what, nan_rows=()):
    """The fraction of the allowance the device's rows use: row i belongs to base row i % 2 times its 2**e; ``nan_rows`` hold a NaN sample."""
    nbatch = len(got)
    true, scale = sg.tile(case['true'], nbatch).copy(), sg.tile(case['scale'], nbatch)
    true[list(nan_rows)] = np.nan
    extra = sg.SQRT_EXTRA if case['post_sqrt'] else 0.
    widen = sg.pair_factors(case['syn'], case['base'], sg.exponents(nbatch, case['root']), nan_rows)      # (pairs the kernel leaves unscaled: the module's docstring)
    return sg.fraction(sg.unscale(got, case['root'], case['post_sqrt']), true, scale, case['level'], case['post_sqrt'], extra, what='%s, %s' % (what, case['name']),
                       widen=widen)


def batch_rows(case, nbatch, nan_rows=()):
    rows = sg.batch(case['base'], nbatch, case['root'])
    for i, row in enumerate(nan_rows):
        rows[row, (100 + 411 * i) % sg.N] = np.nan
    return rows


def second_trip(env):
    """More pairs than one trip of the grid, an odd count of rows."""
    torch, dev = env[0], env[3]
    return torch.cuda.get_device_properties(dev).multi_processor_count * 4 * 2 + 3


# ---- cp_fftlog_spline_execute ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c[0] for c in sg.band_cases()])
def test_band_operator(env, name):
    from cosmoprimo_amd.spline import LinearOperator
    case = sg.band_case(name)
    op = LinearOperator.dense(case['w'], device=env[3])
    assert op.bandwidth == sg.band_of(case['w'])[2]
    with FftPlan(env, case['syn']) as fft:
        assert env[2].cp_sigma_rz_fused_available(fft.handle, op._handle) == 1
        got = band_execute(env, fft, op, batch_rows(case, 3), case['post_sqrt'])
    assert note('fftlog_spline_kernel', held(case, got, 'band operator')) <= 1.


def test_band_real_spline_operator(env):
    from cosmoprimo_amd.spline import LinearOperator
    case = sg.spline_operator_case()
    op = LinearOperator.spline(sg.S_GRID, case['r'], bc='natural', device=env[3])
    print('LinearOperator.spline(natural) on the geometric grid: bandwidth %d' % op.bandwidth)
    assert op.bandwidth == sg.band_of(case['w'])[2]
    with FftPlan(env, case['syn']) as fft:
        got = band_execute(env, fft, op, batch_rows(case, 5), 0)
    assert note('fftlog_spline_kernel', held(case, got, 'natural spline operator')) <= 1.


def test_band_batches(env):
    """1, 2, 3 rows; a NaN sample in row 2j and in row 2j + 1 (their partners untouched); a second trip of the grid with an odd count: every row held."""
    from cosmoprimo_amd.spline import LinearOperator
    for name in ('nq257_bw44', 'root_nq257_bw9'):
        case = sg.band_case(name)
        op = LinearOperator.dense(case['w'], device=env[3])
        with FftPlan(env, case['syn']) as fft:
            for nbatch, nan_rows in ((1, ()), (2, ()), (3, ()), (9, (2, 5)), (second_trip(env), (0, second_trip(env) - 1))):
                got = band_execute(env, fft, op, batch_rows(case, nbatch, nan_rows), case['post_sqrt'])
                assert note('fftlog_spline_kernel', held(case, got, '%d rows' % nbatch, nan_rows)) <= 1.


def test_band_beyond_512_mib(env):
    """One launch of more than 512 MiB of rows (stream_rows), two queries; the rows are formed on the device from the base rows by exact scaling."""
    torch, _lib, lib, dev, stream = env
    from cosmoprimo_amd.spline import LinearOperator
    nbatch = (512 << 20) // (8 * sg.N) + 3
    assert nbatch * sg.N * 8 > 512 << 20
    syn, base, y_true, y_f64 = sg._transformed('spread', False)
    w = sg.dense_weights([(3, 44), (sg.N - 44, 44)], seed=7)
    true, scale = sg.band_truth(w, y_true), sg.band_scale(w, y_true)
    level = sg.levels(true, scale, [sg.band_product(w, y_f64)])
    assert float(level.max()) < sg.CAP * sg.FLOOR
    case = dict(name='%d rows x 2 queries' % nbatch, true=true, scale=scale, level=level, post_sqrt=False, root=False, syn=syn, base=base)
    factor = torch.as_tensor(np.ldexp(1., sg.exponents(nbatch)), device=dev)      # (exact powers of two: the products are exact)
    rows = (torch.as_tensor(base, device=dev)[torch.arange(nbatch, device=dev) % 2] * factor[:, None]).contiguous()
    assert rows.dtype == torch.float64 and bool(torch.isfinite(rows).all())
    op = LinearOperator.dense(w, device=dev)
    with FftPlan(env, syn) as fft:
        got = band_execute(env, fft, op, rows, 0)
    del rows
    assert note('fftlog_spline_kernel', held(case, got, 'stream_rows')) <= 1.


def test_band_lds_bound(env):
    """The largest number of queries the 160 KiB of a workgroup admit, (163840 - 34960) / 16 = 8055, runs and is held; one more is refused."""
    torch, _lib, lib, dev, stream = env
    from cosmoprimo_amd.spline import LinearOperator
    nq = (160 * 1024 - LDS_FFT) // 16
    assert LDS_FFT + 16 * nq == 160 * 1024
    syn, base, y_true, y_f64 = sg._transformed('spread', False)
    w = sg.dense_weights(sg.band_layout(nq + 1, 9, seed=3), seed=3)
    true, scale = sg.band_truth(w, y_true), sg.band_scale(w, y_true)
    level = sg.levels(true[:, :nq], scale[:, :nq], [sg.band_product(w[:nq], y_f64)])
    assert float(level.max()) < sg.CAP * sg.FLOOR
    case = dict(name='%d queries' % nq, true=true[:, :nq], scale=scale[:, :nq], level=level, post_sqrt=False, root=False, syn=syn, base=base)
    with FftPlan(env, syn) as fft:
        got = band_execute(env, fft, LinearOperator.dense(w[:nq], device=dev), batch_rows(case, 3), 0)
        assert note('fftlog_spline_kernel', held(case, got, 'LDS bound')) <= 1.
        over = LinearOperator.dense(w, device=dev)
        rows = torch.as_tensor(batch_rows(case, 3), device=dev)
        out = guarded(env, 3 * (nq + 1))
        assert lib.cp_fftlog_spline_execute(fft.handle, over._handle, rows.data_ptr(), out.data_ptr(), 3, 0, stream) == _lib.CP_EUNSUPPORTED
        torch.cuda.synchronize()
        assert bool((out == CANARY).all())


# ---- cp_fftlog_geospline_execute, the spline solved on the CU ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c[0] for c in sg.cu_cases()])
def test_cu_solve(env, name):
    case = sg.cu_case(name)
    with FftPlan(env, case['syn']) as fft, GeoPlan(env, case['r']) as plan:
        assert plan.info() == case['plan'][:2] + (case['r'].size,)
        got = geo_execute(env, fft, plan, batch_rows(case, 3), case['post_sqrt'])
    assert note('fftlog_geospline_kernel<false>', held(case, got, 'CU solve')) <= 1.


def mixed(env, family, basis, fft_of, plan_of):
    case = sg.mixed_sign_case(family, basis)
    nbatch = 3
    rows = sg.batch(case['base'], nbatch, root=True)
    with fft_of(case) as fft, plan_of(case) as plan:
        got = geo_execute(env, fft if family == 'cu' else None, plan, rows, 1)
    true, scale = sg.tile(case['true'], nbatch), sg.tile(case['scale'], nbatch)
    assert (true[np.isfinite(true)] < 0).any()
    return sg.mixed_fraction(sg.unscale(got, True, True), true, scale, case['level'], what='%s, root of rows of both signs' % family,
                             widen=sg.pair_factors(case['syn'], case['base'], sg.exponents(nbatch, True)))


def test_cu_solve_root_of_both_signs(env, basis):
    assert note('fftlog_geospline_kernel<false>', mixed(env, 'cu', basis, lambda c: FftPlan(env, c['syn']), lambda c: GeoPlan(env, c['r']))) <= 1.


@pytest.mark.parametrize('prefiltered', [False, True])
def test_geospline_batches(env, basis, prefiltered):
    """1, 2, 3 rows (one pair in all; a last pair without a second row, evaluated behind the loop in the prefiltered form), a NaN sample in row 2j and in
    row 2j + 1, and a second trip with an odd count, plain layout."""
    kernel = 'fftlog_geospline_kernel<true>' if prefiltered else 'fftlog_geospline_kernel<false>'
    for name in ('nq257', 'root_nq257'):
        case = sg.prefiltered_case(name, basis) if prefiltered else sg.cu_case(name)
        with FftPlan(env, case['syn']) as fft, GeoPlan(env, case['r'], case['syn'] if prefiltered else None) as plan:
            for nbatch, nan_rows in ((1, ()), (2, ()), (3, ()), (9, (2, 5)), (second_trip(env), (0, second_trip(env) - 1))):
                got = geo_execute(env, None if prefiltered else fft, plan, batch_rows(case, nbatch, nan_rows), case['post_sqrt'])
                assert note(kernel, held(case, got, '%d rows' % nbatch, nan_rows)) <= 1.


@pytest.mark.parametrize('prefiltered', [False, True])
@pytest.mark.parametrize('group', [2, 10, 64])
def test_geospline_grouped(env, basis, prefiltered, group):
    """The grouped layout out[table, q, row in group] and its walk over the XCDs: 3 tables (five XCD shares empty), 9 (uneven shares), and as many as need a
    second round of the workgroups of an XCD."""
    torch, dev = env[0], env[3]
    kernel = 'fftlog_geospline_kernel<true>' if prefiltered else 'fftlog_geospline_kernel<false>'
    case = sg.prefiltered_case('nq257', basis) if prefiltered else sg.cu_case('nq257')
    slots = max(1, torch.cuda.get_device_properties(dev).multi_processor_count * 4 // 8)      # workgroups of one XCD in a round
    two_rounds = 8 * (slots // (group // 2)) + 9      # per XCD more pairs than slots
    with FftPlan(env, case['syn']) as fft, GeoPlan(env, case['r'], case['syn'] if prefiltered else None) as plan:
        for tables in (3, 9, two_rounds):
            nbatch = tables * group
            nan_rows = (1, nbatch - 2) if nbatch > 4 else ()
            got = geo_execute(env, None if prefiltered else fft, plan, batch_rows(case, nbatch, nan_rows), case['post_sqrt'], group)
            assert note(kernel, held(case, got, '%d tables of %d' % (tables, group), nan_rows)) <= 1.


# ---- cp_fftlog_geospline_execute, prefiltered ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c[0] for c in sg.prefiltered_cases()])
def test_prefiltered(env, basis, name):
    case = sg.prefiltered_case(name, basis)
    with GeoPlan(env, case['r'], case['syn']) as plan:
        assert plan.info() == case['plan'] + (case['r'].size,)
        got = geo_execute(env, None, plan, batch_rows(case, 3), case['post_sqrt'])
    kernel = 'fftlog_geospline_kernel<true, %d>' % (4 if case['r'].size <= 256 else 8)
    assert note(kernel, held(case, got, 'prefiltered')) <= 1.


def test_prefiltered_root_of_both_signs(env, basis):
    import contextlib
    assert note('fftlog_geospline_kernel<true, 4>', mixed(env, 'prefiltered', basis, lambda c: contextlib.nullcontext(), lambda c: GeoPlan(env, c['r'], c['syn']))) <= 1.
