"""GPU: a plan gives back the device memory it took.  Every plan type of the C ABI is created and destroyed 100 times at the smallest size at which ALL
of its device tables exist -- a spline plan with its dense copy, a dense operator, a spline-rows plan, a spliced spline on the uniform-stretch
scheme (both sets of tables) and one on the elimination alone, the sine transform with and without its abscissa, the real FFT, the fused FFTLog, the
large-size FFTLog with its scratch, both geometric-spline constructors (the second owns a transform), interpolation tables with and without a law.
The plan is applied once in the first and once in the last cycle, to the same input: the two results must be equal bit for bit.  Then the free
device memory (``torch.cuda.mem_get_info``) must be where it was before the first cycle, within DRIFT_ALLOWED.

The bound: the larger of twice what the same loop drifted on the library before its plans were given one owner of their device tables (per type,
tools/bench_plan_tables.py, recorded in profiles/plan_tables.txt: zero for every type) and one 2 MB granule of the device allocator -- 2 MB for every
type.  What this test cannot see: a leaked table smaller than the bound divided by the 100 cycles, 20 KB, need not move the free memory by a granule
-- the 4-byte flag of an interpolation table, the constants of a geometric spline, the small tables of the sizes used here.  Their ownership is
checked call by call under fault injection on the host (tests/host_san/device_array_driver.cpp); here it is the large tables that count: the 128 MB
scratch of the large-size FFTLog, the dense copies, the tables of the transform a prefiltered spline owns.

The inputs and both outputs are allocated before the first reading, so that the caching allocator of the framework takes nothing from the device
inside the loop.  tools/bench_plan_tables.py runs the same cases (``CASES``) to time the constructors and destructors."""
import ctypes

import numpy as np
import pytest

CYCLES = 100
GRANULE = 2 << 20
DRIFT_PARENT = 0      # bytes, every type (profiles/plan_tables.txt)
DRIFT_ALLOWED = max(2 * DRIFT_PARENT, GRANULE)
NROWS = 8
DST_FUSED = 1      # CP_DST_FUSED


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _ip(values):
    return (ctypes.c_int * len(values))(*values)


def _fftlog_tables(npad, rng):
    return np.ones(npad), np.geomspace(1., 100., npad), rng.uniform(0.5, 1.5, size=2 * (npad // 2 + 1))


def cases(lib, device=0):
    """{name: (create, apply, destroy, input shape, output shape)}: ``create()`` returns a handle (ctypes.c_void_p) or raises, ``apply(handle, d_in,
    d_out, stream)`` runs the plan on device pointers of NROWS rows, ``destroy(handle)`` frees it."""
    from cosmoprimo_amd import _lib
    from test_plan_abi_errors_host import wallish_knots
    rng = np.random.default_rng(7)

    def creator(entry, *args):
        def create():
            handle = ctypes.c_void_p()
            _lib.check(getattr(lib, entry)(ctypes.byref(handle), *args))
            return handle
        create.keep = args      # (the host arrays live as long as the case)
        return create

    out = {}
    x64, xq256 = np.linspace(0., 1., 64), np.linspace(0., 1., 256)
    spline_apply = lambda h, d_in, d_out, s: lib.cp_spline_apply(h, d_in, d_out, NROWS, 0, 1., s)  # noqa: E731
    out['spline'] = (creator('cp_spline_plan_create', 64, _dp(x64), 256, _dp(xq256), 0, 0, 0, device), spline_apply, lib.cp_spline_plan_destroy, 64, 256)
    w = rng.normal(size=(80, 48))
    out['linop'] = (creator('cp_linop_plan_create', 48, 80, _dp(w), device), spline_apply, lib.cp_spline_plan_destroy, 48, 80)
    x128, xq64 = np.linspace(0., 1., 128), np.linspace(0.1, 0.9, 64)
    out['spline_rows'] = (creator('cp_spline_rows_plan_create', 128, _dp(x128), 0, 0, 64, _dp(xq64), device),
                          lambda h, d_in, d_out, s: lib.cp_spline_rows_apply(h, d_in, NROWS, 0, 1., 0, d_out, s), lib.cp_spline_rows_plan_destroy, 128, 64)
    knots, src, start, count, k = wallish_knots()
    # (rows of 4096: the first 1024 columns are the first array's, the rows themselves the second's -- the pieces address columns of either)
    out['splice_uniform'] = (creator('cp_splice_plan_create', knots.size, _dp(knots), 3, _ip(src), _ip(start), _ip(count), k.size, _dp(k), device),
                             lambda h, d_in, d_out, s: lib.cp_splice_apply(h, d_in, 4096, d_in, 4096, NROWS, None, d_out, s), lib.cp_splice_plan_destroy, 4096, 1024)
    g700, gq300 = np.geomspace(1e-4, 1., 700), np.geomspace(2e-4, 0.9, 300)
    out['splice_lds'] = (creator('cp_splice_plan_create', 700, _dp(g700), 1, _ip([0]), _ip([0]), _ip([700]), 300, _dp(gq300), device),
                         lambda h, d_in, d_out, s: lib.cp_splice_apply(h, d_in, 700, None, 0, NROWS, None, d_out, s), lib.cp_splice_plan_destroy, 700, 300)
    kx = np.geomspace(1e-3, 10., 256)
    out['dst_kx'] = (creator('cp_dst_plan_create', 256, _dp(kx), device), lambda h, d_in, d_out, s: lib.cp_dst_execute(h, d_in, d_out, NROWS, 0, DST_FUSED, s),
                     lib.cp_dst_plan_destroy, 256, 256)
    out['dst'] = (creator('cp_dst_plan_create', 256, None, device), lambda h, d_in, d_out, s: lib.cp_dst_execute(h, d_in, d_out, NROWS, 0, 0, s),
                  lib.cp_dst_plan_destroy, 256, 256)
    out['rfft'] = (creator('cp_rfft_plan_create', 256, device), lambda h, d_in, d_out, s: lib.cp_rfft_forward(h, d_in, d_out, NROWS, s), lib.cp_rfft_plan_destroy, 256, 258)
    fftlog_apply = lambda h, d_in, d_out, s: lib.cp_fftlog_execute(h, d_in, d_out, NROWS, 0, 0., 0, 0., 0, s)  # noqa: E731
    pre, post, u = _fftlog_tables(256, rng)
    out['fftlog'] = (creator('cp_fftlog_plan_create', 128, 256, 1, _dp(pre), _dp(post), _dp(u), device), fftlog_apply, lib.cp_fftlog_plan_destroy, 128, 128)
    pre, post, u = _fftlog_tables(1 << 14, rng)
    out['fftlog_large'] = (creator('cp_fftlog_plan_create', 1 << 13, 1 << 14, 1, _dp(pre), _dp(post), _dp(u), device), fftlog_apply, lib.cp_fftlog_plan_destroy,
                           1 << 13, 1 << 13)
    pre, post, u = _fftlog_tables(2048, rng)
    geo_knots, geo_queries = np.geomspace(1e-2, 1e2, 1024), np.geomspace(1., 10., 64)
    transform = creator('cp_fftlog_plan_create', 1024, 2048, 1, _dp(pre), _dp(post), _dp(u), device)
    shared = []      # the transform of the plain geometric spline: the caller's, made once, freed by free_shared()

    def geospline_apply(h, d_in, d_out, s):
        if not shared:
            shared.append(transform())
        return lib.cp_fftlog_geospline_execute(shared[0], h, d_in, d_out, NROWS, 0, 0, s)

    out['geospline'] = (creator('cp_geospline_plan_create', _dp(geo_knots), 1024, _dp(geo_queries), 64, device), geospline_apply, lib.cp_geospline_plan_destroy, 1024, 64)
    out['geospline_prefiltered'] = (creator('cp_geospline_plan_create_prefiltered', 1024, 2048, _dp(pre), _dp(post), _dp(u), _dp(geo_knots), _dp(geo_queries), 64, device),
                                    lambda h, d_in, d_out, s: lib.cp_fftlog_geospline_execute(None, h, d_in, d_out, NROWS, 0, 0, s), lib.cp_geospline_plan_destroy,
                                    1024, 64)
    irregular, uniform, f = np.cumsum(1. + 0.5 * np.sin(np.arange(64.))), np.linspace(0., 1., 64), rng.normal(size=64)
    interp_apply = lambda h, d_in, d_out, s: lib.cp_interp_table_apply(h, d_in, d_out, NROWS * 64, ctypes.byref(ctypes.c_int()), s)  # noqa: E731
    out['interp_law0'] = (creator('cp_interp_table_create', 64, _dp(irregular), _dp(f), device), interp_apply, lib.cp_interp_table_destroy, 64, 64)
    out['interp_law1'] = (creator('cp_interp_table_create', 64, _dp(uniform), _dp(f), device), interp_apply, lib.cp_interp_table_destroy, 64, 64)

    def free_shared():
        while shared:
            lib.cp_fftlog_plan_destroy(shared.pop())
    return out, free_shared


CASES = ['spline', 'linop', 'spline_rows', 'splice_uniform', 'splice_lds', 'dst_kx', 'dst', 'rfft', 'fftlog', 'fftlog_large', 'geospline',
         'geospline_prefiltered', 'interp_law0', 'interp_law1']


def inputs(name, n_in, torch, device):
    """(NROWS, n_in) positive values inside every case's range of samples (interpolation tables: inside their knots)."""
    rng = np.random.default_rng(11)
    lo, hi = {'interp_law0': (1., 60.), 'interp_law1': (0., 1.)}.get(name, (0.5, 1.5))
    return torch.as_tensor(rng.uniform(lo, hi, size=(NROWS, n_in)), device=device)


def cycle(lib, name, case, torch, device, cycles=CYCLES):
    """(first result, last result, free bytes before the first cycle - free bytes behind the last) of ``cycles`` create / destroy cycles of ``case``."""
    from cosmoprimo_amd import _lib
    create, apply, destroy, n_in, n_out = case
    d_in = inputs(name, n_in, torch, device)
    results = [torch.full((NROWS, n_out), float('nan'), dtype=torch.float64, device=device) for i in range(2)]
    stream = torch.cuda.current_stream(device).cuda_stream
    torch.cuda.synchronize(device)
    free_before = torch.cuda.mem_get_info(device)[0]
    for i in range(cycles):
        handle = create()
        if i in (0, cycles - 1):
            _lib.check(apply(handle, d_in.data_ptr(), results[min(i, 1)].data_ptr(), stream))
            torch.cuda.synchronize(device)
        _lib.check(destroy(handle))
    torch.cuda.synchronize(device)
    return results[0], results[1], free_before - torch.cuda.mem_get_info(device)[0]


@pytest.fixture(scope='module')
def built():
    import torch
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    device = torch.device('cuda', 0)
    table, free_shared = cases(lib)
    assert sorted(table) == sorted(CASES)
    # one cycle of every case ahead of the readings: code objects, the kernels' LDS opt-ins and the transform of 'geospline' load once per process
    for name in CASES:
        cycle(lib, name, table[name], torch, device, cycles=1)
    yield lib, table, torch, device
    free_shared()


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_create_destroy_cycles_return_the_memory(built, name):
    lib, table, torch, device = built
    first, last, drift = cycle(lib, name, table[name], torch, device)
    print('%s: free device memory drifted by %d bytes over %d cycles (allowed: %d)' % (name, drift, CYCLES, DRIFT_ALLOWED))
    assert bool(torch.isfinite(first).any())      # the plan ran
    assert torch.equal(first.view(torch.int64), last.view(torch.int64))
    assert drift <= DRIFT_ALLOWED, (name, drift)
