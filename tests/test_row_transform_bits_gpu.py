"""GPU: the results of the paired real-row transforms -- cp_rfft_forward / cp_rfft_backward, cp_dst_execute, the analytic entry points of the wallish2018
filter (cp_dst_forward_analytic, cp_dst_forward_analytic_box, cp_wallish_tail, cp_wallish_full) and the fused FFTLog tails (cp_sigma_rz_analytic,
cp_fftlog_spline_execute, cp_fftlog_geospline_execute) -- bit for bit, against tests/golden/row_transform_bits.npz: what the library gave while the
workgroup FFT, the handling of a pair and the phase chain of the fused tails were still written out in every kernel (recorded on an MI355X by
tools/gen_row_transform_bits.py, every call run twice there and refused if its two runs differed).  The only atomics of these kernels are an integer
atomicMax and atomicAdd, whose results do not depend on order, and a change of their source that keeps their instructions keeps every output, so every
output must be EQUAL: a tolerance would not see a barrier moved past a flag's reader, or a row screened with its partner's flag.

The inputs come from seeded numpy, so the file holds outputs only: one SHA-256 digest (32 bytes) per output row, and the names and shapes of the entries
the rows belong to -- a mismatch names its entry and its row.  The cases are the smallest that reach every shared piece:
  cp_dst_execute at n = 256, 1024, 4096: forward and inverse; flags none, CP_DST_SPLIT, CP_DST_FUSED | CP_DST_SPLIT with an abscissa; 3 rows (a pair and a
    row without a partner), and the same rows with an infinity in one row of the pair (the flagged-pair path of the inverse); at n = 256 one batch of
    2 * 512 + 3 rows, so that a workgroup takes a second pair;
  cp_rfft_forward / cp_rfft_backward at the twelve instantiated sizes: 3 rows, one with a NaN; conj_input both ways; at size 8 one batch of 2048 + 3 rows
    (the launch has at most 2048 workgroups);
  the analytic entry points with the three engines: 3 cosmologies, the second one driven non-finite (h = NaN); cp_wallish_full with and without d_coef;
  cp_sigma_rz_analytic by the band route and by the prefiltered route: 3 cosmologies, nz = 2 and 3 (the even and the odd store path), with and without
    d_pk_out;
  cp_fftlog_spline_execute on 3 rows, with and without the root;
  cp_fftlog_geospline_execute on a solved and on a prefiltered plan: 3 rows plain, 4 rows grouped by 2, with and without the root."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from test_analytic_front_bits_gpu import ENGINES, wallish_filter

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'row_transform_bits.npz')
DST_SIZES = [256, 1024, 4096]
DST_FLAGS = [('plain', False, False), ('split', False, True), ('fused_split', True, True)]
DST_LARGE = 2 * 512 + 3      # cp_dst_execute launches at most 512 workgroups, one pair each per trip
RFFT_SIZES = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]      # CP_RFFT_SIZES (csrc/cp_rfft.hip)
RFFT_LARGE = 2048 + 3        # rfft_run launches at most 2048 workgroups, one row each per trip
K = np.geomspace(1e-7, 1e2, 1024)
RADII = np.geomspace(1., 60., 8)


def _device():
    import torch
    return torch.device('cuda', 0)


def _up(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array), device=_device())


def _host(x):
    import torch
    torch.cuda.synchronize()
    return np.ascontiguousarray(x.cpu().numpy())


def digests(entries):
    """(labels 'name shape dtype', (rows, 32) uint8: the SHA-256 of every row -- the last axis -- of every entry, in the order of the names)."""
    names = sorted(entries)
    labels = np.array(['%s %s %s' % (name, entries[name].shape, entries[name].dtype) for name in names])
    rows = [hashlib.sha256(row.tobytes()).digest() for name in names for row in np.ascontiguousarray(entries[name]).reshape(-1, entries[name].shape[-1])]
    return labels, np.frombuffer(b''.join(rows), dtype='u1').reshape(-1, 32)


def assert_equal_rows(got, recorded, group):
    labels, rows = digests(got)
    assert list(labels) == list(recorded[group + '.entries']) and rows.shape == recorded[group].shape
    offset = 0
    for label, name in zip(labels, sorted(got)):
        count = got[name].size // got[name].shape[-1]
        differ = np.flatnonzero((rows[offset:offset + count] != recorded[group][offset:offset + count]).any(axis=1))
        assert differ.size == 0, '%s: %s: rows %s differ' % (group, label, differ[:8])
        offset += count


def dst_entries(n):
    from cosmoprimo_amd.dst import DST
    rng = np.random.default_rng(n)
    plan = DST(n, kx=np.linspace(1e-3, 2., n), device=_device())
    inputs = {'forward': rng.uniform(0.5, 2., (3, n)), 'inverse': rng.normal(0., 1., (3, n))}      # (the fused forward map takes logarithms)
    large = rng.normal(0., 1., (DST_LARGE, n)) if n == 256 else None
    out = {}
    for direction, rows in inputs.items():
        flagged = rows.copy()
        flagged[1, n // 3] = np.inf      # rows 0 and 1 share a transform
        for label, fused, split in DST_FLAGS:
            out['%s.%s' % (direction, label)] = _host(plan(_up(rows), inverse=direction == 'inverse', fused=fused, split=split))
            out['%s.%s.inf' % (direction, label)] = _host(plan(_up(flagged), inverse=direction == 'inverse', fused=fused, split=split))
        if large is not None:
            out['%s.large' % direction] = _host(plan(_up(large), inverse=direction == 'inverse'))
    return out


def rfft_entries():
    import torch
    from cosmoprimo_amd import _lib
    lib, dev, out = _lib.load(), _device(), {}
    stream = torch.cuda.current_stream(dev).cuda_stream
    for size in RFFT_SIZES:
        rng = np.random.default_rng(size)
        half = size // 2 + 1
        cases = [('', 3)] + ([('.large', RFFT_LARGE)] if size == RFFT_SIZES[0] else [])
        plan = ctypes.c_void_p()
        _lib.check(lib.cp_rfft_plan_create(ctypes.byref(plan), size, 0))
        try:
            for label, nrows in cases:
                x, z = rng.normal(0., 1., (nrows, size)), rng.normal(0., 1., (nrows, half)) + 1j * rng.normal(0., 1., (nrows, half))
                x[1, size // 3], z[2, 1] = np.nan, np.nan
                dx, dz = _up(x), _up(z)
                forward = torch.empty((nrows, half), dtype=torch.complex128, device=dev)
                _lib.check(lib.cp_rfft_forward(plan, dx.data_ptr(), forward.data_ptr(), nrows, stream))
                out['%d.forward%s' % (size, label)] = _host(forward)
                for conj_input in (1, 0) if not label else (1,):
                    backward = torch.empty((nrows, size), dtype=torch.float64, device=dev)
                    _lib.check(lib.cp_rfft_backward(plan, dz.data_ptr(), backward.data_ptr(), nrows, conj_input, stream))
                    out['%d.backward%s.conj%d' % (size, label, conj_input)] = _host(backward)
        finally:
            lib.cp_rfft_plan_destroy(plan)
    return out


def cosmologies(seed, bad=None):
    """(bg, pk) of 3 cosmologies; ``bad``: the one whose h is NaN."""
    rng = np.random.default_rng(seed)
    bg = dict(h=rng.uniform(0.6, 0.8, 3), Omega_cdm=rng.uniform(0.2, 0.3, 3), Omega_b=rng.uniform(0.04, 0.06, 3))
    if bad is not None:
        bg['h'][bad] = np.nan
    return bg, dict(n_s=0.96)


def analytic_entries(engine, f):
    import torch
    from cosmoprimo_amd import _lib, _device as dv, power as pw
    lib, dev, out = _lib.load(), _device(), {}
    bg, pk = cosmologies(31, bad=1)
    ops = f._operators()
    dst, splice, tophat = ops['dst'], ops['splice'], ops['tophat']
    box_args = (f._margin_first, f._margin_second, f._offset[0], f._offset[1])
    out['forward.plain'] = _host(dst.forward_analytic(engine, bg, pk))
    split = dst.forward_analytic(engine, bg, pk, split=True)
    out['forward.split'] = _host(split)
    coefficients, boxes = dst.forward_analytic(engine, bg, pk, split=True, box=box_args)
    out['forward.box'], out['forward.box.boxes'] = _host(coefficients), _host(boxes.view(-1, 4))
    rows = pw.analytic(engine, 'matter', f.k, bg=bg, pk=pk, device=dev).contiguous()
    assert tuple(rows.shape) == (3, f.k.size)
    stream = dv.stream_of(dev)
    coef, box, res = split.clone(), torch.empty((6, 2), dtype=torch.int32, device=dev), torch.empty_like(rows)
    _lib.check(lib.cp_wallish_tail(dst._handle, splice._handle, coef.data_ptr(), rows.data_ptr(), rows.shape[1], 3, *box_args, tophat.data_ptr(), box.data_ptr(),
                                   res.data_ptr(), stream))
    out['tail'], out['tail.boxes'], out['tail.coef'] = _host(res), _host(box.view(-1, 4)), _host(coef)
    args, ncosmo, keep = dv.pack_cosmologies(bg, pk, dev)
    assert ncosmo == 3
    work = torch.empty(int(lib.cp_dst_forward_analytic_workspace_bytes(3)), dtype=torch.uint8, device=dev)
    for label, with_coef in (('full', False), ('full_coef', True)):
        coef, box, res = torch.zeros((3, 4096), dtype=torch.float64, device=dev), torch.empty((6, 2), dtype=torch.int32, device=dev), torch.empty_like(rows)
        _lib.check(lib.cp_wallish_full(dst._handle, splice._handle, _lib.ENGINES[engine], *args(), rows.data_ptr(), rows.shape[1], *box_args, tophat.data_ptr(),
                                       box.data_ptr(), coef.data_ptr() if with_coef else None, res.data_ptr(), work.data_ptr(), stream))
        out[label], out[label + '.boxes'] = _host(res), _host(box.view(-1, 4))
        if with_coef:
            out[label + '.coef'] = _host(coef)
    return out


def sigma_entries(engine):
    from cosmoprimo_amd import interpolator as itp
    dev, out = _device(), {}
    bg, pk = cosmologies(47)
    rng = np.random.default_rng(48)
    saved = itp._SIGMA_RZ_PREFILTERED
    try:
        for route, prefiltered in (('band', False), ('prefiltered', True)):
            itp._SIGMA_RZ_PREFILTERED = prefiltered
            for nz in (2, 3):
                growth_sq = _up(rng.uniform(0.3, 1., (3, nz)))
                for keep in (False, True):
                    sigma, spectra, _ = itp.sigma_rz_analytic(engine, bg, pk, RADII, growth_sq, dev, keep_spectra=keep)
                    tag = '%s.nz%d.%s' % (route, nz, 'pk' if keep else 'nopk')
                    out[tag] = _host(sigma).reshape(3, -1)
                    if keep:
                        out[tag + '.spectra'] = _host(spectra)
    finally:
        itp._SIGMA_RZ_PREFILTERED = saved
    return out


def tabulated_rows(nrows, seed):
    rng = np.random.default_rng(seed)
    return _up(rng.uniform(0.5, 2., (nrows, 1)) * (K / 0.05)**rng.uniform(-2.2, -1.8, (nrows, 1)) * 1e4)


def spline_entries():
    import torch
    import cosmoprimo_amd as cp
    from cosmoprimo_amd import _lib, _device as dv
    from cosmoprimo_amd.spline import LinearOperator
    lib, dev, out = _lib.load(), _device(), {}
    fft = cp.TophatVariance(K, device=dev)
    radii = np.geomspace(0.7, 150., 40)
    radii[0], radii[-1] = 1e-5, 1e9      # outside the output grid of the transform
    op = LinearOperator.spline(fft.y[0], radii, bc='natural', device=dev)
    plan = fft._get_plan(dev)
    assert lib.cp_sigma_rz_fused_available(plan.handle, op._handle) == 1
    rows = tabulated_rows(3, 3)
    for post in (0, 1):
        res = torch.empty((3, radii.size), dtype=torch.float64, device=dev)
        _lib.check(lib.cp_fftlog_spline_execute(plan.handle, op._handle, rows.data_ptr(), res.data_ptr(), 3, post, dv.stream_of(dev)))
        out['root%d' % post] = _host(res)
    return out


def geospline_entries():
    import cosmoprimo_amd as cp
    from cosmoprimo_amd import interpolator as itp
    dev, out = _device(), {}
    fft = cp.TophatVariance(K, device=dev)
    s = fft.y[0]
    radii = np.geomspace(0.7, 150., 40)
    radii[0], radii[-1] = 1e-5, 1e9
    plain, grouped = tabulated_rows(3, 5), tabulated_rows(4, 6).reshape(2, 2, 1024)
    saved = itp._GEOSPLINE_PREFILTERED
    try:
        for route, prefiltered in (('solved', False), ('prefiltered', True)):
            itp._GEOSPLINE_PREFILTERED = prefiltered
            for sqrt in (False, True):
                for label, rows, group in (('plain', plain, 0), ('grouped', grouped, 2)):
                    got = itp._fftlog_then_geospline(fft, s, radii, rows, dev, sqrt=sqrt, group=group)
                    assert got is not None
                    plans = [v for key, v in itp._op_cache.items() if key[0] == 'geospline' and key[2] == prefiltered and key[4] == radii.tobytes()]
                    assert plans and all(plan.prefiltered == prefiltered for plan in plans)
                    out['%s.%s.root%d' % (route, label, sqrt)] = _host(got).reshape(-1, got.shape[-1])
    finally:
        itp._GEOSPLINE_PREFILTERED = saved
    return out


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


@pytest.fixture(scope='module')
def wallish():
    return wallish_filter()


@pytest.mark.parametrize('n', DST_SIZES)
def test_dst_execute(recorded, n):
    assert_equal_rows(dst_entries(n), recorded, 'dst%d' % n)


def test_rfft(recorded):
    assert_equal_rows(rfft_entries(), recorded, 'rfft')


@pytest.mark.parametrize('engine', ENGINES)
def test_analytic_entries(recorded, wallish, engine):
    assert_equal_rows(analytic_entries(engine, wallish), recorded, 'analytic.' + engine)


@pytest.mark.parametrize('engine', ENGINES)
def test_sigma_rz_analytic(recorded, engine):
    assert_equal_rows(sigma_entries(engine), recorded, 'sigma.' + engine)


def test_fftlog_spline(recorded):
    assert_equal_rows(spline_entries(), recorded, 'spline')


def test_fftlog_geospline(recorded):
    assert_equal_rows(geospline_entries(), recorded, 'geospline')
