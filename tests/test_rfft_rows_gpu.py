"""GPU: the real FFTs of rows (cp_rfft_forward / cp_rfft_backward, csrc/cp_rfft.hip) against an extended-precision truth, with more rows than
workgroups: the kernel walks ``row += gridDim.x`` and reuses its LDS from one row to the next behind one barrier, which no other test makes it do.

Truth and rows: tests/transform_truth.py (longdouble radix-2 FFT of seven base rows per size; row i of a batch is base row i % 7 times 2^e_i,
e_i in [-300, 300], and so is its truth -- batch and expected values are formed on the device).
Bound: the project's own for these kernels (tests/test_fftlog_gpu.py, test_engine_forward_backward_are_real_ffts), per row
    |got - truth|.max() < 16e-16 log2(size) |truth|.max().
A row that holds a NaN or an infinity comes out as NaN, every number of it, and no other row notices -- on whichever trip of whichever workgroup.

Measured on an MI355X, largest fraction of that bound over all rows and row counts (the same on every trip):
    size                       8      16     32     64     128    256    512    1024   2048   4096   8192   16384
    forward                    0.027  0.036  0.024  0.024  0.017  0.021  0.019  0.017  0.019  0.015  0.014  0.016
    backward                   0.034  0.033  0.035  0.024  0.021  0.029  0.020  0.019  0.019  0.026  0.028  0.020
    backward, conj_input = 0   0.034  0.034  0.025  0.026  0.022  0.020  0.017  0.020  0.017  0.022  0.019  0.020
That leaves more than a factor of 8, so the tests ask for LIMIT = 4 x the worst of them, 0.0356: 2.3e-16 log2(size) |truth|.max() -- room for another order
of the instructions under another compiler or clock, none for an error of the kind the tests look for.
"""
import ctypes
import functools

import numpy as np
import pytest

import transform_truth as tt

pytestmark = pytest.mark.gpu

G = 2048      # the grid cap of rfft_run: ``const int grid = (int)(nrows < 2048 ? nrows : 2048);`` (csrc/cp_rfft.hip)
SIZES = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]      # the twelve instantiations (CP_RFFT_SIZES)


def row_counts(size):
    """G: one trip per workgroup; G + 1: workgroup 0 makes two; 2 G + 3: three trips, ragged end (sizes up to 2048: buffers below 300 MB)."""
    return [G, G + 1] + ([2 * G + 3] if size <= 2048 else [])


CASES = [(size, nrows) for size in SIZES for nrows in row_counts(size)]


LIMIT = 4 * 0.0356      # of the bound, see above


def bound(size):
    return 16e-16 * np.log2(size)


@functools.lru_cache(maxsize=None)
def truths(size):
    """The seven base rows of both directions and their truths as (hi, lo) pairs of doubles, on the device; computed once per size."""
    import torch
    x, z = tt.base_rows(size, 'real'), tt.base_rows(size, 'spectrum')

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')

    return {'x': dev(x), 'z': dev(z), 'forward': tuple(map(dev, tt.split_double(tt.rfft_truth(x)))),
            'backward': tuple(map(dev, tt.split_double(tt.irfft_truth(z.conj(), size)))),      # the engine's convention: irfft(conj(.))
            'backward_plain': tuple(map(dev, tt.split_double(tt.irfft_truth(z, size))))}


def fractions(got, truth, nrows, size):
    """Per row, the fraction of the bound that |got - truth|.max() takes; truth = hi + lo, scaled as the rows were."""
    hi, lo = (tt.batch(part, nrows) for part in truth)
    assert got.shape == hi.shape and got.dtype == hi.dtype
    error = ((got - hi) - lo).abs().amax(dim=1)
    return (error / (bound(size) * hi.abs().amax(dim=1))).cpu().numpy()


def check_rows(name, got, truth, nrows, size, bad=()):
    """Rows ``bad`` hold nothing but NaN, every other row meets the bound (and is therefore finite)."""
    import torch
    numbers = torch.view_as_real(got) if got.is_complex() else got
    nan_rows = torch.isnan(numbers.reshape(nrows, -1)).all(dim=1).cpu().numpy()
    frac = fractions(got, truth, nrows, size)
    good = np.ones(nrows, dtype=bool)
    good[list(bad)] = False
    assert good.sum() == nrows - len(bad)
    worst = float(np.nanmax(np.where(good, frac, 0.)))
    print('rfft %s size %d rows %d: %.3g of the bound (row %d)' % (name, size, nrows, worst, int(np.nanargmax(np.where(good, frac, 0.)))))
    for i in bad:
        missing = int((~torch.isnan(numbers[i])).sum())
        assert nan_rows[i], '%s size %d: row %d holds %d numbers that are not NaN: %s' % (name, size, i, missing, numbers[i].flatten()[:6].tolist())
    assert np.flatnonzero(nan_rows).tolist() == sorted(bad)
    failing = np.flatnonzero(good & ~(frac < LIMIT))
    assert failing.size == 0, '%s size %d: rows %s (workgroups %s, trips %s) at %s of the bound' % (
        name, size, failing[:8].tolist(), (failing[:8] % G).tolist(), (failing[:8] // G).tolist(), frac[failing[:8]].tolist())
    return worst


@pytest.mark.parametrize('size,nrows', CASES, ids=['%d-%d' % case for case in CASES])
def test_rows_against_truth(size, nrows):
    """Forward and backward through ``NumpyFFTEngine`` with device tensors.  Beyond G rows: a NaN in row 5 (trip 0 of workgroup 5) and an infinity in row
    G (trip 1 of workgroup 0) stay where they are -- rows 0 and 5 + G, which the same workgroups transform on their other trips, among the rest."""
    import torch
    from cosmoprimo_amd.fftlog import NumpyFFTEngine
    engine, t = NumpyFFTEngine(size), truths(size)
    bad = (5, G) if nrows > G else ()
    x = tt.batch(t['x'], nrows)
    if bad:
        x[5, 3] = float('nan')
        x[G, 2] = float('inf')
    spectrum = engine.forward(x)
    assert spectrum.is_cuda and spectrum.dtype == torch.complex128 and spectrum.shape == (nrows, size // 2 + 1)
    check_rows('forward', spectrum, t['forward'], nrows, size, bad)
    ends = spectrum[:, [0, -1]].imag      # DC and Nyquist of a real row are real: exact zeros
    assert bool((ends[[i for i in range(nrows) if i not in bad]] == 0.).all())
    del x, spectrum
    z = tt.batch(t['z'], nrows)
    if bad:
        z[5, 1] = float('nan')
        z[G, 2] = float('inf')
    back = engine.backward(z)
    assert back.is_cuda and back.dtype == torch.float64 and back.shape == (nrows, size)
    check_rows('backward', back, t['backward'], nrows, size, bad)


@pytest.mark.parametrize('size', SIZES)
def test_backward_without_the_conjugate(size):
    """cp_rfft_backward(conj_input = 0), which the engines never ask for: irfft(z) itself, G + 1 rows."""
    import torch
    from cosmoprimo_amd import _lib
    lib, t, nrows = _lib.load(), truths(size), G + 1
    z = tt.batch(t['z'], nrows)
    out = torch.empty((nrows, size), dtype=torch.float64, device=z.device)
    plan = ctypes.c_void_p()
    _lib.check(lib.cp_rfft_plan_create(ctypes.byref(plan), size, 0))
    try:
        _lib.check(lib.cp_rfft_backward(plan, z.data_ptr(), out.data_ptr(), nrows, 0, torch.cuda.current_stream(z.device).cuda_stream))
        torch.cuda.synchronize()
    finally:
        lib.cp_rfft_plan_destroy(plan)
    check_rows('backward, conj_input = 0,', out, t['backward_plain'], nrows, size)


def test_argument_checks():
    """What tests/test_lib_abi.py does not ask of these entry points: a transform in place is refused, no rows is a success that looks at no pointer,
    a size that is no power of two from 8 to 16384 gets no plan."""
    import torch
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    plan = ctypes.c_void_p()
    for size in (0, -8, 4, 12, 100, 16383, 32768):
        assert lib.cp_rfft_plan_create(ctypes.byref(plan), size, 0) == _lib.CP_EUNSUPPORTED and not plan.value and b'cp_rfft_plan_create' in lib.cp_last_error()
    _lib.check(lib.cp_rfft_plan_create(ctypes.byref(plan), 64, 0))
    try:
        buffer = torch.full((2, 66), -7.25, dtype=torch.float64, device='cuda:0')
        stream = torch.cuda.current_stream(buffer.device).cuda_stream
        assert lib.cp_rfft_forward(plan, buffer.data_ptr(), buffer.data_ptr(), 1, stream) == _lib.CP_EINVAL and b'in place' in lib.cp_last_error()
        assert lib.cp_rfft_backward(plan, buffer.data_ptr(), buffer.data_ptr(), 1, 1, stream) == _lib.CP_EINVAL and b'in place' in lib.cp_last_error()
        assert lib.cp_rfft_forward(plan, None, None, 0, None) == _lib.CP_OK and lib.cp_rfft_backward(plan, None, None, 0, 1, None) == _lib.CP_OK
        torch.cuda.synchronize()
        assert bool((buffer == -7.25).all())
    finally:
        lib.cp_rfft_plan_destroy(plan)
