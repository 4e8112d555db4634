"""CPU: the extended-precision truth of tests/transform_truth.py, held to something independent of it before the GPU tests lean on it.

Tolerances (derived, not measured), with eps of the format that limits the comparison -- ``np.finfo(np.longdouble).eps`` between two longdouble
results (equal to double's where the platform has no wider type), double's against numpy / scipy:
  O(N^2) DFT         a sum of N products accumulated in order: N eps sum_n |x_n| (Higham, Accuracy and Stability, section 3.1), the FFT's own
                     error being of order log2 N eps; twice that is asked
  numpy.fft          (8 log2 n + 1) eps_double ||truth||_2: the FFT bound of Higham's theorem 24.2 with twiddles good to a few eps, plus the rounding
                     of the result; the maximum norm is below the 2-norm
  scipy.fftpack      the same with the log of the longest transform an implementation may take (4N) and the rotation: (8 log2 4N + 4) eps_double ||x||_2
                     (the orthonormal transform keeps the 2-norm)
  there and back     one direct sum, pairwise in blocks: (log2 N + 16) eps f sum_n |x_n| <= (log2 N + 16) eps sqrt(2) ||x||_2 per coefficient; the
                     second sum adds as much and carries the errors of the first, at most their 2-norm, sqrt(N) times the bound of one
"""
import numpy as np
import pytest
from scipy import fftpack

import transform_truth as tt

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
EPS = float(np.finfo('f8').eps)
RFFT_SIZES = [8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]
DST_SIZES = [256, 1024, 4096]


def dft_matrix(n):
    """W[j, k] = exp(-2 pi i j k / n) from longdouble cosines and sines of phases reduced in integers."""
    jk = (np.arange(n)[:, None] * np.arange(n)[None, :]) % n
    theta = (2 * tt.PI / LD(n)) * jk.astype(LD)
    W = np.empty((n, n), dtype=tt.CLD)
    W.real, W.imag = np.cos(theta), -np.sin(theta)
    return W


def norm2(a):
    return np.sqrt((np.abs(np.asarray(a, dtype='c16' if np.iscomplexobj(a) else 'f8'))**2).sum(axis=-1, keepdims=True))


@pytest.mark.parametrize('n', [8, 64, 256])
def test_fft_truth_against_the_quadratic_dft(n):
    W = dft_matrix(n)
    x = tt.base_rows(n, 'real')
    want = x.astype(tt.CLD) @ W
    got = tt.rfft_truth(x)
    assert got.dtype == tt.CLD and got.shape == (tt.NBASE, n // 2 + 1)
    tol = 2 * n * EPS_LD * np.abs(x).sum(axis=-1, keepdims=True)
    assert (np.abs(got - want[:, :n // 2 + 1]) <= tol).all()
    assert (got[:, 0].imag == 0).all() and (got[:, -1].imag == 0).all()
    z = tt.base_rows(n, 'spectrum')
    full = z.astype(tt.CLD)
    full[:, 0], full[:, -1] = full[:, 0].real, full[:, -1].real      # numpy's c2r: DC and Nyquist count as real
    full = np.concatenate([full, np.conj(full[:, 1:n // 2])[:, ::-1]], axis=-1)
    want = (full @ np.conj(W)) / LD(n)
    got = tt.irfft_truth(z, n)
    assert got.dtype == LD and got.shape == (tt.NBASE, n)
    tol = 2 * n * EPS_LD * np.abs(full).sum(axis=-1, keepdims=True) / n
    assert (np.abs(want.imag) <= tol).all() and (np.abs(got - want.real) <= tol).all()
    ignored = z.copy()
    ignored[:, 0], ignored[:, -1] = ignored[:, 0].real, ignored[:, -1].real
    assert np.array_equal(tt.irfft_truth(ignored, n), got)


@pytest.mark.parametrize('n', RFFT_SIZES)
def test_fft_truth_against_numpy(n):
    x = tt.base_rows(n, 'real')
    truth = tt.rfft_truth(x)
    assert (np.abs(np.fft.rfft(x, axis=-1) - truth) <= (8 * np.log2(n) + 1) * EPS * norm2(truth)).all()
    z = tt.base_rows(n, 'spectrum')
    truth = tt.irfft_truth(z, n)
    assert (np.abs(np.fft.irfft(z, n=n, axis=-1) - truth) <= (8 * np.log2(n) + 1) * EPS * norm2(truth)).all()
    # the conjugate that the engine's backward takes first
    assert (np.abs(np.fft.irfft(z.conj(), n=n, axis=-1) - tt.irfft_truth(z.conj(), n)) <= (8 * np.log2(n) + 1) * EPS * norm2(truth)).all()
    # there and back in longdouble
    back = tt.irfft_truth(tt.rfft_truth(x), n)
    assert (np.abs(back - x) <= 2 * (8 * np.log2(n) + 1) * EPS_LD * norm2(x)).all()


@pytest.mark.parametrize('n', DST_SIZES)
def test_dst_truth_against_scipy_and_itself(n):
    x = tt.base_rows(n, 'real')
    forward, inverse = tt.dst2_truth(x), tt.idst2_truth(x)
    assert forward.dtype == LD and inverse.dtype == LD and forward.shape == inverse.shape == x.shape
    tol = (8 * np.log2(4 * n) + 4) * EPS * norm2(x)
    assert (np.abs(fftpack.dst(x, type=2, norm='ortho', axis=-1) - forward) <= tol).all()
    assert (np.abs(fftpack.idst(x, type=2, norm='ortho', axis=-1) - inverse) <= tol).all()
    tol = 2 * (np.log2(n) + 16) * (1. + np.sqrt(n)) * EPS_LD * norm2(x)
    assert (np.abs(tt.idst2_truth(forward) - x) <= tol).all()
    assert (np.abs(tt.dst2_truth(inverse) - x) <= tol).all()


def test_rows_and_batches():
    """The seven rows are what their names say, the scaling of a batch is exact and so is the split of a truth into two doubles."""
    n = 64
    x = tt.base_rows(n, 'real')
    assert x.shape == (tt.NBASE, n) and np.flatnonzero(x[3]).tolist() == [1] and (x[4] == x[4, 0]).all() and (x[5, 0::2] == 1.).all() and (x[5, 1::2] == -1.).all()
    spectrum = np.abs(np.fft.rfft(x, axis=-1))
    assert spectrum[5, :-1].max() < 1e-12 * n and spectrum[5, -1] == n                                  # all energy in Nyquist
    assert spectrum[6].argmax() == n // 2 - 1 and np.delete(spectrum[6], n // 2 - 1).max() < 1e-12 * n      # the highest bin below it
    z = tt.base_rows(n, 'spectrum')
    assert z.shape == (tt.NBASE, n // 2 + 1) and z.dtype == np.complex128 and (z[:, [0, -1]].imag != 0.).all()
    for nrows in (7, 2049, 4099):
        e = tt.exponents(nrows)
        assert e.min() >= -300 and e.max() <= 300 and np.array_equal(e, tt.exponents(4099)[:nrows])
        rows = tt.batch(x, nrows)
        assert rows.shape == (nrows, n)
        for i in (0, 6, min(7, nrows - 1), nrows - 1):
            assert np.array_equal(rows[i], np.ldexp(x[i % 7], int(e[i]))) and np.array_equal(np.ldexp(rows[i], -int(e[i])), x[i % 7])
    assert np.array_equal(tt.batch(x, 15, scaled=False), x[np.arange(15) % 7])
    assert len(set(tt.exponents(4099).tolist())) > 500
    truth = tt.rfft_truth(x)
    hi, lo = tt.split_double(truth)
    assert hi.dtype == lo.dtype == np.complex128 and (np.abs(lo) <= EPS * np.abs(hi)).all()
    assert (np.abs((truth - hi) - lo) <= EPS_LD * np.abs(truth)).all()
    hi, lo = tt.split_double(tt.dst2_truth(tt.base_rows(256)))
    assert hi.dtype == lo.dtype == np.float64 and (np.abs(lo) <= EPS * np.abs(hi)).all()
    with pytest.raises(ValueError):
        tt.rfft_truth(np.zeros(12))
    with pytest.raises(ValueError):
        tt.irfft_truth(np.zeros(8, dtype='c16'), 8)
