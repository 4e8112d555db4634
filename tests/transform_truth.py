"""
Extended-precision truth of the two standalone row transforms -- the real FFTs of csrc/cp_rfft.hip and the orthonormal DST-II / DST-III of
csrc/cp_dst.hip -- and the rows that tests/test_rfft_rows_gpu.py and tests/test_dst_rows_gpu.py feed them.  numpy only (``batch`` also takes device
tensors, which it only indexes and multiplies).

Truth: computed at run time in ``np.longdouble`` (64-bit mantissa where the platform has one; the module also works where longdouble is double, and
the truth then carries double rounding, which tests/test_transform_truth_host.py allows for through ``np.finfo``).
  rfft_truth / irfft_truth   a recursive radix-2 FFT; the twiddles are ``np.exp`` of longdouble phases pi j / (n / 2) with j reduced in integers
  dst2_truth / idst2_truth   the direct sum  Y_k = f_k sum_n x_n sin(pi j / (2N)),  j = (k + 1)(2n + 1) mod 4N  in integers, summed in longdouble
tests/test_transform_truth_host.py holds them to an O(N^2) DFT written as a matrix product, to numpy.fft and to scipy.fftpack.

Rows: seven base rows per size (``base_rows``); a batch of any number of rows is base row ``i % 7`` times ``2**e_i`` (``batch``).  The product
with a power of two is exact and both transforms are linear, so the truth of row i is the truth of its base row times ``2**e_i``: the longdouble work
stays at seven rows per size.  Seven is coprime to the grid caps of the two launches (2048 workgroups, 512 pairs of rows), so the rows a workgroup
meets on its consecutive trips always differ.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
PI = LD(4) * np.arctan(LD(1))
NBASE = 7
EXPONENT_RANGE = 300
# e_i, drawn once: row i of every scaled batch is multiplied by 2**EXPONENTS[i]
EXPONENTS = np.random.default_rng(20240607).integers(-EXPONENT_RANGE, EXPONENT_RANGE + 1, 8192)


def _unit_roots(j, n):
    """exp(-2 pi i j / n) for integer j, in longdouble: the phase is reduced modulo n in integers before it meets pi."""
    j = np.asarray(j, dtype='i8') % n
    theta = (PI / LD(n // 2)) * j.astype(LD)
    return np.exp(theta * CLD(-1j))


def _fft(z):
    """Forward DFT (sign -) along the last axis, length a power of two: recursive radix-2 decimation in time."""
    n = z.shape[-1]
    if n == 1:
        return z
    even, odd = _fft(z[..., 0::2]), _fft(z[..., 1::2])
    odd = odd * _unit_roots(np.arange(n // 2), n)
    return np.concatenate([even + odd, even - odd], axis=-1)


def _power_of_two(n):
    if n < 2 or n & (n - 1):
        raise ValueError('length {} is not a power of two'.format(n))


def rfft_truth(x):
    """``rfft(x, axis=-1)``: (..., n) real -> (..., n // 2 + 1) complex longdouble."""
    x = np.asarray(x, dtype=LD)
    n = x.shape[-1]
    _power_of_two(n)
    return _fft(x.astype(CLD))[..., :n // 2 + 1]


def irfft_truth(z, n):
    """``irfft(z, n, axis=-1)``: (..., n // 2 + 1) complex -> (..., n) real longdouble; the imaginary parts of the DC and Nyquist bins are ignored,
    as numpy's c2r does."""
    z = np.array(z, dtype=CLD)
    _power_of_two(n)
    if z.shape[-1] != n // 2 + 1:
        raise ValueError('last dimension must be {:d}'.format(n // 2 + 1))
    z[..., 0] = z[..., 0].real
    z[..., -1] = z[..., -1].real
    full = np.concatenate([z, np.conj(z[..., 1:n // 2])[..., ::-1]], axis=-1)      # Hermitian extension
    return (np.conj(_fft(np.conj(full))).real / LD(n)).astype(LD)


def _dst_sines(n):
    """sin(pi j / (2n)) for j = 0 .. 4n - 1: every sine the direct sums need."""
    return np.sin((PI / LD(2 * n)) * np.arange(4 * n).astype(LD))


def _dst_factors(n):
    f = np.full(n, np.sqrt(LD(2) / LD(n)))
    f[-1] = np.sqrt(LD(1) / LD(n))
    return f


def _dst_sum(v, transpose, chunk=64):
    """out[..., a] = sum_b v[..., b] sin(pi (k + 1)(2 n + 1) / (2N)) with (k, n) = (a, b), or (b, a) when ``transpose``; ``chunk`` values of a at a
    time (7 rows of 4096: 30 MB of longdouble products per chunk)."""
    N = v.shape[-1]
    sines = _dst_sines(N)
    b = np.arange(N, dtype='i8')
    out = np.empty(v.shape, dtype=LD)
    for start in range(0, N, chunk):
        a = np.arange(start, min(start + chunk, N), dtype='i8')[:, None]
        j = ((b + 1) * (2 * a + 1) if transpose else (a + 1) * (2 * b + 1)) % (4 * N)
        out[..., start:start + a.size] = (v[..., None, :] * sines[j]).sum(axis=-1)
    return out


def dst2_truth(x):
    """``scipy.fftpack.dst(x, type=2, norm='ortho', axis=-1)`` in longdouble: Y_k = f_k sum_n x_n sin(pi (k + 1)(2n + 1) / (2N)),
    f_k = sqrt(2 / N), f_{N-1} = sqrt(1 / N)."""
    x = np.asarray(x, dtype=LD)
    return _dst_factors(x.shape[-1]) * _dst_sum(x, transpose=False)


def idst2_truth(y):
    """``scipy.fftpack.idst(y, type=2, norm='ortho', axis=-1)``: the transpose, x_n = sum_k f_k y_k sin(pi (k + 1)(2n + 1) / (2N))."""
    y = np.asarray(y, dtype=LD)
    return _dst_sum(y * _dst_factors(y.shape[-1]), transpose=True)


def base_rows(n, kind='real'):
    """The seven base rows of size n.
    kind 'real' (n samples): three standard-normal draws; a unit impulse at index 1 (its spectrum is the bare rot / twiddle table); a constant;
    the alternating row +1, -1, ... (for the rfft all of its energy is in the Nyquist bin, which a single thread writes); a cosine in the highest
    bin below Nyquist.
    kind 'spectrum' (n // 2 + 1 complex bins, the input of the backward real FFT): the analogous seven, with non-zero imaginary parts in the DC and
    Nyquist bins, which the transform has to ignore."""
    rng = np.random.default_rng(1000003 * n + (0 if kind == 'real' else 1))
    if kind == 'real':
        m = np.arange(n)
        rows = np.zeros((NBASE, n))
        rows[:3] = rng.standard_normal((3, n))
        rows[3, 1] = 1.
        rows[4] = 0.75
        rows[5] = 1. - 2. * (m % 2)
        rows[6] = np.cos(2. * np.pi * ((m * (n // 2 - 1)) % n) / n)
        return rows
    if kind == 'spectrum':
        nh = n // 2 + 1
        k = np.arange(nh)
        rows = np.zeros((NBASE, nh), dtype='c16')
        rows[:3] = rng.standard_normal((3, nh)) + 1j * rng.standard_normal((3, nh))
        rows[3, 1] = 1. - 0.5j
        rows[4] = 0.75 + 0.25j
        rows[5] = (1. - 2. * (k % 2)) * (1. + 0.5j)
        rows[6] = np.exp(2j * np.pi * ((k * (n // 2 - 1)) % n) / n)
        rows[3:, 0] += 0.375j       # something to ignore in DC and Nyquist of every row
        rows[3:, -1] -= 0.625j
        assert (rows[:, 0].imag != 0.).all() and (rows[:, -1].imag != 0.).all()
        return rows
    raise ValueError('unknown kind {}'.format(kind))


def split_double(truth):
    """(hi, lo) float64 (or complex128) with hi + lo = truth to ~2^-106: the expected values travel to the device without the rounding of truth to
    double being charged to the kernel."""
    truth = np.asarray(truth)
    double = 'c16' if np.iscomplexobj(truth) else 'f8'
    hi = truth.astype(double)
    return hi, (truth - hi).astype(double)


def exponents(nrows, scaled=True):
    if nrows > EXPONENTS.size:
        raise ValueError('at most {:d} rows'.format(EXPONENTS.size))
    return EXPONENTS[:nrows] if scaled else np.zeros(nrows, dtype=EXPONENTS.dtype)


def batch(base, nrows, scaled=True):
    """(nrows, ...): row i = base[i % 7] * 2**e_i (e_i = 0 when not ``scaled``).  ``base`` is a numpy array or a torch tensor -- the batch is then
    formed where the tensor lives, by one index and one multiplication; given the seven truths instead, the same call forms the expected values."""
    index = np.arange(nrows) % NBASE
    scale = np.ldexp(1., exponents(nrows, scaled))
    if isinstance(base, np.ndarray):
        return base[index] * scale[:, None]
    import torch
    index = torch.as_tensor(index, device=base.device)
    rows = base[index]
    if scaled:
        rows *= torch.as_tensor(scale, device=base.device)[:, None]
    return rows
