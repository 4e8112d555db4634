"""
Extended-precision truth of brieden2022's re-sampling kernel ``brieden_resample_kernel<S, PEAKS, OPLDS>`` (csrc/cp_bao.hip) behind both of its entry
points, ``cp_brieden_resample`` and ``cp_brieden_smooth``, with the cases that tests/test_brieden_edges_gpu.py feeds it.  numpy only.

Truth: the samples formed in ``np.longdouble`` (cp_brieden_resample: envelope x pknow x ratio_now_fid; cp_brieden_smooth: ratio_p = P_peak /
(now[peak_p] g0 corr[peak_p]) / ratio_fid[peak_p], envelope_j = sum_p op[p, j] ratio_p, sample_j = envelope_j now_j g0 corr_j ratio_now_fid_j), their
log10 on the knots log10(k_fid / rescale), the four knots of ``_pad_log`` (tests/test_brieden_host.pad_knots, in longdouble) and the natural spline
of tests/spline_truth.py -- a Thomas solve for the FIRST derivatives over all n + 4 knots, no lanes, no closed forms -- evaluated at log10 k_fid.
Judged in v = log10(out): a block is a row, its scale the largest |v| of the row.

Tolerance: the rule of tests/spline_truth.py.  A row's level is the larger distance from the truth of two float64 results, floored at FLOOR:
(a) the same plain solve in float64, (b) the kernel's scheme restated in float64 (tests/test_brieden_host.second_derivatives_as_the_kernel: S knots
per lane, two recursions, the neighbours' totals, A p^i + B p^(n-1-i) in closed form; and :func:`evaluate_as_the_kernel`: the uniform-interval
and the end-interval form).  The device gets ALLOW = 16 levels; a case whose level exceeds CAP = 32 FLOOR is not used (none does: 22 at most).

Cases: n samples per cosmology at every S = 3 .. 8 with the last lane full, owning one knot or straddling the last knot (SIZES); a row i of a batch is
base row i % 7 with rescale i % 11 (RESCALE: 1 exactly -- every query on a knot --, 1 +- 1e-9, 0.85 and 1.2 -- queries in the extrapolated
intervals on either side --, six random values between), so 77 distinct rows serve a batch of any size.
"""
import functools

import numpy as np

import spline_truth as st
from test_brieden_host import KAPPA, pad_knots, second_derivatives_as_the_kernel

LD = st.LD
CAP = st.CAP
NBASE = st.NBASE
SIZES = [129, 191, 192, 193, 256, 257, 320, 321, 384, 385, 448, 449, 511, 512]
UNSUPPORTED = [128, 513]
RESCALE = np.concatenate([[1., 1. + 1e-9, 1. - 1e-9, 0.85, 1.2], np.random.default_rng(20221).uniform(0.85, 1.2, 6)])
NRESCALE = RESCALE.size
NUNIQUE = NBASE * NRESCALE
KMIN, KMAX = 1e-7, 1e2
# extrapolation bounds INSIDE the k_fid range: min(kmin, k_fid[0] / r (1 - 1e-9)) and max(kmax, ...) take their second argument.  The knots must not move
# beyond the queries then (the outermost knot is the end of the spline): rescale >= 1 where kmin is reached (first = 0), <= 1 where kmax is (first = nk - n)
TIGHT = (2e-5, 40.)
# The outermost knot then lies 4.3e-10 from the first (last) sample, the next one 3.9e-10: intervals known to 1e-6 of themselves in float64.  The plain
# float64 solve (scipy's too) takes the slope towards them from rounded values and is off by 1e3 to 7e5 FLOOR at queries inside an interval for rescales
# of 0.85 to 1.2 (the kernel's closed form, whose right-hand sides there are zero by construction, by 2 to 300); such rows are over the cap.  Rescales
# within 1e-8 of 1 keep the queries within 1e-6 of an interval from a knot, where the second derivatives weigh that much less, and the level under it
# (at 3e-7 the plain solve is still 200 to 900 FLOOR away)
TIGHT_OFFSETS = np.array([0., 1e-9, 3e-9, 1e-8])
FIRSTS = ('zero', 'middle', 'end')      # first = 0, 137, nk - n
BATCHES = [1, 3, 4, 5, 11, 12, 13]      # and 12 x CUs + 5: more cosmologies than one launch has waves (OPLDS: 12 waves on each CU; otherwise 4 x 3 per CU)
NB = 13
# (n, np): cp_brieden_smooth.  np odd and even, 1 and 64; every S; (341, 31 | 32) either side of the OPLDS threshold, restated in :func:`oplds`
SMOOTH = [(257, 1), (256, 2), (512, 23), (385, 24), (449, 63), (129, 64), (341, 31), (341, 32), (341, 33), (191, 5)]
BENT = [257, 385]      # S = 5 and S = 7


def samples_per_lane(n):
    return (n + 63) // 64


def last_lane(n):
    """How the last lane that owns knots holds them: 'full' (S knots), 'one' (knot n - 1 alone) or 'straddle' (2 .. S - 1 knots, the rest beyond n - 1)."""
    rem = n % samples_per_lane(n)
    return 'full' if rem == 0 else ('one' if rem == 1 else 'straddle')


def oplds(n, npk):
    """Whether ``launch_resample`` keeps the operator's columns in LDS (the 768-thread form), and the LDS bytes it asks for."""
    shared, per_wave, op = 3 * n * 8, 2 * (n + 8) * 8, npk * n * 8
    fits = 12 * per_wave + shared + op + 2048 <= 160 * 1024
    return fits, (12 * per_wave + shared + op if fits else 4 * per_wave + shared)


def grid(n, first):
    """(k, first, k_fid, log10 k_fid as the device is given it): n + 300 wavenumbers, the k_fid range at ``first`` = 'zero' | 'middle' | 'end'."""
    nk = n + 300
    first = {'zero': 0, 'middle': 137, 'end': nk - n}[first]
    k = np.geomspace(1e-5, 50., nk)
    k_fid = k[first:first + n].copy()
    return k, first, k_fid, np.log10(k_fid)


def rows_of(nb):
    """(base row, rescale, distinct row) of each row of a batch."""
    i = np.arange(nb)
    return i % NBASE, i % NRESCALE, (i % NBASE) * NRESCALE + (i % NRESCALE)


def rest_of_the_rows(nb, nk):
    return np.random.default_rng(7 * nb + nk).uniform(1., 2., (nb, nk))


# ---- the kernel's evaluation, in float64 ---------------------------------------------------------------------------------------------------------

def evaluate_as_the_kernel(x, X, Y, M, xq):
    """The kernel's two forms at the queries: on the uniform stretch x[0] + i h by the fraction of the interval and M in units of 6 kappa / h^2, in the
    four end intervals by their own ends and (length / h)^2.  M: (n + 4) in those units."""
    n = x.size
    x_first, x_last = x[0], x[-1]
    h = (x_last - x_first) / (n - 1)
    inv_h = 1. / h
    xa, xb, xc, xd = X[0], X[1], X[-2], X[-1]
    u = (xq - x_first) * inv_h
    fi = np.floor(u)
    inner = (xq >= x_first) & (fi < n - 1)
    j = np.where(inner, 2 + fi, 0).astype(int)
    b = u - fi
    a = 1. - b
    v_inner = a * Y[j] + b * Y[j + 1] + KAPPA * ((a * a * a - a) * M[j] + (b * b * b - b) * M[j + 1])
    j = np.where(xq < x_first, np.where(xq >= xb, 1, 0), np.where(xq < xc, n + 1, n + 2))
    xl = np.where(j == 1, xb, np.where(j == 0, xa, np.where(j == n + 1, x_last, xc)))
    hh = np.where(j == 1, x_first - xb, np.where(j == 0, xb - xa, np.where(j == n + 1, xc - x_last, xd - xc)))
    b = (xq - xl) / hh
    a = 1. - b
    ratio = hh * inv_h
    v_end = a * Y[j] + b * Y[j + 1] + KAPPA * (ratio * ratio) * ((a * a * a - a) * M[j] + (b * b * b - b) * M[j + 1])
    v = np.where(inner, v_inner, v_end)
    return np.where((xq >= xa) & (xq <= xd), v, np.nan)


def _three_results(samples_ld, samples_f8, samples_kernel, k_fid, log_k_fid, rescale, kmin, kmax, mistake=None):
    """(truth, plain float64, the scheme in float64), each (rows, n) in v = log10 P at log10 k_fid; row u has rescale[u]."""
    truth, plain, scheme = [], [], []
    for u, r in enumerate(rescale):
        if mistake is None:
            for samples, dtype, out in ((samples_ld[u], LD, truth), (samples_f8[u], 'f8', plain)):
                x = np.log10(k_fid.astype(dtype) / dtype(r) if dtype is LD else k_fid / r)
                X, Y = pad_knots(x, np.log10(samples), kmin, kmax)
                X, Y = np.asarray(X, dtype=dtype), np.asarray(Y, dtype=dtype)
                out.append(st.spline(X, Y[None, :], log_k_fid, 'natural', dtype=dtype)[0])
        x = log_k_fid - np.log10(r)      # the kernel: the first and last of these and n - 1 equal steps between them
        y = np.log10(samples_kernel[u])
        X, Y = pad_knots(x, y, kmin, kmax)
        M = second_derivatives_as_the_kernel(x, y, X, mistake=mistake, scaled=False)
        scheme.append(evaluate_as_the_kernel(x, X, Y, M, log_k_fid))
    if mistake is not None:
        return np.array(scheme)
    return np.array(truth), np.array(plain), np.array(scheme)


def worse(truth, plain, scheme):
    """Row by row the float64 result that lies further from the truth: what :func:`spline_truth.levels` takes the level from."""
    dist = [np.abs(np.asarray(f).astype(LD) - truth).max(axis=-1) for f in (plain, scheme)]
    return np.where((dist[1] > dist[0])[:, None], scheme, plain)


# ---- cp_brieden_resample ---------------------------------------------------------------------------------------------------------------------------

def _smooth_spectrum(k_fid):
    return 2e4 * (k_fid / 0.02)**0.96 / (1. + (k_fid / 0.02)**2)**1.3


def _rescales(first, bounds):
    if bounds == TIGHT:
        picked = 1. + (1. if first == 'zero' else -1.) * TIGHT_OFFSETS
        return picked[np.arange(NRESCALE) % picked.size]
    return RESCALE


@functools.lru_cache(maxsize=None)
def resample_case(n, first='middle', bounds=(KMIN, KMAX)):
    """dict of one (n, first, (kmin, kmax)): the inputs of cp_brieden_resample (7 base rows, 11 rescales) and truth / float64 of the 77 distinct rows."""
    k, first_index, k_fid, log_k_fid = grid(n, first)
    rng = np.random.default_rng(1009 * n + FIRSTS.index(first))
    pknow = _smooth_spectrum(k_fid)[None, :] * rng.uniform(0.5, 2., (NBASE, 1))
    envelope = 1. + 0.05 * np.sin(k_fid[None, :] * rng.uniform(80., 120., (NBASE, 1))) * np.exp(-(k_fid / 0.3)**2)
    ratio_now_fid = 1. + 0.01 * np.cos(np.log(k_fid))
    rescale = _rescales(first, bounds)
    base, which = np.divmod(np.arange(NUNIQUE), NRESCALE)
    ld = (envelope.astype(LD) * pknow.astype(LD) * ratio_now_fid.astype(LD))[base]
    f8 = (envelope * pknow * ratio_now_fid)[base]
    case = dict(n=n, nk=k.size, first=first_index, k_fid=k_fid, log_k_fid=log_k_fid, envelope=envelope, pknow=pknow, ratio_now_fid=ratio_now_fid, rescale=rescale,
                bounds=bounds, samples=f8, samples_kernel=f8, row_rescale=rescale[which])
    case['truth'], case['plain'], case['scheme'] = _three_results(ld, f8, f8, k_fid, log_k_fid, rescale[which], *bounds)
    case['f8'] = worse(case['truth'], case['plain'], case['scheme'])
    return case


def mistaken(case, mistake):
    """The scheme's float64 result with one of the mistakes of test_brieden_host.second_derivatives_as_the_kernel made in it (CPU only)."""
    return _three_results(None, None, case['samples_kernel'], case['k_fid'], case['log_k_fid'], case['row_rescale'], *case['bounds'], mistake=mistake)


# ---- cp_brieden_smooth -----------------------------------------------------------------------------------------------------------------------------

def hats(n, peaks):
    """(np, n): non-negative hat functions centred on the extrema, summing to 1 over p at every sample (one extremum: ones)."""
    if len(peaks) == 1:
        return np.ones((1, n))
    return np.stack([np.interp(np.arange(n), peaks, np.eye(len(peaks))[p]) for p in range(len(peaks))])


@functools.lru_cache(maxsize=None)
def smooth_case(n, npk, first='middle'):
    """dict of one (n, np): the inputs of cp_brieden_smooth and truth / float64 of the 77 distinct rows.  The extrema include knot 0 and, from two on,
    knot n - 1."""
    k, first_index, k_fid, log_k_fid = grid(n, first)
    rng = np.random.default_rng(2003 * n + npk)
    peaks = np.array([0] if npk == 1 else sorted([0, n - 1] + list(rng.choice(np.arange(1, n - 1), npk - 2, replace=False))), dtype='i4')
    op = hats(n, peaks)
    now = _smooth_spectrum(k_fid)[None, :] * rng.uniform(0.5, 2., (NBASE, 1))
    g0 = rng.uniform(0.5, 1., NBASE)
    correction = 1. + 0.02 * np.sin(np.log(k_fid))
    ratio_fid = 1. + 0.03 * np.cos(3. * np.log(k_fid))
    ratio_now_fid = 1. + 0.01 * np.cos(np.log(k_fid))
    pk_peaks = now[:, peaks] * g0[:, None] * correction[peaks] * ratio_fid[peaks] * (1. + 0.05 * rng.uniform(-1., 1., (NBASE, npk)))
    base, which = np.divmod(np.arange(NUNIQUE), NRESCALE)

    def samples(dtype):
        t = lambda a: a.astype(dtype)      # noqa: E731
        ratio = t(pk_peaks) / (t(now)[:, peaks] * t(g0)[:, None] * t(correction)[peaks]) / t(ratio_fid)[peaks]
        envelope = ratio @ t(op)
        return envelope * t(now) * t(g0)[:, None] * t(correction) * t(ratio_now_fid)

    # the kernel: reciprocals, the columns summed in order, pknow = now x g0 x correction formed first
    ratio = pk_peaks * (1. / (now[:, peaks] * g0[:, None] * correction[peaks])) * (1. / ratio_fid[peaks])
    envelope = np.zeros((NBASE, n))
    for p in range(npk):
        envelope = op[p] * ratio[:, p:p + 1] + envelope
    kernel = envelope * (now * g0[:, None] * correction) * ratio_now_fid
    ld, f8 = samples(LD), samples('f8')
    assert (ld > 0).all() and (np.abs(op.sum(axis=0) - 1.) < 4e-16).all() and (op >= 0.).all()
    case = dict(n=n, np=npk, nk=k.size, first=first_index, k_fid=k_fid, log_k_fid=log_k_fid, pk_peaks=pk_peaks, now=now, g0=g0, correction=correction, ratio_fid=ratio_fid,
                peaks=peaks, op=op, ratio_now_fid=ratio_now_fid, rescale=RESCALE, bounds=(KMIN, KMAX), samples=f8[base], samples_kernel=kernel[base],
                row_rescale=RESCALE[which])
    case['truth'], case['plain'], case['scheme'] = _three_results(ld[base], f8[base], kernel[base], k_fid, log_k_fid, RESCALE[which], KMIN, KMAX)
    case['f8'] = worse(case['truth'], case['plain'], case['scheme'])
    return case


def assert_within(out, case, what):
    """The k_fid range of a device result (nb, nk), as v = log10 in longdouble, within the allowance of its rows; the fraction used."""
    out = np.asarray(out)
    first, n = case['first'], case['n']
    unique = rows_of(len(out))[2]
    got = np.log10(out[:, first:first + n].astype(LD))
    return st.assert_within(got, case['truth'][unique], case['f8'][unique], what=what)
