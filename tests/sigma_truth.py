"""
Extended-precision truth of the fused sigma kernels of csrc/cp_sigma.hip -- ``fftlog_spline_kernel`` (cp_fftlog_spline_execute: FFTLog of a pair of
rows, then a band operator out of LDS), ``fftlog_geospline_kernel<false>`` (the natural spline of the geometric output grid solved on the CU on a
stretch with a halo of 32 knots), ``fftlog_geospline_kernel<true, 4 / 8>`` (the prefiltered form: the transform delivers B-spline coefficients, a radius
is four of them times four cubic pieces) and the stores of ``sigma_rz_kernel`` -- composed of truths the tree already has: the tap transform of
tests/fftlog_taps_truth.py at n = 1024, npad = 2048 (one kernel index, zero padding, cropped output) and the natural spline of tests/spline_truth.py.
numpy only; the four cubic pieces of the prefiltered form (the host-only ABI call cp_geospline_basis) are handed in by the callers.
The kernels that form their spectra themselves (sigma_rz_kernel, sigma_functional_kernel, sigma8_normalise_kernel) are further down, with the spectra of
tests/power_truth.py and the growth factor of tests/background_truth.py: see the comment in front of :func:`rz_base`.

Transform   truth / restated of fftlog_taps_truth with five-tap u tables: a sparse circular correlation in longdouble, no FFT.  Rows: two dense base
            rows; batch item i is base row i % 2 times an exact 2**e, |e| <= 300 (even e where a root follows: the root of 4**e is exact).
Tables      'generic': pre, post of random sign and magnitude in [0.5, 1.5] (fftlog_taps_truth.tables).  'power': post_j = post_0 LAMBDA^j with the
            LAMBDA = RHO^-1.5 of the TophatVariance postfactor (what a prefiltered plan insists on, to 1e-11), pre random.  ``positive``: tap weights,
            pre and post positive and within 15 % of one, rows in [0.85, 1.15]: the cases that take the root (see ROOT below).  'spread' /
            'spread_wide' (the band operator): positive taps, pre and rows, post of random sign times 2^-e_j, e_j uniform in 0 ... 40 / 300, so that the
            output samples under a band differ in scale (see "Band").
Band        the kernel promises out[q] = sum_i wb[i, q] y[min(j0[q] + i, 1023)] for the band of the operator it is handed (plan_from_dense of
            csrc/cp_spline.hip, restated by :func:`band_of`), not a spline: W (nq, 1024) dense, random entries of both signs in [0.5, 1.5] inside a band
            and exactly zero outside, a NaN first entry for a NaN query, rows of zeros between banded rows.  Truth: the longdouble product with the
            transform's truth.  Restatement: the float64 numpy product of ``restated``.  On outputs of one scale and both signs a sum of bw entries is
            held against the largest of them and no float64 sum stays below the cap (measured: 36 to 46 floors at bw = 44, 136 at bw = 1024, and 1400 at
            bw = 1 where a tap sum cancels), so the band cases take the 'spread' tables: a few samples dominate every band whatever its width (at most
            25 floors; bw = 1024 needs 'spread_wide').  :func:`band_restated` is the same sum in the kernel's order, band by band, for the mutations.
CU solve    truth: spline_truth.spline(s, y_truth, r, 'natural') over ALL 1024 knots.  The kernel solves on the stretch [ws, ws + 64 S) and forgets what
            lies beyond like |pL|^33, pL = -2 a / (b + sqrt(b^2 - 4 a c)), a = RHO^2, b = 2 (1 + RHO), c = 1 / RHO (cp_geospline_plan_create):
            |pL| = 0.2762 at RHO = 1.02046, |pL|^33 = 3.6e-19 of the local scale, below FLOOR (tests/test_sigma_truth_host.py).  Restatement:
            :func:`cu_restated`, the two recursions per lane with their carries in float64.
Prefiltered truth: the same natural spline of the (ordinary) transform's truth.  Restatement :func:`prefiltered_restated`: u divided by
            conj(alpha / LAMBDA e^{-iw} + beta + gamma LAMBDA e^{iw}), numpy FFTs, the four cubic pieces at x = 1 - qa.

Scale of a distance: a geometric spline's value depends on knots d away like 0.27^d, and a power-law post spreads a row over 13 decades.  A query's
distance from the truth is measured against the largest |truth y| over the knots within 32 of its interval (:func:`spline_scale`), for the band operator
against the largest |truth y| inside its band (:func:`band_scale`).
Rule (spline_truth / splice_truth): the level of a block -- one (row, 64 radii); one (cosmology, radius) over redshifts for
sigma(r, z) -- is the LARGER distance from the truth of the plain float64 solve and of the float64 restatement of the scheme that runs, by that scale,
floored at FLOOR = 1.1e-16; the device is allowed ALLOW = 16 levels; NaN exactly where the truth has it; every case in use stays below CAP = 32 floors.
ROOT        (post_op = CP_SPLINE_POST_SQRT): truth is the longdouble root, distances are measured against the root of the scale, the allowance gains
            the 1e-16 that the comment over geo_sqrt states.  Cases that take the root are of one sign and their truth is at least 1/4 of its scale
            at every finite radius (asserted on the host): the root then halves relative errors.  One mixed-sign case holds NaN where the truth is
            negative; its finite values are held squared, by the linear rule.
"""
import numpy as np

import background_truth as bt
import fftlog_taps_truth as tt
import power_truth as pt
import spline_truth as st
from fftlog_taps_truth import LD, FLOOR, ALLOW, CAP

N, NPAD = 1024, 2048
OUT_LEFT = tt.widths(N, NPAD)[2]
K = np.geomspace(1e-7, 1e2, N)
RHO_LD = np.exp(np.log(LD(10)) * 9 / (N - 1))
RHO = float(RHO_LD)
S_GRID = np.asarray(np.sqrt(LD(1e-2) * LD(1e7)) * RHO_LD**(np.arange(N) - LD(N - 1) / 2), dtype='f8')      # geometric to an ulp
LAMBDA_LD = RHO_LD**LD(-1.5)
HALO, REACH_MAX, SMIN, SMAX, QMAX = 32, 9, 4, 8, 8      # GEO_HALO, GEO_REACH, GEO_SMIN, GEO_SMAX, GEO_QMAX of cp_sigma.hip
BLOCK = 64
SQRT_EXTRA = 1e-16      # cp_sigma.hip, over geo_sqrt: "relative error 1e-16"


# ---- tables and rows ---------------------------------------------------------------------------------------------------------------------------
def tables(kind='generic', positive=False, seed=0):
    """A fftlog_taps_truth.Synthetic of one kernel index at npad = 2048."""
    syn = tt.tables(NPAD, 1, seed)
    spread = {'spread': 40, 'spread_wide': 300}.get(kind)
    if positive or spread:
        shifts, weights = syn.taps[0]
        syn.taps = [(shifts, np.abs(weights))]
        syn.u = np.array([tt.u_table(NPAD, syn.taps[0])])
        syn.pre = 1. + 0.15 * (np.abs(syn.pre) - 1.) * 2.      # [0.85, 1.15]
        syn.post = 1. + 0.15 * (np.abs(syn.post) - 1.) * 2.
    if kind == 'power':
        j = np.arange(NPAD) - NPAD // 2
        syn.post = np.asarray(LAMBDA_LD**j, dtype='f8')[None, :] * (1. if positive else -1.)
    elif spread:
        rng = np.random.default_rng([seed, spread])
        syn.post = syn.post * np.ldexp(1., -rng.integers(0, spread + 1, NPAD)) * rng.choice([-1., 1.], NPAD)
    elif kind != 'generic':
        raise ValueError(kind)
    return syn


def base_rows(positive=False, seed=0):
    """(2, 1024): fftlog_taps_truth.base_rows; positive: 1 + 0.3 (|row| - 1) sign(row), in [0.85, 1.15]."""
    base = tt.base_rows(N, seed)
    return 1. + 0.15 * (np.abs(base) - 1.) * 2. * np.sign(base) if positive else base


def exponents(nbatch, root=False):
    """2**e of batch item i; even e where a root follows."""
    e = tt.EXPONENTS[np.arange(nbatch) % tt.EXPONENTS.size]
    return e - (e & 1) if root else e


def batch(base, nbatch, root=False):
    return base[np.arange(nbatch) % tt.NBASE] * np.ldexp(1., exponents(nbatch, root))[:, None]


def unscale(got, root=False, post_sqrt=False):
    """The device's (nbatch, nq) rows with the 2**e of their inputs taken out, exactly, in longdouble (2**(e / 2) behind a root)."""
    e = exponents(len(got), root)
    if post_sqrt:
        assert root
        e = e // 2
    return np.asarray(got).astype(LD) * np.ldexp(LD(1), -e)[:, None]


ROW_SCALE_SPREAD = 4      # CP_ROW_SCALE_SPREAD of csrc/cp_fftlog_body.h


def pair_factors(syn, base, exps, nan_rows=()):
    """(nbatch,) what the packing of two rows into one complex transform costs row i = base[i % 2] 2**exps[i], by the kernel's own statement
    (cp_fftlog_body.h, "Row independence"): the rows of a pair are brought to [1, 2) each only when the exponent fields of their largest tilted samples
    |a_j pre_j| differ by more than CP_ROW_SCALE_SPREAD = 4; "within the spread nothing is done: the error is at most 2^spread times the row-relative
    one" -- rounding is relative to the larger row of the pair.  The factor is that ratio, partner over row, where it exceeds one and the pair is left
    unscaled; one for a row without a partner, next to a NaN row (transformed as zeros) and in a scaled pair."""
    exps = np.asarray(exps)
    nbatch = len(exps)
    pre = np.abs(syn.pre[0][tt.widths(N, NPAD)[0]:tt.widths(N, NPAD)[0] + N])
    top = np.abs(base * pre).max(axis=-1)[np.arange(nbatch) % tt.NBASE]
    mantissa, field = np.frexp(top)
    field = field + exps
    factor = np.ones(nbatch)
    for a in range(0, nbatch - 1, 2):
        b = a + 1
        if a in nan_rows or b in nan_rows or abs(int(field[a] - field[b])) > ROW_SCALE_SPREAD:
            continue
        ratio = float(np.ldexp(top[b], int(exps[b] - exps[a])) / top[a])      # partner over row, for a
        factor[a], factor[b] = max(1., ratio), max(1., 1. / ratio)
    return factor


def packed_restated(syn, rows, u=None, keep_padding=False):
    """The transform of a pair of float64 rows as ONE complex transform of z = (a + i b) pre, unscaled: what the kernel does inside the spread.  For a real
    row irfft(conj(rfft(x) u)) = ifft(X[-k] v[k]) with v the Hermitian extension of conj(u) (real at DC and Nyquist, as irfft reads them), which is linear
    in x: the pair is ifft(Z[-k] v[k]), row a its real and row b its imaginary part."""
    in_left, in_right, out_left = tt.widths(N, NPAD)
    z = np.zeros(NPAD, dtype='c16')
    z[in_left:in_left + N] = np.asarray(rows[0], dtype='f8') + 1j * np.asarray(rows[1], dtype='f8')
    v = np.conj(syn.u[0] if u is None else u).copy()
    v[0], v[-1] = v[0].real, v[-1].real
    v = np.concatenate([v, np.conj(v[1:-1])[::-1]])
    spec = np.fft.fft(z * syn.pre[0])
    g = np.fft.ifft(spec[-np.arange(NPAD) % NPAD] * v)
    out = np.array([g.real, g.imag]) * syn.post[0]
    return out if keep_padding else out[:, out_left:out_left + N]


def transform(syn, base):
    """(truth (2, 1024) longdouble, restated (2, 1024) float64) of the base rows."""
    true = tt.truth(base, N, NPAD, syn.pre[0], syn.post[0], syn.taps[0])
    return true, tt.restated(base, N, NPAD, syn.pre[0], syn.post[0], syn.u[0])


# ---- band operator ----------------------------------------------------------------------------------------------------------------------------
def dense_weights(bands, seed=0, positive=False):
    """W (nq, 1024): ``bands`` is a list of (first knot, width), None for a NaN query, 'zero' for a row of zeros."""
    rng = np.random.default_rng([len(bands), seed, 5])
    w = np.zeros((len(bands), N))
    for q, band in enumerate(bands):
        if band is None:
            w[q] = np.nan
        elif band != 'zero':
            a, width = band
            assert 0 <= a and a + width <= N and width >= 1
            w[q, a:a + width] = rng.uniform(0.5, 1.5, width) * (1. if positive else rng.choice([-1., 1.], width))
    return w


def band_of(w):
    """plan_from_dense (csrc/cp_spline.hip) restated: (wb (bw, nq), j0 (nq,), bw), entries above 1e-18 of the row's maximum."""
    nq, n = w.shape
    j0, j1 = np.empty(nq, dtype='i4'), np.empty(nq, dtype='i4')
    for q in range(nq):
        if np.isnan(w[q, 0]):
            j0[q] = j1[q] = -1
            continue
        mx = np.abs(w[q]).max()
        if mx == 0.:
            j0[q] = j1[q] = -2
            continue
        keep = np.flatnonzero(np.abs(w[q]) > mx * 1e-18)
        j0[q], j1[q] = keep[0], keep[-1]
    bw = max(1, int((j1 - j0 + 1)[j0 >= 0].max()) if (j0 >= 0).any() else 1)
    last = -1
    for q in range(nq):
        if j0[q] >= 0:
            last = j0[q]
        elif j0[q] == -2 and last >= 0:
            j0[q] = j1[q] = last
    last = -1
    for q in range(nq - 1, -1, -1):
        if j0[q] >= 0:
            last = j0[q]
        elif j0[q] == -2:
            j0[q] = j1[q] = last if last >= 0 else 0
    wb = np.zeros((bw, nq))
    for q in range(nq):
        if j0[q] >= 0:
            m = j1[q] - j0[q] + 1
            wb[:m, q] = w[q, j0[q]:j1[q] + 1]
    return wb, j0, bw


def band_truth(w, y_true):
    """(rows, nq) longdouble: the dense product, NaN for a NaN query."""
    nanq = np.isnan(w[:, 0])
    out = np.where(nanq[:, None], 0, w).astype(LD) @ np.asarray(y_true).T
    out = out.T.copy()
    out[:, nanq] = np.nan
    return out


def band_product(w, y):
    """(rows, nq) float64: numpy's product, NaN for a NaN query."""
    nanq = np.isnan(w[:, 0])
    out = np.asarray(y, dtype='f8') @ np.where(nanq[:, None], 0, w).T
    out[:, nanq] = np.nan
    return out


def band_restated(w, y, mutation=None):
    """The band sum of spline_to_radii in float64, in its order: sum_i wb[i, q] y[min(j0[q] + i, 1023)].  Mutations (tests/test_sigma_truth_host.py):
    'shift' the band one knot up, 'last_chunk' the entries i >= 8 floor((bw - 1) / 8) dropped, 'second_query' query q + 128 of a thread answered with
    q's value, 'swap_rows' rows a and b of a pair swapped on output."""
    wb, j0, bw = band_of(w)
    y = np.asarray(y, dtype='f8')
    nq = w.shape[0]
    first = np.where(j0 < 0, 0, j0) + (1 if mutation == 'shift' else 0)
    acc = np.zeros((y.shape[0], nq))
    stop = 8 * ((bw - 1) // 8) if mutation == 'last_chunk' else bw
    for i in range(stop):
        acc = acc + wb[i][None, :] * y[:, np.minimum(first + i, N - 1)]
    acc[:, j0 < 0] = np.nan
    if mutation == 'second_query':
        q = np.arange(nq)
        second = (q % 256) >= 128
        acc[:, second] = acc[:, q[second] - 128]
    if mutation == 'swap_rows':
        acc = acc[np.arange(y.shape[0]) ^ 1]
    return acc


def band_scale(w, y_true):
    """(rows, nq): the largest |truth y| inside each query's band (1 for NaN and zero rows, whose truth is NaN / 0 exactly)."""
    wb, j0, bw = band_of(w)
    mag = np.abs(np.asarray(y_true))
    out = np.ones((mag.shape[0], w.shape[0]), dtype=LD)
    for q in range(w.shape[0]):
        nz = np.flatnonzero(np.nan_to_num(w[q]) != 0.)
        if nz.size:
            out[:, q] = mag[:, nz[0]:nz[-1] + 1].max(axis=-1)
    return out


# ---- the plans of the geometric spline, as cp_geospline_plan_create / _prefiltered form them -----------------------------------------------------
def locate(s, r):
    """(qj, qa, jmin, jmax) of locate_queries: interval (-1 outside the knots or NaN) and A = (s_j+1 - r) / h_j in float64."""
    r = np.asarray(r, dtype='f8')
    inside = (r >= s[0]) & (r <= s[-1])
    j = np.minimum(np.searchsorted(s, np.where(inside, r, s[0]), side='right') - 1, len(s) - 2)
    qa = np.where(inside, (s[j + 1] - r) / (s[j + 1] - s[j]), 0.)
    qj = np.where(inside, j, -1)
    if not inside.any():
        return qj, qa, len(s), -1
    return qj, qa, int(j[inside].min()), int(j[inside].max()) + 1


def cu_plan(s, r):
    """(ws, ne, S) of the CU solve, or None where the library refuses the radii."""
    n = len(s)
    qj, qa, jmin, jmax = locate(s, r)
    if jmax < 0:
        return None
    need = jmax - jmin + 1 + 2 * HALO
    S = max(SMIN, (need + 63) // 64)
    if S > SMAX:
        return None
    ne = 64 * S
    ws = max(jmin - HALO - (ne - need) // 2, 2)
    if ws + ne > n - 2:
        ws = n - 2 - ne
    if ws < 2 or jmin - ws < HALO or ws + ne - 1 - jmax < HALO:
        return None
    return ws, ne, S


def prefiltered_plan(s, r):
    """(ws, ne) of the prefiltered form (the kernel keeps ne + 2 coefficients per row), or None."""
    qj, qa, jmin, jmax = locate(s, r)
    if jmax < 0 or jmax - jmin + 1 + 2 > 64 * SMAX or jmin < HALO or jmax > len(s) - 1 - HALO:
        return None
    return jmin, jmax - jmin + 1


def geo_roots(rho=RHO_LD):
    """(pL, pR, kappa) in longdouble, the formulas of cp_geospline_plan_create."""
    rho = LD(rho)
    a, b, c = rho * rho, 2 * (1 + rho), 1 / rho
    disc = np.sqrt(b * b - 4 * a * c)
    pL, pR = -2 * a / (b + disc), -2 * c / (b + disc)
    return pL, pR, 1 / (a * pR + b + c * pL)


def spline_truth(s, y_true, r):
    return st.spline(s, y_true, r, 'natural')


def spline_plain(s, y, r):
    """The plain float64 solve over all knots."""
    return st.spline(s, np.asarray(y, dtype='f8'), r, 'natural', dtype='f8')


def spline_scale(s, y_true, r):
    """(rows, nq): the largest |truth y| over the knots within 32 of each radius' interval (1 where the radius is outside the knots)."""
    qj = locate(s, r)[0]
    mag = np.abs(np.asarray(y_true))
    out = np.ones((mag.shape[0], len(qj)), dtype=LD)
    for q, j in enumerate(qj):
        if j >= 0:
            out[:, q] = mag[:, max(j - HALO, 0):j + 2 + HALO].max(axis=-1)
    return out


def cu_restated(s, y, r, mutation=None):
    """The CU solve of fftlog_geospline_kernel<false> in float64: lane l owns knots [S l, S l + S) of the stretch, runs F_k = d_k + pL F_{k-1} and
    B_k = d_k + pR B_{k+1} over them from zero and takes the rest from the segment totals of REACH lanes on either side.  mutation ('carry', lane):
    that lane's first carry from the left (cL[0]) left out."""
    ws, ne, S = cu_plan(s, r)
    qj, qa, _, _ = locate(s, r)
    pL, pR, kappa = (float(v) for v in geo_roots())
    plL, plR = geo_roots()[:2]
    rho = RHO_LD
    inv_rho, rho_sq = float(1 / rho), float(rho * rho)
    reach = (HALO + S) // S
    assert reach <= REACH_MAX
    cL = [float(plL**(LD(S) * m)) for m in range(reach)]
    cR = [float(plR**(LD(S) * m)) for m in range(reach)]
    pLk = [float(plL**(k + 1)) for k in range(S)]
    pRk = [float(plR**(S - k)) for k in range(S)]
    y = np.asarray(y, dtype='f8')
    Y = y[:, ws - 1:ws + ne + 1]      # Y[:, e + 1] is knot ws + e
    d = ((Y[:, 2:] - Y[:, 1:-1]) * inv_rho - (Y[:, 1:-1] - Y[:, :-2])).reshape(-1, 64, S)
    f, g = np.empty_like(d), np.empty_like(d)
    acc = np.zeros(d.shape[:2])
    for k in range(S):
        acc = pL * acc + d[:, :, k]
        f[:, :, k] = acc
    acc = np.zeros(d.shape[:2])
    for k in range(S - 1, -1, -1):
        acc = pR * acc + d[:, :, k]
        g[:, :, k] = acc
    fl, gr = f[:, :, S - 1], g[:, :, 0]
    fin, gin = np.zeros_like(fl), np.zeros_like(gr)
    for m in range(reach):
        fl = np.concatenate([np.zeros_like(fl[:, :1]), fl[:, :-1]], axis=1)
        gr = np.concatenate([gr[:, 1:], np.zeros_like(gr[:, :1])], axis=1)
        term = cL[m] * fl
        if mutation is not None and mutation[0] == 'carry' and m == 0:
            term[:, mutation[1]] = 0.
        fin = fin + term
        gin = gin + cR[m] * gr
    Nk = np.empty_like(d)
    bnext = gin
    for k in range(S - 1, -1, -1):
        fk = pLk[k] * fin + f[:, :, k]
        Nk[:, :, k] = kappa * (pR * bnext + fk)
        bnext = pRk[k] * gin + g[:, :, k]
    Nk = Nk.reshape(-1, ne)
    e = np.where(qj < 0, ws, qj) - ws
    assert (e[qj >= 0] >= HALO).all() and (e[qj >= 0] + 1 <= ne - HALO).all()
    a = qa
    b = 1. - a
    v = a * Y[:, e + 1] + b * Y[:, e + 2] + ((a * a * a - a) * (rho_sq * Nk[:, e]) + (b * b * b - b) * Nk[:, e + 1])
    v[:, qj < 0] = np.nan
    return v


def prefiltered_u(u, basis):
    """The u of a prefiltered plan: u / conj(alpha / LAMBDA e^{-iw} + beta + gamma LAMBDA e^{iw}); basis (4, 4) from cp_geospline_basis(RHO)."""
    lam = float(LAMBDA_LD)
    alpha, beta, gamma = basis[0][0] / lam, basis[1][0], basis[2][0] * lam
    w = 2. * np.pi * np.arange(NPAD // 2 + 1) / NPAD
    return u / np.conj(alpha * np.exp(-1j * w) + beta + gamma * np.exp(1j * w))


def prefiltered_restated(syn, base, s, r, basis, mutation=None):
    """The prefiltered scheme in float64: numpy FFTs with the divided u give the coefficients on the padded grid; a radius in [s_j, s_j+1] is
    c_{j-1} ... c_{j+2} times the four cubic pieces at x = 1 - qa.  mutation: ('interval', q) that radius' interval one too high, 'x' the pieces taken
    at qa."""
    c = tt.restated(base, N, NPAD, syn.pre[0], syn.post[0], prefiltered_u(syn.u[0], basis), keep_padding=True)
    return prefiltered_tail(c, s, r, basis, mutation)


def prefiltered_tail(c, s, r, basis, mutation=None):
    """The four cubic pieces on the coefficients c (rows, 2048) of the padded grid."""
    qj, qa, _, _ = locate(s, r)
    j = np.where(qj < 0, HALO, qj).copy()
    if mutation is not None and mutation[0] == 'interval':
        j[mutation[1]] += 1
    x = qa if mutation == 'x' else 1. - qa
    v = np.zeros((c.shape[0], len(qj)))
    for i in range(4):
        wgt = ((basis[i][3] * x + basis[i][2]) * x + basis[i][1]) * x + basis[i][0]
        v = v + wgt * c[:, OUT_LEFT + j - 1 + i]
    v[:, qj < 0] = np.nan
    return v


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------------
def relative(values, true, scale, post_sqrt=False):
    """(rows, nq) float64: |values - truth| / scale, 0 where the truth is NaN; NaN must agree.  post_sqrt: the truth given is that of the argument,
    the values are roots: the longdouble root of both truth and scale."""
    values, true, scale = np.asarray(values).astype(LD), np.asarray(true), np.asarray(scale)
    if post_sqrt:
        with np.errstate(invalid='ignore'):
            true, scale = np.sqrt(true), np.sqrt(scale)
    nan = np.isnan(true)
    assert values.shape == true.shape, (values.shape, true.shape)
    assert np.array_equal(np.isnan(values), nan), 'NaN in other places than the truth has them'
    return np.asarray(np.where(nan, 0, np.abs(values - true)) / scale, dtype='f8')


def blocks(rel, block=BLOCK):
    """(rows, ceil(nq / block)): the largest entry of every block of ``block`` radii."""
    rows, nq = rel.shape
    nb = -(-nq // block)
    padded = np.zeros((rows, nb * block))
    padded[:, :nq] = rel
    return padded.reshape(rows, nb, block).max(axis=-1)


def levels(true, scale, restatements, post_sqrt=False, block=BLOCK):
    """(rows, nblocks): per block the larger distance of the restatements from the truth, floored at FLOOR."""
    level = FLOOR
    for f64 in restatements:
        with np.errstate(invalid='ignore'):
            level = np.maximum(level, blocks(relative(np.sqrt(f64) if post_sqrt else f64, true, scale, post_sqrt), block))
    return level


def fraction(got, true, scale, level, post_sqrt=False, extra=0., block=BLOCK, what='', widen=None):
    """The largest fraction of the allowance ALLOW x level (x widen) + extra that a block of ``got`` uses; printed and returned.  got, true, scale:
    (rows, nq); level (rows, nblocks) or (base rows, nblocks) with row i belonging to base row i % 2; widen (rows,): :func:`pair_factors`."""
    rel = blocks(relative(got, true, scale, post_sqrt), block)
    if level.shape[0] != rel.shape[0]:
        level = level[np.arange(rel.shape[0]) % level.shape[0]]
    if widen is not None:
        level = level * np.asarray(widen, dtype='f8')[:, None]
    used = rel / (ALLOW * level + extra)
    worst = float(used.max()) if used.size else 0.
    at = np.unravel_index(int(np.argmax(used)), used.shape) if used.size else (0, 0)
    print('%s: largest fraction of the allowance %.3g in row %d, block %d (level at most %.3g FLOOR)' % (what, worst, at[0], at[1], float(level.max() / FLOOR)))
    return worst


def tile(a, nbatch):
    """Row i of the batch belongs to base row i % 2."""
    return np.asarray(a)[np.arange(nbatch) % tt.NBASE]


# ---- the stores of sigma_rz_kernel ---------------------------------------------------------------------------------------------------------------
def store_rows(vr, gr, mutation=None):
    """out (nq x nz) = vr[q] gr[z] as the 128 threads of store_rows write it: 16-byte stores of (z, z + 1) with the thread's two growth factors fixed when
    nz divides the stride of 256, the same with a walking (q, z) for other even nz, 8-byte stores for odd nz.  Elements nobody writes stay NaN.
    mutation: 'dz0' the first path for every even nz, 'transpose' out[z, q]."""
    nq, nz = len(vr), len(gr)
    block = nq * nz
    out = np.full(block, np.nan)
    even = nz % 2 == 0
    T = 128
    stride = 2 * T if even else T
    for t in range(T):
        e0 = 2 * t if even else t
        dq, dz = stride // nz, stride % nz
        q, z = e0 // nz, e0 % nz
        fixed = even and (dz == 0 or mutation == 'dz0')
        z0 = z
        for e in range(e0, block, stride):
            if fixed:
                out[e], out[e + 1] = vr[q] * gr[z0], vr[q] * gr[z0 + 1]
                q += dq
                continue
            out[e] = vr[q] * gr[z]
            if even:
                out[e + 1] = vr[q] * gr[z + 1]
            q += dq
            z += dz
            if z >= nz:
                z -= nz
                q += 1
    if mutation == 'transpose':      # written as (nz, nq), read as (nq, nz)
        out = np.ascontiguousarray(out.reshape(nq, nz).T).ravel()
    return out.reshape(nq, nz)


# ---- the shipped lists (tests/test_sigma_truth_host.py holds every one below CAP before it goes to the device) ------------------------------------
def s_between(j, x):
    """A radius at position x in [0, 1) of interval j of S_GRID."""
    return S_GRID[j] + x * (S_GRID[j + 1] - S_GRID[j])


def radii(nq, jlo, jhi, seed=0, outside=True, on_knots=True):
    """nq radii in the intervals jlo ... jhi - 1 (both reached: jmin = jlo, jmax = jhi), unsorted, with repeats, radii exactly on the knots jlo and
    jhi - 1 and -- from 8 radii on -- a radius outside the grid (or NaN) in every block of 64."""
    rng = np.random.default_rng([nq, jlo, jhi, seed])
    j = rng.integers(jlo, jhi, nq)
    r = s_between(j, rng.uniform(0., 1., nq))
    if nq >= 2:
        r[-1] = s_between(jhi - 1, 0.999)
    r[0] = s_between(jlo, 0.001)
    if nq >= 8:
        if on_knots:
            r[1], r[2] = S_GRID[jlo], S_GRID[jhi - 1]
            r[3] = r[4]
        r[5] = s_between(jhi - 1, 0.5)
        if outside:
            for b in range(0, nq, BLOCK):
                at = min(b + 6 + (b // BLOCK) % 50, nq - 1)
                r[at] = [S_GRID[0] / 2., S_GRID[-1] * 3., np.nan][(b // BLOCK) % 3]
    return r


BAND_WIDTHS = [1, 7, 8, 9, 16, 17, 44, 1024]
BAND_NQ = [1, 127, 128, 129, 255, 256, 257, 513]


def band_layout(nq, bw, seed=0, hi=N, lo=0):
    """The bands of a (nq, bw) case: the first band starts on knot 0, the last ends on knot 1023, one band lies at 1024 - ceil(bw / 2) so that, padded to
    the common width, it reaches beyond knot 1023 (a narrower band there); a NaN query and a row of zeros in the first and the last position and in
    both slots of a thread (q and q + 128) where nq has room."""
    rng = np.random.default_rng([nq, bw, seed, 9])
    bands = [(int(a), bw) for a in rng.integers(lo, hi - bw + 1, nq)]
    bands[0] = (lo, bw)
    bands[-1] = (hi - bw, bw)
    if nq >= 16:
        narrow = (bw + 1) // 2
        bands[7] = (hi - narrow, narrow)
        bands[1], bands[-2] = None, None
        bands[2], bands[-3] = 'zero', 'zero'
        bands[0], bands[3] = 'zero', (lo, bw)
        bands[-1], bands[-4] = None, (hi - bw, bw)
    if nq >= 160:
        bands[5], bands[5 + 128] = None, None
        bands[9], bands[9 + 128] = 'zero', 'zero'
    return bands


def band_cases():
    """(name, nq, bw, tables kind, positive, post_sqrt)."""
    cases = [('nq%d_bw44' % nq, nq, 44, 'spread', False, False) for nq in BAND_NQ]
    cases += [('nq257_bw%d' % bw, 257, bw, 'spread_wide' if bw == 1024 else 'spread', False, False) for bw in BAND_WIDTHS if bw != 44]
    cases += [('root_nq257_bw%d' % bw, 257, bw, 'generic', True, True) for bw in (9, 44)]
    return cases


# spans of intervals [jlo, jhi): need = jhi - jlo + 1 + 64 knots; S = max(4, ceil(need / 64))
def cu_span(S, one_more=False):
    """(jlo, jhi) in the middle of the grid whose ``need`` is exactly 64 S (S >= 5: one more than 64 (S - 1))."""
    need = 64 * S if not one_more else 64 * (S - 1) + 1
    count = need - 2 * HALO      # = jmax - jmin + 1
    jlo = 300
    return jlo, jlo + count - 1


CU_NQ = [1, 63, 64, 65, 255, 256, 257, 512]


def cu_cases():
    """(name, radii, tables kind, positive, post_sqrt): every S at need = 64 S and at need = 64 (S - 1) + 1, stretches against ws = 2 and against
    ws + ne = n - 2, the first and the last admitted interval, every nq."""
    cases = []
    for S in range(SMIN, SMAX + 1):
        jlo, jhi = cu_span(S)
        cases.append(('S%d_full' % S, radii(257, jlo, jhi, S), 'generic', False, False))
        if S > SMIN:
            jlo, jhi = cu_span(S, one_more=True)
            cases.append(('S%d_first' % S, radii(130, jlo, jhi, S + 10), 'generic', False, False))
    cases.append(('low_end', radii(200, HALO + 2, 140, 1), 'generic', False, False))                 # ws = 2, the first admitted interval (32 knots from ws)
    cases.append(('high_end', radii(200, N - 140, N - 3 - HALO, 2), 'generic', False, False))        # ws + ne = n - 2, the last admitted interval
    for nq in CU_NQ:
        cases.append(('nq%d' % nq, radii(nq, 400, 520, nq), 'power', False, False))
    cases.append(('root_nq257', radii(257, 380, 600, 3), 'power', True, True))
    cases.append(('root_generic_nq65', radii(65, 380, 600, 4), 'generic', True, True))
    return cases


def prefiltered_cases():
    """(name, radii, positive, post_sqrt): QS = 4 / 8 at 256 / 257 radii, ne + 2 = 373 / 374 (four / three workgroups per CU), the largest span
    (ne + 2 = 512), the ends of the admitted range, every nq."""
    cases = [('nq%d' % nq, radii(nq, 400, 520, nq), False, False) for nq in CU_NQ]
    cases.append(('ne371', radii(256, 300, 300 + 370, 5), False, False))
    cases.append(('ne372', radii(257, 300, 300 + 371, 6), False, False))
    cases.append(('ne510', radii(512, 250, 250 + 509, 7), False, False))
    cases.append(('low_end', radii(100, HALO, 120, 8), False, False))                    # jmin = 32
    cases.append(('high_end', radii(100, N - 130, N - 1 - HALO, 9), False, False))       # jmax = n - 1 - 32
    cases.append(('root_nq257', radii(257, 380, 600, 3), True, True))
    return cases


RZ_SHAPES = [(nq, nz) for nz in (1, 2, 3, 64, 66, 128, 256, 258, 7) for nq in (1, 127, 128, 129, 257)]


# ---- truth, scale and level of a shipped case: computed once per process, read-only --------------------------------------------------------------
_cache = {}


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return case


def _transformed(kind, positive):
    key = ('transform', kind, positive)
    if key not in _cache:
        syn, base = tables(kind, positive), base_rows(positive or kind.startswith('spread'))
        true, f64 = transform(syn, base)
        _cache[key] = (syn, base, true, f64)
    return _cache[key]


def band_case(name):
    """dict(w, syn, base, y_true, y_f64, true, scale, level, f64, post_sqrt, root) of a case of :func:`band_cases`; truth and level of the two base rows."""
    if ('band', name) in _cache:
        return _cache['band', name]
    _, nq, bw, kind, positive, post_sqrt = [c for c in band_cases() if c[0] == name][0]
    syn, base, y_true, y_f64 = _transformed(kind, positive)
    w = dense_weights(band_layout(nq, bw), positive=positive)
    true, scale, f64 = band_truth(w, y_true), band_scale(w, y_true), band_product(w, y_f64)
    level = levels(true, scale, [f64], post_sqrt)
    _cache['band', name] = _freeze(dict(name=name, w=w, syn=syn, base=base, y_true=y_true, y_f64=y_f64, true=true, scale=scale, f64=f64, level=level,
                                        post_sqrt=post_sqrt, root=positive))
    return _cache['band', name]


def cu_case(name):
    """The same of a case of :func:`cu_cases`; restatements: the plain float64 solve and :func:`cu_restated`."""
    if ('cu', name) in _cache:
        return _cache['cu', name]
    _, r, kind, positive, post_sqrt = [c for c in cu_cases() if c[0] == name][0]
    syn, base, y_true, y_f64 = _transformed(kind, positive)
    true, scale = spline_truth(S_GRID, y_true, r), spline_scale(S_GRID, y_true, r)
    plain, f64 = spline_plain(S_GRID, y_f64, r), cu_restated(S_GRID, y_f64, r)
    level = levels(true, scale, [plain, f64], post_sqrt)
    _cache['cu', name] = _freeze(dict(name=name, r=r, syn=syn, base=base, y_true=y_true, y_f64=y_f64, true=true, scale=scale, plain=plain, f64=f64, level=level,
                                      post_sqrt=post_sqrt, root=positive, plan=cu_plan(S_GRID, r)))
    return _cache['cu', name]


def prefiltered_case(name, basis):
    """The same of a case of :func:`prefiltered_cases` ('power' tables); restatements: the plain float64 solve and :func:`prefiltered_restated`."""
    if ('prefiltered', name) in _cache:
        return _cache['prefiltered', name]
    _, r, positive, post_sqrt = [c for c in prefiltered_cases() if c[0] == name][0]
    syn, base, y_true, y_f64 = _transformed('power', positive)
    true, scale = spline_truth(S_GRID, y_true, r), spline_scale(S_GRID, y_true, r)
    plain, f64 = spline_plain(S_GRID, y_f64, r), prefiltered_restated(syn, base, S_GRID, r, basis)
    level = levels(true, scale, [plain, f64], post_sqrt)
    _cache['prefiltered', name] = _freeze(dict(name=name, r=r, syn=syn, base=base, y_true=y_true, y_f64=y_f64, true=true, scale=scale, plain=plain, f64=f64,
                                               level=level, post_sqrt=post_sqrt, root=positive, plan=prefiltered_plan(S_GRID, r)))
    return _cache['prefiltered', name]


def spline_operator(s, r):
    """The natural spline from knots s to radii r as a dense float64 operator (nq, n): the float64 spline of the unit rows (NaN rows for radii outside)."""
    return np.ascontiguousarray(st.spline(s, np.eye(len(s)), r, 'natural', dtype='f8').T)


OPERATOR_RADII = dict(nq=130, jlo=100, jhi=900, seed=11)


def spline_operator_case():
    """One real operator behind the band kernel: LinearOperator.spline(S_GRID, r, bc='natural'), whose band plan_from_dense cuts at 1e-18 of a row's
    maximum, against the longdouble natural spline of the transform's truth ('generic' tables).  Restatements: the plain float64 spline and the
    float64 product with :func:`spline_operator`."""
    if 'operator' in _cache:
        return _cache['operator']
    o = OPERATOR_RADII
    r = radii(o['nq'], o['jlo'], o['jhi'], o['seed'])
    syn, base, y_true, y_f64 = _transformed('generic', False)
    w = spline_operator(S_GRID, r)
    true, scale = spline_truth(S_GRID, y_true, r), spline_scale(S_GRID, y_true, r)
    plain, f64 = spline_plain(S_GRID, y_f64, r), band_product(w, y_f64)
    level = levels(true, scale, [plain, f64])
    _cache['operator'] = _freeze(dict(name='spline_operator', r=r, w=w, syn=syn, base=base, y_true=y_true, y_f64=y_f64, true=true, scale=scale, plain=plain, f64=f64,
                                      level=level, post_sqrt=False, root=False))
    return _cache['operator']


MIXED_EXTRA = 2 * SQRT_EXTRA + FLOOR      # a root within 1e-16, squared again: twice that and the rounding of the square


def mixed_sign_case(family, basis=None):
    """The root of rows of both signs: NaN exactly where the truth is negative.  ``true`` is the truth of the ARGUMENT of the root; the device's finite
    values are held squared, by the linear rule (:func:`mixed_fraction`)."""
    key = ('mixed', family)
    if key in _cache:
        return _cache[key]
    r = radii(130, 380, 600, 12)
    kind = 'generic' if family == 'cu' else 'power'
    syn, base, y_true, y_f64 = _transformed(kind, False)
    true, scale = spline_truth(S_GRID, y_true, r), spline_scale(S_GRID, y_true, r)
    plain = spline_plain(S_GRID, y_f64, r)
    f64 = cu_restated(S_GRID, y_f64, r) if family == 'cu' else prefiltered_restated(syn, base, S_GRID, r, basis)
    level = levels(true, scale, [plain, f64])
    _cache[key] = _freeze(dict(name='mixed_sign', r=r, syn=syn, base=base, y_true=y_true, y_f64=y_f64, true=true, scale=scale, plain=plain, f64=f64, level=level,
                               post_sqrt=False, root=False))
    return _cache[key]


def mixed_fraction(got, true, scale, level, what='', widen=None):
    """got: the device's roots, unscaled (longdouble).  NaN where the truth is negative or NaN and nowhere else; the squares of the others by the linear rule."""
    true = np.where(np.asarray(true) < 0, np.nan, true)
    got = np.asarray(got)
    return fraction(got * got, true, scale, level, extra=MIXED_EXTRA, what=what, widen=widen)


# ---- sigma(r, z): spectra formed inside the kernel (sigma_rz_kernel<E, false / true>), and the functional kernels ----------------------------------
# Cosmologies: RZ_NBASE base members of power_truth.make_case; batch item i is base member i % 4 with A_s times an exact 4**e_i, so that its spectrum
# scales by exactly 4**e_i (every factor of P but A_s is unchanged and a product with a power of two is exact) and sigma by 2**e_i: truth for the base
# members only.  The two members of a pair stay within 2^4 in amplitude (|e_a - e_b| <= 1, the base members' own spectra within a factor 4): the rows of a
# pair share a complex transform and the front end leaves them unscaled inside that spread (cp_fftlog_body.h), so the restatement that sets the level
# packs the pair as the kernel does (:func:`packed_restated`).
# Tables: the spectra span ten decades over the 1024 wavenumbers; a float64 transform rounds relative to the row's largest tilted sample, so that most
# output samples of such a row lie thousands of floors from their truth in any float64 arithmetic (measured: 96 to 221 floors with members spread as the
# generator draws them), and the root condition (truth at least 1/4 of its scale) is left to a few radii.  pre is therefore 1 / (the engine's float64
# spectrum of base member 0) times a factor in [0.95, 1.05], an input like any other, and the other members lie within a tenth of the generator's spread
# of member 0: the tilted rows are of order one with the differences between the cosmologies on them, and an error of the kernel's spectrum reaches sigma
# in full.  With the five taps, output knot j sees the wavenumbers around sample 1024 - j; bands and radii stay between knots 8 and RZ_KNOTS = 400 (knots 0 and 1 see the first two samples through the fifth tap), k > 0.03 h/Mpc:
# below, BBKS as the reference codes it loses 2^-53 / x of the result in any float64 arithmetic (power_truth's weight; pk_out keeps that weight over the
# whole grid).  Taps, post and band weights positive (every sigma takes the root).
# Allowance: ALLOW levels + (extra of the spectrum) / 2 + 1e-16, the spectrum's extra being power_truth's for the engine + 1e-15 for the geometric
# stepping of k (cp_sigma.hip, over evaluate_spectrum); sigma^2 is a positive combination of spectrum samples and the root halves relative errors.
# The level of the fused kernel is the larger one of two float64 restatements: spectra at the tabulated wavenumbers, and at the wavenumbers as the
# kernel steps them (:func:`stepped_k`), which the 1e-15 of the comment did not cover (2.0e-14 on P in the last eighth of the grid, measured here on the
# CPU; the comment is corrected).  The cap is held by the first.
RZ_NBASE = 4
RZ_CYCLE = np.array([0, 1, -1, -1, 1, 0, 0, 0])      # e_i of batch item i % 8
K_STEP_EXTRA = 1e-15
RZ_SEED = 21


RZ_NEAR = 0.1
RZ_KNOTS = 400      # the bands and radii of sigma(r, z) lie below this knot of the output grid


def rz_base():
    """power_truth.make_case's members, members 1 ... 3 moved to within RZ_NEAR of member 0 in every parameter: the tilted rows of all members are
    then of order one under ONE table pre (see above)."""
    if 'rz_base' not in _cache:
        case = pt.make_case('sigma', RZ_NBASE, K, seed=RZ_SEED)
        for name in ('p', 'pk'):
            case[name] = case[name][:1] + RZ_NEAR * (case[name] - case[name][:1])
        _cache['rz_base'] = case
    return _cache['rz_base']


def rz_parameters(ncosmo, nan=()):
    """(p (ncosmo, 8), pk (ncosmo, 5), e (ncosmo,)) of a batch; the members ``nan`` have h = NaN."""
    base = rz_base()
    index = np.arange(ncosmo) % RZ_NBASE
    e = RZ_CYCLE[np.arange(ncosmo) % RZ_CYCLE.size]
    p, pk = base['p'][index].copy(), base['pk'][index].copy()
    pk[:, 0] = pk[:, 0] * np.ldexp(1., 2 * e)
    for i in nan:
        p[i, 0] = np.nan
    return p, pk, e


def rz_spectra(engine, k=None):
    """(truth (4, nk) longdouble, float64 (4, nk), x of BBKS or None) of the base members without growth."""
    key = ('rz_spectra', engine, None if k is None else np.asarray(k).tobytes())
    if key not in _cache:
        base = dict(rz_base())
        if k is not None:
            base['k'] = np.asarray(k, dtype='f8')
        x = pt.case_x(base) if engine == 'bbks' else None
        _cache[key] = (pt.case_truth(base, engine, 'matter'), pt.case_truth(base, engine, 'matter', np.float64), x)
    return _cache[key]


def stepped_k():
    """The wavenumbers as sigma_rz_kernel forms them (cp_sigma.hip, evaluate_spectrum and the top of a pair), in float64: thread t0 = 0 ... 127 takes
    log k of its first sample from the thread index, k = exp of it, and steps seven times by k[128] / k[0] to its samples t0 + 128 r."""
    T = 128
    ln_k = np.log(K)
    ln_step, ratio = (ln_k[-1] - ln_k[0]) / (N - 1), K[T] / K[0]
    out = np.empty(N)
    kh = np.exp(np.arange(T) * ln_step + ln_k[0])
    for r in range(N // T):
        out[T * r:T * (r + 1)] = kh
        kh = kh * ratio
    return out


def rz_spectra_stepped(engine):
    """The float64 spectra at :func:`stepped_k`, (4, 1024): the restatement of the scheme that runs.  The stepped k is up to 7.1e-15 (32 ulp) from the
    table and P up to 2.0e-14 from its truth in the last eighth of the grid (k > 7.6 h/Mpc, |dlnP / dlnk| = 3); the kernel's comment said 1e-15."""
    key = ('rz_stepped', engine)
    if key not in _cache:
        _cache[key] = rz_spectra(engine, stepped_k())[1]
    return _cache[key]


def farther(true, a, b):
    """Entry by entry the one of two restatements that lies farther from the truth: its level is the larger of the two levels."""
    true = np.asarray(true)
    return np.where(np.abs(np.asarray(a).astype(LD) - true) >= np.abs(np.asarray(b).astype(LD) - true), a, b)


def pk_extra(engine, stepped):
    return pt.extra_of(engine, 'matter') + (K_STEP_EXTRA if stepped else 0.)


def sigma_extra(engine, stepped):
    return pk_extra(engine, stepped) / 2. + SQRT_EXTRA


def rz_tables(kind, engine):
    """tables(kind, positive) with pre = [0.95, 1.05] / (the engine's float64 spectrum of base member 0) over the samples."""
    key = ('rz_tables', kind, engine)
    if key not in _cache:
        syn = tables(kind, positive=True)
        in_left = tt.widths(N, NPAD)[0]
        pre = 1. + (syn.pre - 1.) / 3.
        pre[0, in_left:in_left + N] /= rz_spectra(engine)[1][0]
        syn.pre = pre
        _cache[key] = syn
    return _cache[key]


def rz_growth(ncosmo, nz, seed=0):
    return np.random.default_rng([ncosmo, nz, seed, 3]).uniform(0.2, 1., (ncosmo, nz))


def fft_truth(syn, rows):
    """The promised transform of longdouble rows for ANY u table, taken as given in float64: longdouble FFTs (transform_truth.rfft_truth / irfft_truth)."""
    import transform_truth as trt
    in_left, in_right, out_left = tt.widths(N, NPAD)
    z = np.zeros(rows.shape[:-1] + (NPAD,), dtype=LD)
    z[..., in_left:in_left + N] = np.asarray(rows).astype(LD) * syn.pre[0][in_left:in_left + N].astype(LD)
    g = trt.irfft_truth(np.conj(trt.rfft_truth(z) * syn.u[0].astype(tt.CLD)), NPAD) * syn.post[0].astype(LD)
    return g[..., out_left:out_left + N]


def _rz_variances(engine, form, syn, w=None, r=None, basis=None, s=None):
    """Per batch item of one period (8) and per base member: (v_true (4, nq), scale (4, nq), v_f64 paired (8, nq), v_f64 alone (8, nq), plain ...).
    form 'operator': the band form behind a real natural-spline operator on the knots s (w its float64 dense restatement)."""
    s = S_GRID if s is None else s
    p_true, p_plain, _ = rz_spectra(engine)
    y_true = fft_truth(syn, p_true) if syn.taps is None else tt.truth(p_true, N, NPAD, syn.pre[0], syn.post[0], syn.taps[0])
    if form == 'band':
        v_true, scale = band_truth(w, y_true), band_scale(w, y_true)
        tail = lambda y, c: [band_product(w, y)]      # noqa: E731
        u = None
    elif form == 'operator':
        v_true, scale = spline_truth(s, y_true, r), spline_scale(s, y_true, r)
        tail = lambda y, c: [band_product(w, y), spline_plain(s, y, r)]      # noqa: E731
        u = None
    else:
        v_true, scale = spline_truth(s, y_true, r), spline_scale(s, y_true, r)
        tail = lambda y, c: [prefiltered_tail(c, s, r, basis), spline_plain(s, y, r)]      # noqa: E731
        u = prefiltered_u(syn.u[0], basis)
    v_pair, v_alone, plain_count = [], [], 0
    for p_f64 in (p_plain, rz_spectra_stepped(engine)):      # the spectra at the tabulated wavenumbers, then at the kernel's
        rows = p_f64[np.arange(8) % RZ_NBASE] * np.ldexp(1., 2 * RZ_CYCLE)[:, None]
        paired, alone = [], []
        for a in range(0, 8, 2):
            for pair, out in ((rows[a:a + 2], paired), (rows[[a, a]], alone), (rows[[a + 1, a + 1]], alone)):
                y = packed_restated(syn, pair)
                c = packed_restated(syn, pair, u, keep_padding=True) if u is not None else None
                res = tail(y, c)
                out.append([t[:2] if out is paired else t[:1] for t in res])
        # paired: list over pairs of [restatements] each (2, nq); alone: list over items of [restatements] each (1, nq)
        nres = len(paired[0])
        v_pair += [np.concatenate([pr[i] for pr in paired]) for i in range(nres)]      # each (8, nq)
        v_alone += [np.concatenate([al[i] for al in alone]) for i in range(nres)]
        plain_count = plain_count or nres
    return v_true, scale, v_pair, v_alone, plain_count


def real_tables(pre, post, u):
    """The tables of a real transform (TophatVariance) as a Synthetic without taps: the truth transforms with longdouble FFTs."""
    syn = tt.Synthetic()
    syn.npad, syn.nker, syn.taps = NPAD, 1, None
    syn.pre, syn.post, syn.u = (np.ascontiguousarray(np.asarray(a).reshape(1, -1)) for a in (pre, post, u))
    return syn


def rz_case(engine, form, nq, nz, ncosmo, basis=None, nan=(), seed=0, bw=9, real=None):
    """A launch of the fused kernel: dict with the inputs (p, pk, growth, syn, w or r) and truth (ncosmo, nq, nz) longdouble, scale, level (ncosmo, nq),
    pk_true / pk_f64 / x (ncosmo, 1024) of the UNSCALED spectra and e.  form 'band': dense positive weights of bandwidth ``bw``; 'prefiltered': radii.
    real = (syn of :func:`real_tables`, knots s): the real TophatVariance tables, radii between knots 300 and 400 of s (4 to 30 Mpc/h), the band form
    behind the natural-spline operator of those radii."""
    p, pk, e = rz_parameters(ncosmo, nan)
    growth = rz_growth(ncosmo, nz, seed)
    knots = None
    if real is not None:
        syn, knots = real
        j = np.random.default_rng([nq, seed, 41]).integers(300, 400, nq)
        r = knots[j] + np.random.default_rng([nq, seed, 42]).uniform(0., 1., nq) * (knots[j + 1] - knots[j])
        w = spline_operator(knots, r) if form == 'band' else None
    elif form == 'band':
        syn, r = rz_tables('generic', engine), None
        w = dense_weights(band_layout(nq, bw, seed, hi=RZ_KNOTS, lo=8), seed, positive=True)
    else:
        syn, w = rz_tables('power', engine), None
        r = radii(nq, RZ_KNOTS - 100, RZ_KNOTS, seed + nq)
    key = ('rz_var', engine, form, nq, seed, bw, real is not None)
    if key not in _cache:
        _cache[key] = _rz_variances(engine, 'operator' if real is not None and form == 'band' else form, syn, w, r, basis, knots)
    v_true, scale_v, v_pair, v_alone, plain_count = _cache[key]
    member, period = np.arange(ncosmo) % RZ_NBASE, np.arange(ncosmo) % 8
    factor = np.ldexp(LD(1), 2 * e)[:, None, None] * growth.astype(LD)[:, None, :]
    with np.errstate(invalid='ignore'):
        true = np.sqrt(v_true[member][:, :, None] * factor)
        scale = np.sqrt(scale_v[member][:, :, None] * factor)
    level, level_plain = np.full((ncosmo, nq), FLOOR), None
    for count, (vp, va) in enumerate(zip(v_pair, v_alone)):
        if count == plain_count:
            level_plain = level.copy()      # of the restatements at the tabulated wavenumbers: what the cap is about
        v = vp[period].copy()
        if ncosmo % 2:
            v[-1] = va[period[-1]]
        with np.errstate(invalid='ignore'):
            f64 = np.sqrt(v)[:, :, None] * np.sqrt(growth)[:, None, :]
        nanq = np.isnan(true)
        assert np.array_equal(np.isnan(f64), nanq)
        rel = np.asarray(np.where(nanq, 0, np.abs(f64.astype(LD) - true)) / scale, dtype='f8')
        level = np.maximum(level, rel.max(axis=-1))
    true[list(nan)] = np.nan
    p_true, p_f64, x = rz_spectra(engine)
    p_f64 = farther(p_true, p_f64, rz_spectra_stepped(engine))
    return dict(engine=engine, form=form, p=p, pk=pk, e=e, growth=growth, syn=syn, w=w, r=r, true=true, scale=scale, level=level, level_plain=level_plain,
                nan=tuple(nan), pk_true=p_true[member], pk_f64=p_f64[member], x=None if x is None else x[member], v_true=v_true, scale_v=scale_v)


def rz_fraction(got, case, extra, what=''):
    """The largest fraction of ALLOW x level + extra over the (cosmology, radius) blocks of sigma(r, z); NaN exactly where the truth has it."""
    got, true = np.asarray(got).astype(LD), case['true']
    assert got.shape == true.shape, (got.shape, true.shape)
    nanq = np.isnan(true)
    assert np.array_equal(np.isnan(got), nanq), '{}: NaN in other places than the truth has them'.format(what)
    rel = np.asarray(np.where(nanq, 0, np.abs(got - true)) / case['scale'], dtype='f8').max(axis=-1)
    used = rel / (ALLOW * case['level'] + extra)
    worst = float(used.max())
    at = np.unravel_index(int(np.argmax(used)), used.shape)
    print('%s: largest fraction of the allowance %.3g at cosmology %d, radius %d (level at most %.3g FLOOR)' % (what, worst, at[0], at[1], float(case['level'].max() / FLOOR)))
    return worst


def pk_fraction(got, case, extra, what='', cap=None):
    """``pk_out`` by power_truth's per-decade rule and caps: the device's spectra with the exact 4**e taken out against the base members' truth.  ``cap``:
    None for power_truth's (the restatement at the tabulated wavenumbers); the fused kernel's restatement at its own, stepped wavenumbers is a property
    of the scheme and not of the case (tests/test_sigma_truth_host.py holds the case itself below the cap)."""
    got = np.asarray(got).astype(LD) * np.ldexp(LD(1), -2 * case['e'])[:, None]
    keep = np.array([i not in case['nan'] for i in range(len(got))])
    assert np.isnan(got[~keep]).all(), what
    engine = case['engine']
    x = None if case['x'] is None else case['x'][keep]
    d, t, f = pt.prepared(engine, 'matter', K if got.shape[1] == N else case['k'], got[keep], case['pk_true'][keep], case['pk_f64'][keep], x)
    return bt.assert_pointwise(d, t, f, what, extra=extra, cap=pt.cap_of('matter') if cap is None else cap)


# the functional kernels: sigma^2(r_q) = sum_j F[q, j] P(k_j) with F an input
FUNCTIONAL_NK = [1, 63, 64, 65, 1024, 1030]


def functional_k(nk):
    return K if nk == N else (np.array([0.05]) if nk == 1 else np.geomspace(1e-4, 30., nk))


def functional_case(engine, nq, nz, nk, ncosmo, nan=(), seed=0):
    """cp_sigma_rz_functional: d_functional (nq, nk) random positive; truth: the longdouble dot product, then growth, then root."""
    k = functional_k(nk)
    p, pk, e = rz_parameters(ncosmo, nan)
    growth = rz_growth(ncosmo, nz, seed)
    functional = np.random.default_rng([nq, nk, seed, 8]).uniform(0.5, 1.5, (nq, nk))
    p_true, p_f64, x = rz_spectra(engine, k)
    member = np.arange(ncosmo) % RZ_NBASE
    acc_true = p_true @ functional.astype(LD).T      # (4, nq)
    acc_f64 = np.zeros((RZ_NBASE, nq))
    for j in range(nk):      # (in the order of the wavenumbers)
        acc_f64 = acc_f64 + p_f64[:, j:j + 1] * functional[None, :, j]
    factor = np.ldexp(LD(1), 2 * e)[:, None, None] * growth.astype(LD)[:, None, :]
    true = np.sqrt(acc_true[member][:, :, None] * factor)
    f64 = np.sqrt(acc_f64[member] * np.ldexp(1., 2 * e)[:, None])[:, :, None] * np.sqrt(growth)[:, None, :]
    level = np.maximum(np.asarray(np.abs(f64.astype(LD) - true) / true, dtype='f8').max(axis=-1), FLOOR)
    true[list(nan)] = np.nan
    return dict(engine=engine, p=p, pk=pk, e=e, growth=growth, functional=functional, k=k, true=true, scale=np.where(np.isnan(true), 1, true), level=level,
                nan=tuple(nan), pk_true=p_true[member], pk_f64=p_f64[member], x=None if x is None else x[member], acc_true=acc_true, acc_f64=acc_f64)


def normalise_case(engine, ncosmo, per_cosmology, nan=(), seed=0):
    """cp_sigma8_normalise: rs = target / (sqrt(acc) |g0|) with g0 the CPT92 growth factor at z = 0 (background_truth), amplitude = A_s rs^2 and
    pk_out = P rs^2, each with the float64 restatement that sets its level (entry by entry)."""
    case = functional_case(engine, 1, 1, N, ncosmo, nan, seed)
    rng = np.random.default_rng([ncosmo, seed, 12])
    target = rng.uniform(0.6, 1., ncosmo) if per_cosmology else np.full(ncosmo, 0.8)
    member = np.arange(ncosmo) % RZ_NBASE
    base = rz_base()
    out = {}
    for dtype in (LD, np.float64):
        c = pt.case_cosmo(base, dtype)
        g0 = np.abs(bt.elementwise(c, np.array([0.]), 'growth_cpt')[:, 0])[member]
        acc = (case['acc_true'] if dtype is LD else case['acc_f64'])[member, 0] * np.ldexp(dtype(1), 2 * case['e'])
        rs = target.astype(dtype) / (np.sqrt(acc) * g0)
        spectra = (case['pk_true'] if dtype is LD else case['pk_f64']) * np.ldexp(dtype(1), 2 * case['e'])[:, None]
        out[dtype] = dict(rsigma8=rs, amplitude=case['pk'][:, 0].astype(dtype) * rs * rs, pk_out=spectra * (rs * rs)[:, None])
    for v in out.values():
        for a in v.values():
            a[list(nan)] = np.nan
    case.update(target=target, per_cosmology=per_cosmology, norm_true=out[LD], norm_f64=out[np.float64])
    return case


RZ_SMALL = [(1, 1), (127, 2), (129, 3)]      # (nq, nz) run with all three engines


def rz_cases():
    """(engine, form, nq, nz, ncosmo, nan members, pk_out given) of the fused kernel: the three store paths and their seams (RZ_SHAPES) with one
    engine, the small shapes with all three; 1, 2, 3 cosmologies; a NaN cosmology in slot a and in slot b of a pair, and of an odd batch's last."""
    cases = []
    for form in ('band', 'prefiltered'):
        for engine in pt.ENGINES:
            cases += [(engine, form, nq, nz, 3, (), engine != 'bbks') for nq, nz in RZ_SMALL]
        cases += [('eisenstein_hu', form, nq, nz, 3, (), (nq + nz) % 2 == 0) for nq, nz in RZ_SHAPES if (nq, nz) not in RZ_SMALL]
        cases += [('eisenstein_hu_nowiggle', form, 128, 7, ncosmo, (), True) for ncosmo in (1, 2)]
        cases += [('bbks', form, 129, 66, 5, (2,), True), ('bbks', form, 129, 66, 5, (1, 4), False)]
    return cases


FUNCTIONAL_NZ = [1, 2, 63, 64, 65]
FUNCTIONAL_NCOSMO = [1, 3, 4, 5, 257]


def functional_cases():
    """(engine, nq, nz, nk, ncosmo, nan, pk_out given)."""
    cases = []
    for i, nk in enumerate(FUNCTIONAL_NK):
        cases.append((pt.ENGINES[i % 3], 1 + i % 4, FUNCTIONAL_NZ[i % 5], nk, FUNCTIONAL_NCOSMO[i % 5], (), i % 2 == 0))
    for i, nz in enumerate(FUNCTIONAL_NZ):
        cases.append((pt.ENGINES[(i + 1) % 3], 4 - i % 4, nz, 65, 5, (), i % 2 == 1))
    for i, ncosmo in enumerate(FUNCTIONAL_NCOSMO):
        cases.append((pt.ENGINES[(i + 2) % 3], 1 + (i + 1) % 4, 3, 1024, ncosmo, (), True))
    cases += [(engine, 4, 65, 1030, 9, (wave,), wave % 2 == 0) for wave, engine in zip(range(4), pt.ENGINES + ('eisenstein_hu',))]      # a NaN cosmology in each wave of block 0
    cases.append(('eisenstein_hu', 2, 2, 64, 9, (4, 7), True))
    return cases
