"""
Exact truth of the FFTLog transform for kernel tables made of a few taps, and the rows tests/test_fftlog_large_truth_gpu.py feeds the four-step path
of csrc/cp_fftlog_large.hip (padded lengths Np = 2^14 ... 2^24).  numpy only, no device.

The transform a plan promises for ANY tables pre, post, u is that of oracle/fftlog.py:apply,
  g = irfft(conj(rfft(z) u), Np) post,   z = pad(row) pre.
With  u[k] = sum_t h_t exp(+2 pi i ((k d_t) mod Np) / Np),  k = 0 ... Np/2  (real weights h_t, integer shifts d_t, the product k d_t reduced in int64
before it meets pi) the spectrum product is a sum of pure shifts and, exactly,
  g[m] = post[m] sum_t h_t z[(d_t - m) mod Np],
a sparse circular correlation: O(taps x Np) operations in ``np.longdouble`` and no FFT, at every size the path takes.  (The DC and Nyquist bins of
u are real up to the rounding of sin(pi x integer), which irfft ignores.)  tests/test_fftlog_taps_host.py holds :func:`truth` to an O(Np^2)
longdouble DFT of the promised transform and :func:`restated` to ``oracle.fftlog.apply``.

Taps (:func:`taps`): five per kernel index, d = (0, 1, Np/3 + 7, Np - 5, Np/2 + 1) for index 0 and moved by a few samples for the others, weights of
order one and of both signs.  Shifts of both kinds -- next to 0 and generic -- so that u has no short period in k: a permutation of the frequency
index inside the U layout cannot hide behind a period.
Tables (:func:`tables`): pre and post random, magnitude in [0.5, 1.5], both signs, different per kernel index.

Tolerance rule (that of tests/spline_truth.py and tests/jacobian_reference.py), :func:`levels` and :func:`check`: per row,
``level`` is the largest distance of the float64 restatement (:func:`restated`: np.fft.rfft / irfft with the u table as handed to the plan) from
the truth over the row's largest |truth|, floored at FLOOR = 1.1e-16; the device is allowed ALLOW = 16 levels; NaN exactly where the truth has it.

Rows (:func:`base_rows`, :func:`batch`): two dense base rows per size, entries of magnitude uniform in [0.5, 1.5] and of random sign; batch item i
is base row i % 2 times an exact 2**e, |e| <= 300, another e for every (item, kernel index).  The two members of a pair of the kernel (items 2j and
2j + 1 of one kernel index) therefore always differ in content and in scale.  The transform is linear and zero / 'edge' padding scale with the
row, so the truth of a row is the truth of its base row times 2**e: longdouble work and restatement once per (base row, kernel index).  'log'
padding is left out: over paddings this long the geometric continuation overflows, in the reference as well (test_large_sizes covers it at 2^14).
"""
import numpy as np

from oracle import fftlog as ofl

LD = np.longdouble
CLD = np.clongdouble
FLOOR = 1.1e-16
ALLOW = 16.
CAP = 32.       # the level of every case in use stays below CAP x FLOOR (tests/test_fftlog_taps_host.py)
NBASE = 2
EXPONENT_RANGE = 300
EXPONENTS = np.random.default_rng(20241019).integers(-EXPONENT_RANGE, EXPONENT_RANGE + 1, 4096)


def taps(npad, ker=0):
    """(shifts, weights) of kernel index ``ker``: int64 shifts in [0, npad), float64 weights."""
    shifts = np.array([3 * ker, 1, npad // 3 + 7 + 11 * ker, npad - 5 - ker, npad // 2 + 1 + 2 * ker], dtype='i8') % npad
    weights = np.roll(np.array([0.9, -0.7, 1.3, -1.1, 0.6]), ker) * (1. + 0.125 * ker)
    assert np.unique(shifts).size == shifts.size
    return shifts, weights


def u_table(npad, tap, dtype='f8'):
    """u[k] = sum_t h_t exp(+2 pi i ((k d_t) mod Np) / Np), k = 0 ... Np/2: complex128 (``dtype=LD``: complex longdouble, for the host tests)."""
    shifts, weights = tap
    k = np.arange(npad // 2 + 1, dtype='i8')
    real = np.dtype(dtype).type
    two_pi = real(8) * np.arctan(real(1))
    u = np.zeros(k.size, dtype=CLD if real is LD else 'c16')
    for d, h in zip(shifts, weights):
        phase = ((k * int(d)) % npad).astype(dtype) * (two_pi / real(npad))
        u += real(h) * (np.cos(phase) + 1j * np.sin(phase))
    return u


class Synthetic(object):
    """pre, post (nker, npad) float64, u (nker, npad/2 + 1) complex128 and the taps u was made of, per kernel index."""


def tables(npad, nker=1, seed=0):
    rng = np.random.default_rng([npad, nker, seed])
    t = Synthetic()
    t.npad, t.nker = npad, nker
    t.pre = rng.uniform(0.5, 1.5, (nker, npad)) * rng.choice([-1., 1.], (nker, npad))
    t.post = rng.uniform(0.5, 1.5, (nker, npad)) * rng.choice([-1., 1.], (nker, npad))
    t.taps = [taps(npad, ker) for ker in range(nker)]
    t.u = np.array([u_table(npad, tap) for tap in t.taps])
    return t


def widths(n, npad):
    """(in_left, in_right, out_left) as oracle.fftlog.setup has them (fftlog.py:152-153)."""
    tot = npad - n
    return tot // 2, tot - tot // 2, tot - tot // 2


def truth(rows, n, npad, pre, post, tap, extrap=0, keep_padding=False):
    """The promised transform of ``rows`` (..., n) for ONE kernel index (pre, post of shape (npad,)) in longdouble: (..., npad if keep_padding
    else n).  A row that is not finite gives a row of NaN, as the FFTs of the promise do."""
    rows = np.asarray(rows)
    assert rows.shape[-1] == n and pre.shape == (npad,) and post.shape == (npad,)
    in_left, in_right, out_left = widths(n, npad)
    m = np.arange(npad, dtype='i8') if keep_padding else np.arange(out_left, out_left + n, dtype='i8')
    shifts, weights = tap
    flat = rows.reshape(-1, n)
    out = np.empty((flat.shape[0], m.size), dtype=LD)
    pre, post_m = pre.astype(LD), post[m].astype(LD)
    for i, row in enumerate(flat):        # (row by row: one padded longdouble row of 2^24 samples takes 268 MB)
        with np.errstate(invalid='ignore'):
            z = ofl.pad(row.astype(LD), (in_left, in_right), extrap) * pre
        if not np.isfinite(z).all():
            out[i] = np.nan
            continue
        acc = np.zeros(m.size, dtype=LD)
        for d, h in zip(shifts, weights):
            acc += LD(h) * z[(int(d) - m) % npad]
        out[i] = post_m * acc
    return out.reshape(rows.shape[:-1] + (m.size,))


def restated(rows, n, npad, pre, post, u, extrap=0, keep_padding=False):
    """The same operation in float64 through numpy's FFTs (the arithmetic of oracle.fftlog.apply), with the u table as handed to the plan."""
    in_left, in_right, out_left = widths(n, npad)
    a = ofl.pad(np.asarray(rows, dtype='f8'), (in_left, in_right), extrap)
    spec = np.fft.rfft(a * pre, axis=-1) * u
    g = np.fft.irfft(spec.conj(), n=npad, axis=-1) * post
    return g if keep_padding else g[..., out_left:out_left + n]


def levels(true, f64):
    """(top, level), each (rows,): per row the largest |truth| and the rounding level of the float64 restatement, floored at FLOOR."""
    true, f64 = np.asarray(true), np.asarray(f64).astype(LD)
    nan = np.isnan(true)
    top = np.where(nan, 0, np.abs(true)).max(axis=-1)
    dist = np.where(nan, 0, np.abs(f64 - true)).max(axis=-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        level = np.where(top > 0, dist / top, 0)
    return top, np.maximum(np.asarray(level, dtype='f8'), FLOOR)


def check(got, true, level, what=''):
    """Largest fraction of the allowance ALLOW x level x max|truth| that a row of ``got`` (rows, m) is away from its truth (rows, m); printed and
    returned.  NaN must be exactly where the truth has it (AssertionError otherwise); a row whose truth is
    zero throughout has no allowance: inf unless it is zero throughout."""
    got, true = np.asarray(got).astype(LD), np.asarray(true)
    assert got.shape == true.shape, (what, got.shape, true.shape)
    level = np.broadcast_to(np.asarray(level, dtype='f8'), got.shape[:-1])
    nan = np.isnan(true)
    assert np.array_equal(np.isnan(got), nan), '{}: NaN in other places than the truth has them'.format(what)
    assert np.isfinite(got[~nan]).all(), what
    top = np.where(nan, 0, np.abs(true)).max(axis=-1)
    dist = np.where(nan, 0, np.abs(got - true)).max(axis=-1)
    allowed = LD(ALLOW) * level * top
    with np.errstate(divide='ignore', invalid='ignore'):
        fraction = np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0)).astype('f8')
    worst = float(fraction.max())
    print('%s: largest fraction of the allowance %.3g in row %d (level at most %.3g FLOOR)' % (what, worst, int(np.argmax(fraction)), float(level.max() / FLOOR)))
    return worst


def base_rows(n, seed=0):
    """(2, n) float64: magnitude uniform in [0.5, 1.5], random sign."""
    rng = np.random.default_rng([n, seed, 77])
    return rng.uniform(0.5, 1.5, (NBASE, n)) * rng.choice([-1., 1.], (NBASE, n))


def exponents(nbatch, nker):
    if nbatch * nker > EXPONENTS.size:
        raise ValueError('at most {:d} rows'.format(EXPONENTS.size))
    return EXPONENTS[:nbatch * nker].reshape(nbatch, nker)


def batch(base, nbatch, nker):
    """(nbatch, nker, n): item i of kernel index ker is base row i % 2 times 2**exponents[i, ker]."""
    scale = np.ldexp(1., exponents(nbatch, nker))
    return base[np.arange(nbatch) % NBASE][:, None, :] * scale[:, :, None]


def unscale(got, nbatch, nker):
    """The device's (nbatch, nker, m) rows divided by their 2**e, exactly, in longdouble."""
    got = np.asarray(got)
    assert got.shape[:2] == (nbatch, nker)
    return got.astype(LD) * np.ldexp(LD(1), -exponents(nbatch, nker))[:, :, None]


def base_case(n, npad, syn, extrap, keep_padding, seed=0):
    """Truth and level of the two base rows under every kernel index of ``syn``: (base (2, n), truth (2, nker, m) longdouble, level (2, nker))."""
    base = base_rows(n, seed)
    true, level = [], []
    for ker in range(syn.nker):
        t = truth(base, n, npad, syn.pre[ker], syn.post[ker], syn.taps[ker], extrap, keep_padding)
        f = restated(base, n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep_padding)
        true.append(t)
        level.append(levels(t, f)[1])
    return base, np.stack(true, axis=1), np.stack(level, axis=1)


_shared = {}
_last_tables = [None]


def ladder_tables(npad):
    """:func:`tables` of the ladder's case of npad (seed 0); up to the first three-pass size the last one made is kept, for the modes of one size
    (beyond it a size has one mode, and its tables take hundreds of MB)."""
    if npad > THREE_PASS:
        return tables(npad, ladder_case(npad)[2])
    if _last_tables[0] is None or _last_tables[0].npad != npad:
        _last_tables[0] = tables(npad, ladder_case(npad)[2])
    return _last_tables[0]


def ladder_truth(npad, extrap, keep_padding):
    """(syn, base, truth, level) of a case of the ladder: :func:`tables` with the ladder's number of kernel indices and :func:`base_case` of them.
    The case of the first three-pass size serves two tests: it is computed once, kept, and read-only."""
    key = (npad, extrap, keep_padding)
    if key in _shared:
        return _shared[key]
    n, nbatch, nker, modes = ladder_case(npad)
    syn = ladder_tables(npad)
    case = (syn,) + base_case(n, npad, syn, extrap, keep_padding)
    if npad == THREE_PASS:
        for array in (syn.pre, syn.post, syn.u) + case[1:]:
            array.flags.writeable = False
        _shared[key] = case
    return case


def expected(true, level, nbatch):
    """Truth (nbatch, nker, m) and level (nbatch, nker) of the UNSCALED batch from those of the base rows (a view per row, no copy of the values)."""
    index = np.arange(nbatch) % NBASE
    return true[index], level[index]


# ---- the ladder of tests/test_fftlog_large_truth_gpu.py: one case per column plan N1 = Np / 4096 = 4 ... 4096 -----------------------------------
LADDER = [1 << e for e in range(14, 25)]
THREE_PASS = 1 << 21      # from here on the column transform takes three passes


def ladder_case(npad):
    """(n, nbatch, nker, modes) of padded length npad: n odd with npad - n odd (in_left != out_left); about Np/3 below 2^21, 10^6 + 3 from there
    on, where 'edge' padding makes z dense.  Three batch items: two pairs per kernel index, the second without a partner.  modes: (extrap,
    keep_padding)."""
    if npad < THREE_PASS:
        return (npad // 3) | 1, 3, 2, [('edge', False), ((0, 'edge'), True)]
    return 1000003, 3, 1, [('edge', False)]


def extrap_codes(extrap):
    """(code, value, code, value) of cp_fftlog_execute for 0 / 'edge' per side."""
    left, right = extrap if isinstance(extrap, tuple) else (extrap, extrap)
    code = lambda e: (1, 0.) if e == 'edge' else (0, float(e))      # noqa: E731
    return code(left) + code(right)
