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

The fused sizes Np = 4 ... 8192 (tests/test_fftlog_fused_truth_gpu.py): the identity holds at every size; up to Np = 32 the taps follow
:func:`small_taps`; :func:`fused_cases` names the cases of a size; 'log' padding takes rows whose end ratios are exact (:func:`log_rows`: it is
homogeneous in the row, so the 2**e batches serve it as well); ``batch`` / ``unscale`` / ``exponents`` take the exponent table as an argument
(:func:`pair_table`: pairs a chosen number of binades apart, or all equal in scale).
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


SMALL = 32      # up to here the five shifts of the large sizes collide modulo Np: the small-size rule of small_taps


def small_taps(npad, ker=0):
    """Taps of Np = 4 ... SMALL: min(5, Np - 1) of them, shifts distinct modulo Np, 0 and 1 among them and the third one above Np/2 (Np - 1 - ker where that
    is, Np - 1 otherwise), the rest moved with the kernel index; the weights of :func:`taps`, cut to that number, of both signs."""
    count = min(5, npad - 1)
    high = npad - 1 - ker if npad - 1 - ker > npad // 2 else npad - 1
    shifts = [0, 1]
    for cand in [high, npad // 2 + 1 + ker, npad // 3 + 2 + 2 * ker] + list(range(2, npad)):
        if len(shifts) < count and cand % npad not in shifts:
            shifts.append(cand % npad)
    shifts = np.array(shifts, dtype='i8')
    weights = (np.roll(np.array([0.9, -0.7, 1.3, -1.1, 0.6]), ker) * (1. + 0.125 * ker))[:count]
    assert shifts.size == count and np.unique(shifts).size == count and (shifts > npad // 2).any() and weights.min() < 0. < weights.max()
    return shifts, weights


def taps(npad, ker=0):
    """(shifts, weights) of kernel index ``ker``: int64 shifts in [0, npad), float64 weights."""
    if npad <= SMALL:
        return small_taps(npad, ker)
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


def exponents(nbatch, nker, table=None):
    """(nbatch, nker) exponents, row-major from ``table`` (default: the module's EXPONENTS), repeated cyclically where the batch has more rows."""
    table = EXPONENTS if table is None else np.asarray(table, dtype='i8').ravel()
    return table[np.arange(nbatch * nker) % table.size].reshape(nbatch, nker)


def paired_exponents(difference):
    """A table for :func:`exponents` that gives the two members of every pair (items 2j, 2j + 1 of one kernel index, nker = 1 or 3) exponents
    ``difference`` apart, the larger one now in the first and now in the second member, around a base that moves with the pair.
    difference = 0: all exponents 0 -- every pair equal in scale, different in content, no fix-up taken."""
    if difference == 0:
        return np.zeros(1, dtype='i8')
    pairs = np.arange(64)
    base = (7 * pairs) % 23 - 11
    first = np.where(pairs % 2 == 0, difference, 0)
    return np.stack([base + first, base + difference - first], axis=1)      # (pair, member); laid out per nker by pair_table


def pair_table(nbatch, nker, difference):
    """(nbatch, nker) exponents whose pairs are ``difference`` apart (:func:`paired_exponents`), for ``exponents(..., table=...)``."""
    pe = paired_exponents(difference)
    if difference == 0:
        return np.zeros((nbatch, nker), dtype='i8')
    item, ker = np.meshgrid(np.arange(nbatch), np.arange(nker), indexing='ij')
    pair = ((item // 2) * nker + ker) % pe.shape[0]
    return pe[pair, item % 2]


def batch(base, nbatch, nker, table=None):
    """(nbatch, nker, n): item i of kernel index ker is base row i % 2 times 2**exponents[i, ker]."""
    scale = np.ldexp(1., exponents(nbatch, nker, table))
    return base[np.arange(nbatch) % NBASE][:, None, :] * scale[:, :, None]


def unscale(got, nbatch, nker, table=None):
    """The device's (nbatch, nker, m) rows divided by their 2**e, exactly, in longdouble."""
    got = np.asarray(got)
    assert got.shape[:2] == (nbatch, nker)
    return got.astype(LD) * np.ldexp(LD(1), -exponents(nbatch, nker, table))[:, :, None]


def log_rows(n, npad, seed=0, negative=False):
    """(2, n) base rows for 'log' padding: :func:`base_rows` with end ratios that are exact in float64.  The end samples are rounded to 12 mantissa
    bits and their neighbours set to a_0 (1 + 2^-k) and a_{n-1} (1 + 2^-k), k = max(6, log2 Np - 1): both ratios of the continuation (a_1 / a_0 and
    a_{n-2} / a_{n-1}) are 1 + 2^-k exactly, it decays outwards, by at most e^2 over Np/2 steps.  (A random ratio is rounded, and the rounding is
    raised to a power of up to Np/2 in the restatement: levels of 30 ... 1270 FLOOR.)  negative: a_1 = -a_0 (1 + 2^-k) in row 1, a left end ratio
    the kernel hands to the library's pow."""
    assert n >= 3
    k = max(6, npad.bit_length() - 2)
    a = base_rows(n, seed).copy()
    step = 1. + 2.**-k
    for end in (0, n - 1):
        mant, expo = np.frexp(a[:, end])
        a[:, end] = np.ldexp(np.round(mant * 4096.) / 4096., expo)
    if n == 3:
        a[:, 2] = a[:, 0]
    a[:, 1] = a[:, 0] * step
    a[:, n - 2] = a[:, n - 1] * step
    if negative:
        a[1, 1] = -a[1, 1]
        assert n >= 4
    assert (np.abs(a[:, 1] / a[:, 0]) == step).all() and (a[:, n - 2] / a[:, n - 1] == step).all() and (a[0, 1] / a[0, 0] == step)
    return a


def base_case(n, npad, syn, extrap, keep_padding, seed=0, kind='dense'):
    """Truth and level of the two base rows under every kernel index of ``syn``: (base (2, n), truth (2, nker, m) longdouble, level (2, nker)).
    kind: 'dense' (:func:`base_rows`), 'log' or 'logneg' (:func:`log_rows`)."""
    base = base_rows(n, seed) if kind == 'dense' else log_rows(n, npad, seed, negative=kind == 'logneg')
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
    """(code, value, code, value) of cp_fftlog_execute for a number / 'edge' / 'log' per side."""
    left, right = extrap if isinstance(extrap, tuple) else (extrap, extrap)
    code = lambda e: (1, 0.) if e == 'edge' else (2, 0.) if e == 'log' else (0, float(e))      # noqa: E731
    return code(left) + code(right)


# ---- the sizes of the fused kernel (csrc/cp_fftlog_body.h), tests/test_fftlog_fused_truth_gpu.py ---------------------------------------------------
FUSED_LADDER = [1 << e for e in range(2, 14)]
HALF_MIN = 512      # CP_FFTLOG_HALF_MIN_NP: from here on 2 n = Np without keep_padding takes a HALF variant
LOG_MAX_N = 2048    # the facade offers 'log' padding up to this row length
VARIANTS = ('generic', 'log', 'half', 'half_zero')


def variant_of(n, npad, extrap, keep_padding):
    """The rule of select_variant (csrc/cp_fftlog_dispatch.h), restated: which kernel variant a case runs."""
    left, right = extrap if isinstance(extrap, tuple) else (extrap, extrap)
    if 'log' in (left, right):
        return 'log'
    if npad >= HALF_MIN and 2 * n == npad and not keep_padding:
        return 'half_zero' if (left, right) == (0, 0) else 'half'
    return 'generic'


def fused_cases(npad, variants=VARIANTS):
    """The cases of one fused size, [(n, extrap, keep_padding, kind)] (each is run with nker = 1 and 3; kind: the rows of :func:`base_case`):
    generic    n = (Np/3)|1 (n and Np - n odd: in_left != out_left; 2 at Np = 4) and n = Np - 1, padding 0, 'edge', (1.5, 'edge'), cropped and with keep_padding;
               from Np = 512 on also 2 n = Np with keep_padding (the rule of select_variant that refuses HALF), 0 and 'edge'
    half       n = Np/2, 'edge' and (0.7, 0.), Np >= 512
    half_zero  n = Np/2, zero padding, Np >= 512
    log        the exact-ratio rows: 'log', ('log', 0.3), (0.2, 'log') at n = Np/2 and (Np/3)|1 (3 <= n <= 2048: Np = 4 takes n = 3, Np = 8192
               n = 2047), and one case whose row 1 has a negative left end ratio."""
    cases = []
    third, half = max((npad // 3) | 1, 2), npad // 2      # (a plan needs n >= 2: Np = 4 takes n = 2 and 3)
    if 'generic' in variants:
        for n in (third, npad - 1):
            for extrap in (0, 'edge', (1.5, 'edge')):
                cases += [(n, extrap, False, 'dense'), (n, extrap, True, 'dense')]
        if npad >= HALF_MIN:
            cases += [(half, 0, True, 'dense'), (half, 'edge', True, 'dense')]
    if npad >= HALF_MIN:
        if 'half' in variants:
            cases += [(half, 'edge', False, 'dense'), (half, (0.7, 0.), False, 'dense')]
        if 'half_zero' in variants:
            cases += [(half, 0, False, 'dense')]
    if 'log' in variants:
        sizes = sorted(set(LOG_MAX_N - 1 if n > LOG_MAX_N else max(n, 3) for n in (half, third)))
        for n in sizes:
            cases += [(n, 'log', n == sizes[0], 'log'), (n, ('log', 0.3), False, 'log'), (n, (0.2, 'log'), True, 'log')]
        if sizes[-1] >= 4:
            cases += [(sizes[-1], 'log', False, 'logneg')]
    for n, extrap, keep, kind in cases:
        assert 1 <= n <= npad and variant_of(n, npad, extrap, keep) in variants
    return cases


SPREAD = 4      # CP_ROW_SCALE_SPREAD: pairs whose magnitude fields differ by more are rescaled row by row


def homogeneous(extrap):
    """Whether the padding scales with the row (0, 'edge', 'log' on both sides): then the 2**e batches share the truth of their base rows."""
    left, right = extrap if isinstance(extrap, tuple) else (extrap, extrap)
    return all(isinstance(e, str) or e == 0 for e in (left, right))


def tilted_top(rows, n, npad, pre, extrap):
    """Largest |padded sample x prefactor| per row (..., n) -> (...): the magnitude the kernel's row screening measures."""
    in_left, in_right, _ = widths(n, npad)
    with np.errstate(all='ignore'):
        return np.abs(ofl.pad(np.asarray(rows, dtype='f8'), (in_left, in_right), extrap) * pre).max(axis=-1)


def pair_factor(top):
    """The kernel's documented contract (csrc/cp_fftlog_body.h, "Row independence"): batch items 2j and 2j + 1 of a kernel index share one complex
    transform; when the exponent fields of their tilted magnitudes ``top`` (nbatch, nker) differ by more than SPREAD each row is rescaled and
    rounding is relative to the row itself (factor 1), within the spread nothing is done and rounding is relative to the larger row of the pair:
    factor = that magnitude over the row's own, at most 2^(SPREAD + 1).  Rows that are zero, not finite, or without a partner: 1."""
    top = np.asarray(top, dtype='f8')
    nbatch = top.shape[0]
    partner = np.arange(nbatch) ^ 1
    partner[partner >= nbatch] = nbatch - 1
    other = top[partner]
    ok = np.isfinite(top) & np.isfinite(other) & (top > 0) & (other > 0)
    field = lambda v: np.frexp(np.where(ok, v, 1.))[1]      # noqa: E731
    near = ok & (np.abs(field(top) - field(other)) <= SPREAD)
    with np.errstate(all='ignore'):
        return np.where(near, np.maximum(1., other / np.where(ok, top, 1.)), 1.)


class FusedBatch(object):
    """One batch of a fused case: rows (nbatch, nker, n) for the device, and for its answer ``got`` the pair (comparable(got, items), true[items])
    with the levels ``level`` of the float64 restatement and the factors ``factor`` of :func:`pair_factor`, each (nbatch, nker)."""


def fused_batch(n, npad, syn, extrap, keep_padding, kind, nbatch, table=None, seed=0):
    """Batch item i of kernel index ker is base row i % 2 times 2**exponents(nbatch, nker, table)[i, ker].  Padding that scales with the row
    (:func:`homogeneous`): truth and level once per (base row, kernel index), the device's rows are unscaled exactly before they are compared.
    A constant other than 0 does not scale: truth and level of every row as it is (such batches are kept small)."""
    b = FusedBatch()
    nker = syn.nker
    b.table = table
    b.rows = batch(base_rows(n, seed) if kind == 'dense' else log_rows(n, npad, seed, negative=kind == 'logneg'), nbatch, nker, table)
    b.top = np.stack([tilted_top(b.rows[:, ker], n, npad, syn.pre[ker], extrap) for ker in range(nker)], axis=1)
    b.factor = pair_factor(b.top)
    b.homogeneous = homogeneous(extrap)
    if b.homogeneous:
        base, true, level = base_case(n, npad, syn, extrap, keep_padding, seed, kind)
        b.true, b.level = expected(true, level, nbatch)
        scale = np.ldexp(LD(1), -exponents(nbatch, nker, table))[:, :, None]
        b.comparable = lambda got, items=slice(None): np.asarray(got)[items].astype(LD) * scale[items]      # noqa: E731  (unscaled exactly)
    else:
        true, level = [], []
        for ker in range(nker):
            t = truth(b.rows[:, ker], n, npad, syn.pre[ker], syn.post[ker], syn.taps[ker], extrap, keep_padding)
            true.append(t)
            level.append(levels(t, restated(b.rows[:, ker], n, npad, syn.pre[ker], syn.post[ker], syn.u[ker], extrap, keep_padding))[1])
        b.true, b.level = np.stack(true, axis=1), np.stack(level, axis=1)
        b.comparable = lambda got, items=slice(None): np.asarray(got)[items].astype(LD)      # noqa: E731
    return b


FUSED_NBATCH = 5      # two full pairs and one row without a partner, per kernel index


def fused_table(extrap, nbatch, nker):
    """The exponents of a case of the ladder: the module's EXPONENTS (pairs up to 2^600 apart) where the padding scales with the row, pairs 2^12
    apart (:func:`pair_table`) beside a padding constant of order one."""
    return None if homogeneous(extrap) else pair_table(nbatch, nker, 12)


def grid_bound(npad, compute_units):
    """An upper bound of any variant's grid: the device's CU count times min(32, floor(160 KiB / (16 Np)))."""
    return compute_units * max(1, min(32, (160 * 1024) // (16 * npad)))
