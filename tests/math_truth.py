"""Structured argument sets and ``np.longdouble`` truths for the short transcendental forms of csrc/cp_math.h (tests/test_math_truth_host.py through the
g++ emulation of the header, tests/test_math_edges_gpu.py through cp_math_eval).  Where tests/test_math_gpu.py draws uniformly, these sets sit where a
uniform draw essentially never lands: the ties of every argument reduction, the piece edges of the 64-entry tables, every wrap of ``n & 63``, the
hand-off thresholds, the arguments whose results are subnormal or leave the doubles, and the doubles next to the multiples of pi / 2.  Deterministic: no
random draw.

The bounds are those the header states (BOUNDS); a result is compared with the longdouble truth (64-bit mantissa: relative error 1e-19 for exp / log /
sin of a double; 10^x is the library's pow, see exp10_truth), never with the emulation or with a library's double result.
"""
import functools

import numpy as np

LD = np.longdouble
TINY = LD(2) ** -1074            # the unit of the subnormal results
DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308
LN2, LOG10_2, LN10, HALF_PI = np.log(LD(2)), np.log10(LD(2)), np.log(LD(10)), np.arctan(LD(1)) * 2
SUBNORMAL_UNITS = 2.             # |result - truth| / 2^-1074 of an exponential whose result is subnormal: the form's own rounding and that of ldexp

# What csrc/cp_math.h states, per form: relative error, but absolute error for sin_bounded and absolute error over max(1, |log x|) for log_tab.  "Below 1 ulp"
# (log_pos) and "below 2 ulp" (recip) are 2^-52 and 2^-51.  rsqrt_pos: the budget its comment writes out (half an ulp of the result, half of the half ulp
# of x y in e, the e^3 term of the series: 1.11e-16 + 0.56e-16 + 1e-20).
BOUNDS = {'exp_mid': 2e-16, 'exp_tab': 2.3e-16, 'exp10_mid': 2e-16, 'exp10_tab': 2.4e-16, 'log_pos': 2.0 ** -52, 'log_tab': 2e-16,
          'sin_bounded': 2e-16, 'recip': 2.0 ** -51, 'rsqrt_pos': 1.7e-16}
KINDS = {'exp_mid': 0, 'exp_tab': 1, 'log_pos': 2, 'log_tab': 3, 'exp10_mid': 4, 'exp10_tab': 5, 'sin_bounded': 6, 'recip': 7, 'rsqrt_pos': 8}      # enum cp_math_function


def frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


def around(c, k):
    """The doubles ``c`` and their k neighbours on each side, sorted, each once."""
    c = np.atleast_1d(np.asarray(c, dtype='f8'))
    out, up, dn = [c], c, c
    for _ in range(k):
        with np.errstate(over='ignore'):      # (beyond DBL_MAX: Inf, which the sets drop)
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        out += [up, dn]
    return np.unique(np.concatenate(out))


def ties(step, n0, n1, k=4):
    """The doubles next to (n + 1/2) step, n0 <= n <= n1 (the nearest one and k each side: at least four on each side of the tie)."""
    n = np.arange(n0, n1 + 1).astype(LD)
    return around(((n + LD(0.5)) * step).astype('f8'), k)


# ---- truths ----------------------------------------------------------------------------------------------------------------------------------------
def exp_truth(x):
    with np.errstate(over='ignore', under='ignore'):
        return np.exp(np.asarray(x, dtype='f8').astype(LD))


def exp10_truth(x):
    """pow(10, x) of the longdouble library, NOT e^(x ln 10): the rounding of ln 10 to 64 bits alone is 1e-19, times |x| = 300 an error of 3.7e-17 in the result,
    a sixth of the bounds held here (tests/test_math_truth_host.py compares both with 200-bit arithmetic)."""
    with np.errstate(over='ignore', under='ignore'):
        return np.power(LD(10), np.asarray(x, dtype='f8').astype(LD))


def log_truth(x):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.log(np.asarray(x, dtype='f8').astype(LD))


def sin_truth(x):
    return np.sin(np.asarray(x, dtype='f8').astype(LD))


def recip_truth(x):
    return 1 / np.asarray(x, dtype='f8').astype(LD)


def rsqrt_truth(x):
    return 1 / np.sqrt(np.asarray(x, dtype='f8').astype(LD))


TRUTH = {'exp_mid': exp_truth, 'exp_tab': exp_truth, 'exp10_mid': exp10_truth, 'exp10_tab': exp10_truth, 'log_pos': log_truth, 'log_tab': log_truth,
         'sin_bounded': sin_truth, 'recip': recip_truth, 'rsqrt_pos': rsqrt_truth}


# ---- exponentials ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exp_normal(name):
    """Arguments whose result is a normal double, finite: the ties of the form's reduction (for the table-driven forms every wrap of n & 63, at negative and
    positive n, lies between two of them), and for 10^x the integers."""
    if name == 'exp_mid':
        x = ties(LN2, -1022, 1023)
    elif name == 'exp_tab':
        x = ties(LN2 / 64, -1022 * 64, 1023 * 64 + 63)
    elif name == 'exp10_mid':
        x = np.concatenate([ties(LOG10_2, -1022, 1023), ties(LOG10_2 / 64, -63781, 63780), np.arange(-299., 300.)])
    else:
        x = np.concatenate([ties(LOG10_2, -996, 995), ties(LOG10_2 / 64, -63781, 63780), np.arange(-299., 300.), around(np.nextafter(300., 0.), 4)])
        x = x[np.abs(x) < 300.]
    truth = TRUTH[name](x)
    keep = (truth >= LD(DBL_MIN)) & (truth < LD(DBL_MAX) * (1 - LD(1e-15)))
    return frozen(np.unique(x[keep]))


@functools.lru_cache(maxsize=None)
def exp_subnormal(name):
    """Arguments whose result is subnormal (or rounds to 0 below 2^-1075): a regular sweep and the ties of the reduction there."""
    if name in ('exp_mid', 'exp_tab'):
        x = np.concatenate([np.linspace(-745.2, -708.4, 4001), ties(LN2, -1076, -1023), around([-745.2, -745.13321910194122, -744.44007192138122, -708.4], 4)])
        return frozen(x[(x > -745.3) & (x < -708.397)])
    x = np.concatenate([np.linspace(-323.4, -307.7, 4001), ties(LOG10_2, -1076, -1023), around([-324., -323.60724533877976, -323.30621534311581], 4)])
    return frozen(x[(x >= -324.) & (x < -307.66)])


def exp_beyond(name):
    """(x, expected): arguments whose result leaves the doubles, with the exact answer the header promises (0, Inf, NaN)."""
    inf, nan = np.inf, np.nan
    if name in ('exp_mid', 'exp_tab'):
        over = around(709.78271289338397, 4)
        over = over[exp_truth(over) > LD(DBL_MAX) * (1 + LD(1e-15))]      # (every neighbour is 1e-13 away in the result: none in the round-off of the threshold)
        x = np.concatenate([[-746., -800., -1e4, -inf, 709.79, 710., 711., 1e4, nan], over])
        e = np.concatenate([[0., 0., 0., 0., inf, inf, inf, inf, nan], np.full(over.size, inf)])
        if name == 'exp_mid':
            x, e = np.append(x, inf), np.append(e, inf)
        return x, e
    assert name == 'exp10_mid'
    over = np.concatenate([around(308.25471555991675, 4), around(308.3, 4), [308.26, 308.29]])
    over = over[exp10_truth(over) > LD(DBL_MAX) * (1 + LD(1e-15))]
    under = np.concatenate([around(-324., 4)[:4], around(-1100 * float(LOG10_2), 4), [-325., -400., -1e300, -inf]])
    big = np.concatenate([around(1100 * float(LOG10_2), 4), [309., 400., 1e300, inf]])
    x = np.concatenate([under, over, big, [nan]])
    return x, np.concatenate([np.zeros(under.size), np.full(over.size + big.size, inf), [nan]])


# ---- logarithms ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def log_arguments():
    """Positive, finite, normal arguments: the doubles around every piece edge of log_tab at eight binary exponents, around sqrt(1/2) and sqrt(2) (the fold
    of log_pos), 1 +- 2^-k, every power of two, and the two ends of the normal doubles."""
    edges = 0.5 + np.arange(64) / 128.
    x = [around(np.ldexp(edges, e), 3) for e in (-1021, -500, -1, 0, 1, 2, 500, 1023)]
    x += [around([np.sqrt(0.5), np.sqrt(2.), 1.], 4), 1. + np.ldexp(1., -np.arange(1, 53)), 1. - np.ldexp(1., -np.arange(1, 53))]
    x += [np.ldexp(1., np.arange(-1022, 1024)), around([DBL_MIN, DBL_MAX], 3)]
    x = np.unique(np.concatenate(x))
    return frozen(x[(x >= DBL_MIN) & (x <= DBL_MAX)])


LOG_OUTSIDE = np.array([0., -0., -1., 5e-324, 1e-310, np.nextafter(DBL_MIN, 0.), np.inf, -np.inf, np.nan])      # the library's answers


# ---- sine ------------------------------------------------------------------------------------------------------------------------------------------
SIN_NMAX = 636000                # 636000 pi / 2 = 999026 < 1e6


@functools.lru_cache(maxsize=None)
def sin_arguments(thin=True):
    """The doubles within 2 ulps of n pi / 2 (thin: every 37th n and all |n| < 4096; else every |n| <= 636000: 6.4e6 arguments), the ties of
    rint(x 2 / pi) on the same n, the doubles next to +-1e6 below the hand-off to the library, and +-0."""
    n = np.arange(-SIN_NMAX, SIN_NMAX + 1)
    if thin:
        n = n[(n % 37 == 0) | (np.abs(n) < 4096)]
    nl = n.astype(LD)
    x = [around((nl * HALF_PI).astype('f8'), 2), around(((nl + LD(0.5)) * HALF_PI).astype('f8'), 2), [0., -0.]]
    x = np.concatenate(x)
    x = np.concatenate([x[np.abs(x) < 1e6], sin_below_handoff()])
    return frozen(x)


def sin_below_handoff():
    a = around(1e6, 4)
    a = a[a < 1e6]
    return np.concatenate([a, -a])


def sin_handoff():
    """+-1e6 and the four doubles beyond: the library's sine."""
    a = around(1e6, 4)
    a = a[a >= 1e6]
    return np.concatenate([a, -a])


# ---- reciprocal and root ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def powers_of_two():
    return frozen(np.ldexp(1., np.arange(-1022, 1023)))


@functools.lru_cache(maxsize=None)
def recip_arguments():
    """Every power of two 2^-1022 ... 2^1022 and three neighbours each side of every seventh (normal, with a normal reciprocal), of both signs for recip."""
    p = powers_of_two()
    x = np.unique(np.concatenate([p, around(p[3:-3:7], 3)]))
    return frozen(x[(x >= DBL_MIN) & (x <= np.ldexp(1., 1022))])


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------------
def ulp(x):
    x = np.abs(np.asarray(x, dtype='f8'))
    return np.nextafter(x, np.inf) - x


def exp2_table_truth():
    return np.exp2(np.arange(64).astype(LD) / 64)


def log_table_truth(table):
    """(1 / c_j, -log of the ROUNDED reciprocal the table holds beside it), c_j = (129 + 2 j) / 256."""
    inv = LD(256) / (129 + 2 * np.arange(64)).astype(LD)
    return inv, -np.log(np.asarray(table, dtype='f8')[0::2].astype(LD))


def half_ulp_off(table, truth):
    """|table - truth| in ulps of the table's entries: a correctly rounded entry is at most 1/2 (+ the 2^-11 ulp of the longdouble truth)."""
    table = np.asarray(table, dtype='f8')
    return np.asarray(np.abs(table.astype(LD) - truth) / ulp(table).astype(LD), dtype='f8')


# ---- measures --------------------------------------------------------------------------------------------------------------------------------------
def relative(got, truth):
    got = np.asarray(got, dtype='f8').astype(LD)
    exact = (truth == 0) & (got == 0)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.asarray(np.where(exact, 0, np.abs((got - truth) / truth)), dtype='f8')


def absolute(got, truth):
    return np.asarray(np.abs(np.asarray(got, dtype='f8').astype(LD) - truth), dtype='f8')


def log_tab_error(got, truth):
    return np.asarray(np.abs(np.asarray(got, dtype='f8').astype(LD) - truth) / np.maximum(1, np.abs(truth)), dtype='f8')


def units(got, truth):
    """|got - truth| in units of 2^-1074."""
    return np.asarray(np.abs(np.asarray(got, dtype='f8').astype(LD) - truth) / TINY, dtype='f8')


def same(got, expected):
    """Equal entry by entry, NaN equal to NaN, the sign of a zero left aside."""
    return np.array_equal(np.asarray(got, dtype='f8'), np.asarray(expected, dtype='f8'), equal_nan=True)


# ---- the checks, for any evaluator ev(name, x) -> float64 array (the emulation on the host, cp_math_eval on the device) -------------------------------
def check_exponential(name, ev, who):
    """The contract of one exponential on its sets; returns (worst relative error, worst subnormal error in units of 2^-1074 or None)."""
    x = exp_normal(name)
    rel = relative(ev(name, x), TRUTH[name](x))
    print('%s %s: %d arguments with normal results, worst relative error %.4g at x = %r (stated %.3g)' % (who, name, x.size, rel.max(), float(x[rel.argmax()]), BOUNDS[name]))
    assert rel.max() < BOUNDS[name], (name, float(rel.max()), float(x[rel.argmax()]))
    if name == 'exp10_tab':      # (no range handling: the caller's)
        return float(rel.max()), None
    x = exp_subnormal(name)
    got = ev(name, x)
    u = units(got, TRUTH[name](x))
    print('%s %s: %d arguments with subnormal results, worst error %.4g units of 2^-1074 at x = %r' % (who, name, x.size, u.max(), float(x[u.argmax()])))
    assert u.max() <= SUBNORMAL_UNITS and (got >= 0).all() and (got < DBL_MIN * 1.0001).all(), (name, float(u.max()))
    x, expected = exp_beyond(name)
    got = ev(name, x)
    assert same(got, expected), (name, [(float(a), float(b), float(c)) for a, b, c in zip(x, got, expected) if not (b == c or (b != b and c != c))])
    assert same(ev(name, [0., -0.]), [1., 1.])
    return float(rel.max()), float(u.max())


def check_logarithms(ev, who):
    """log_pos (relative) and log_tab (absolute over max(1, |log x|)) on log_arguments, exactly 0 at 1, the library's answers outside the domain."""
    x = log_arguments()
    truth = log_truth(x)
    got = ev('log_pos', x)
    rel = relative(got, truth)
    print('%s log_pos: %d arguments, worst relative error %.4g at x = %r (stated %.3g)' % (who, x.size, rel.max(), float(x[rel.argmax()]), BOUNDS['log_pos']))
    assert rel.max() < BOUNDS['log_pos'] and got[x == 1.][0] == 0.
    got = ev('log_tab', x)
    err = log_tab_error(got, truth)
    print('%s log_tab: worst absolute error over max(1, |log x|) %.4g at x = %r (stated %.3g)' % (who, err.max(), float(x[err.argmax()]), BOUNDS['log_tab']))
    assert err.max() < BOUNDS['log_tab']
    away = np.abs(truth) >= 1
    assert relative(got[away], truth[away]).max() < BOUNDS['log_tab']
    for name in ('log_pos', 'log_tab'):
        out = ev(name, LOG_OUTSIDE)
        assert out[0] == -np.inf and out[1] == -np.inf and np.isnan(out[2]) and out[6] == np.inf and np.isnan(out[7]) and np.isnan(out[8]), (name, out)
        assert relative(out[3:6], log_truth(LOG_OUTSIDE[3:6])).max() < 2.0 ** -52, (name, out)      # subnormal arguments: the library's logarithm
    return float(rel.max()), float(err.max())


def check_sine(ev, who, thin=True):
    x = sin_arguments(thin)
    got = ev('sin_bounded', x)
    err = absolute(got, sin_truth(x))
    print('%s sin_bounded: %d arguments, worst absolute error %.4g at x = %r (stated %.3g)' % (who, x.size, err.max(), float(x[err.argmax()]), BOUNDS['sin_bounded']))
    assert err.max() < BOUNDS['sin_bounded'] and (np.abs(got) <= 1.).all()
    x = sin_handoff()
    assert relative(ev('sin_bounded', x), sin_truth(x)).max() < 2.0 ** -52      # |x| >= 1e6: the library's sine
    zero = ev('sin_bounded', [0., -0.])
    assert zero[0] == 0. and zero[1] == 0. and not np.signbit(zero[0])
    print('%s sin_bounded(-0.) = %s0 (known deviation: the product r z of the series loses the sign of a zero)' % (who, '-' if np.signbit(zero[1]) else '+'))
    return float(err.max())


def check_reciprocal_root(ev, who):
    x = recip_arguments()
    xs = np.concatenate([x, -x])
    rel = relative(ev('recip', xs), recip_truth(xs))
    print('%s recip: %d arguments, worst relative error %.4g at x = %r (stated %.3g)' % (who, xs.size, rel.max(), float(xs[rel.argmax()]), BOUNDS['recip']))
    assert rel.max() < BOUNDS['recip']
    rel2 = relative(ev('rsqrt_pos', x), rsqrt_truth(x))
    print('%s rsqrt_pos: %d arguments, worst relative error %.4g at x = %r (stated %.3g)' % (who, x.size, rel2.max(), float(x[rel2.argmax()]), BOUNDS['rsqrt_pos']))
    assert rel2.max() < BOUNDS['rsqrt_pos']
    p = powers_of_two()
    even = p[::2]
    print('%s recip: %d of %d reciprocals of powers of two exact; rsqrt_pos: %d of %d roots of even powers exact; recip(DBL_MAX) = %r (true 5.562684646268003e-309, subnormal: no promise)'
          % (who, int((ev('recip', p) == 1. / p).sum()), p.size, int((ev('rsqrt_pos', even) == 1. / np.sqrt(even)).sum()), even.size, float(ev('recip', [DBL_MAX])[0])))
    return float(rel.max()), float(rel2.max())
