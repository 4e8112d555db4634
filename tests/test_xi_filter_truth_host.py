"""CPU: the longdouble truth of tests/xi_filter_truth.py against the same filter in mpmath at 40 digits and against ``oracle.bao.kirkby2013``, the
float64 restatement's equivariance under 2^e, and the two conditions every case of tests/test_xi_filter_edges_gpu.py rests on: a level of at most
1e-10, and a truth that moves by at least 100 allowances when any one fit sample of weight >= 0.5 is left out (``xi_filter_truth.drop_one``)."""
import mpmath
import numpy as np
import pytest

import xi_filter_truth as xt
from oracle import bao as obao


def close(a, b, rtol=1e-9):
    """The convention of test_xi_filter_batch_gpu.py."""
    b = np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-12 * np.nanmax(np.abs(b)), equal_nan=True)


def _mp_of(v):
    """A longdouble as mpf, exactly: its float64 rounding and the rest."""
    hi = np.float64(v)
    return mpmath.mpf(float(hi)) + mpmath.mpf(float(v - xt.LD(hi)))


def _mp_interp(x, xp, fp):
    n = len(xp)
    j = sum(1 for k in xp if x >= k) - 1
    if j < 0 or (j == n - 1 and x != xp[-1]):
        return mpmath.mpf(0)
    if j == n - 1:
        return fp[-1]
    return fp[j] + (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j])


def mp_filter(s, xi, rho, fit, knots, weights):
    """One row at 40 digits: the normal equations of the powers (s / 128)^(1 - j) by mpmath.lu_solve; x the float64 quotient."""
    mp = mpmath.mpf
    x = [mp(float(v)) for v in xt.x_of(s, rho)]
    k, w8 = [mp(float(v)) for v in knots], [mp(float(v)) for v in weights]
    c4 = [mp(float(v)) for v in 1. - np.asarray(weights)[2:6]]
    power = lambda si, j: (mp(float(si)) / 128)**(1 - j)      # noqa: E731
    G, R = mpmath.zeros(5, 5), mpmath.zeros(5, 1)
    for i in range(*fit):
        w = _mp_interp(x[i], k, w8)
        g = [power(s[i], j) for j in range(5)]
        for a in range(5):
            R[a] += w * mp(float(xi[i])) * g[a]
            for b in range(5):
                G[a, b] += w * g[a] * g[b]
    p = mpmath.lu_solve(G, R)
    out = []
    for i in range(len(s)):
        c = _mp_interp(x[i], k[2:6], c4)
        out.append((1 - c) * mp(float(xi[i])) + c * sum(p[j] * power(s[i], j) for j in range(5)))
    return out


@pytest.mark.parametrize('which', ['ns6', 'ns16', 'ns1024', 'edges'])
def test_truth_against_mpmath(which):
    """The distance of the longdouble truth from 40 digits, over the blended samples and relative to their scale: at most 1 / 100 of the case's level."""
    case = {'ns6': lambda: xt.size_case(6), 'ns16': lambda: xt.size_case(16), 'ns1024': lambda: xt.size_case(1024), 'edges': lambda: xt.edge_case(False, True)}[which]()
    picks = [(0, 5)] if which == 'ns1024' else [(r, b) for r in range(len(case.ratios)) for b in (0, 4)]
    worst = 0.
    with mpmath.workprec(140):      # 42 digits
        for r, b in picks:
            exact = mp_filter(case.s, case.base[b], case.ratios[r], case.fit, case.knots, case.weights)
            blend = np.flatnonzero(case.blend[r])
            dist = max(abs(_mp_of(case.truth[r, b, i]) - exact[i]) for i in blend)
            worst = max(worst, float(dist / mpmath.mpf(float(case.top[r, b]))))
    print('%s: truth %.3g of the blended scale from 40 digits, level %.3g' % (case.label, worst, case.level))
    assert worst <= case.level / 100.


@pytest.mark.parametrize('ns', [128, 1023, 1024])
def test_truth_against_the_oracle(ns):
    """Default window, the filter's fit range: the raw-power normal equations of the oracle, within the convention of the batch tests."""
    case = xt.size_case(ns)
    for r, rho in enumerate(case.ratios):
        close(case.truth[r].astype('f8').T, obao.kirkby2013(case.s, case.base.T, rescale=rho))


def test_restatement_follows_the_kernel_orders():
    """64 lane-strided partials and the tree against a sum written out lane by lane; sequential against a loop."""
    rng = np.random.default_rng(5)
    a = rng.standard_normal((150, 3))
    lanes = [sum((a[i] for i in range(l, 150, 64)), np.zeros(3)) for l in range(64)]
    for mask in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ mask] for l in range(64)]
    assert np.array_equal(xt._sum(a, 0, 'wave'), lanes[0])
    total = np.zeros(3)
    for row in a:
        total = total + row
    assert np.array_equal(xt._sum(a, 0, 'sequential'), total)


@pytest.mark.parametrize('order', xt.ORDERS)
def test_restatement_is_equivariant(order):
    """xi times 2^e gives the restatement times 2^e bit for bit, in both summation orders (the device tests unscale their rows on this ground)."""
    for case in (xt.size_case(16), xt.size_case(130), xt.edge_case(True, True)):
        nrows = 23
        scale = np.ldexp(1., xt.exponents(nrows))[:, None]
        rows = xt.batch(case.base, nrows)
        for rho in case.ratios:
            plain = xt.restated(case.s, case.base, rho, *case.fit, case.knots, case.weights, order=order)[np.arange(nrows) % xt.NBASE]
            scaled = xt.restated(case.s, rows, rho, *case.fit, case.knots, case.weights, order=order)
            assert np.array_equal(scaled, plain * scale)
            assert np.array_equal(scaled / scale, plain)


def test_interp_is_np_interp():
    xp, fp = xt.KNOTS, xt.GENERAL
    x = np.concatenate([xp, np.nextafter(xp, np.inf), np.nextafter(xp, -np.inf), np.linspace(40., 200., 57), [np.nan, 0., 1e300]])
    ours = xt.interp(x, xp, fp, dtype=np.float64)
    ref = np.interp(x, xp, fp, left=0., right=0.)
    assert np.array_equal(np.isnan(ours), np.isnan(ref)) and np.isnan(ours).sum() == 1
    np.testing.assert_allclose(ours, ref, rtol=0, atol=2e-16, equal_nan=True)
    exact = xt.interp(xp, xp, fp)
    assert np.array_equal(exact.astype('f8'), fp) and xt.interp(np.nextafter(xp[-1:], np.inf), xp, fp)[0] == 0 and xt.interp(np.nextafter(xp[:1], 0.), xp, fp)[0] == 0


def test_non_finite_rows_of_the_truth():
    """0 x NaN is NaN: a NaN or inf at a fit sample of weight 0, a NaN ratio and a ratio without weighted samples make the row NaN; a NaN outside
    the fit range and the blend stays alone."""
    case = xt.many_case(16)
    b, e = case.fit
    w, c = xt.window_of(case.s, 1., case.knots, case.weights)
    unweighted = b + int(np.flatnonzero((w[b:e] == 0) & (c[b:e] == 0))[0])
    for bad in (np.nan, np.inf):
        row = case.base[0].copy()
        row[unweighted] = bad
        assert np.isnan(xt.truth(case.s, row, 1., b, e)).all()
    row = case.base[0].copy()
    assert b == 1 and c[0] == 0
    row[0] = np.nan
    out = xt.truth(case.s, row, 1., b, e)
    assert np.isnan(out[0]) and np.isfinite(out[1:]).all()
    assert np.isnan(xt.truth(case.s, case.base[0], np.nan, b, e)).all()
    assert np.isnan(xt.truth(case.s, case.base[0], 100., b, e)).all()
    for order in xt.ORDERS:
        assert np.isnan(xt.restated(case.s, case.base[0], 100., b, e, order=order)).all()


def test_device_cases():
    """Every case of the device tests: level at most 1e-10; one fit sample of weight >= 0.5 less moves the truth by 100 allowances or more; the
    lists keep at least five weighted samples at each of their ratios."""
    assert xt.CAP == 1e-10 and xt.ALLOW == 16. and xt.FLOOR == 1.1e-16
    cases = xt.device_cases()
    for case in cases:
        moved = xt.drop_one(case)
        weighted = min(int((xt.window_of(case.s, rho, case.knots, case.weights)[0][case.fit[0]:case.fit[1]] > 0).sum()) for rho in case.ratios)
        print('%-55s level %.3g, one fit sample less moves the truth by at least %.3g allowances, %d weighted samples or more' % (case.label, case.level, moved, weighted))
        assert case.level <= xt.CAP, case.label
        assert moved >= 100., case.label
        assert weighted >= 5, case.label
    assert not xt.size_case(5).blend.any() and all(case.blend.any() for case in cases if case.ns != 5)
    # the cases stand where they are meant to: knots hit exactly, margin samples with blend factor 0, ranges that cut a box or end between the boxes
    edge = xt.edge_case(False, True)
    for r, rho in enumerate(edge.ratios[:3]):
        x = xt.x_of(edge.s, rho)
        for k in xt.KNOTS:
            assert (x == k).sum() == 1 and (x == np.nextafter(k, np.inf)).sum() == 1 and (x == np.nextafter(k, -np.inf)).sum() == 1
        margin = ((x < xt.KNOTS[2]) & (x >= xt.KNOTS[2] * (1. - 1e-12))) | ((x > xt.KNOTS[5]) & (x <= xt.KNOTS[5] * (1. + 1e-12)))
        assert margin.sum() >= 4 and edge.zero[r][margin].all() and not edge.blend[r][margin].any()
    for begin, length in xt.RANGES:
        case = xt.range_case(begin, length)
        w = xt.window_of(case.s, 1., case.knots, case.weights)[0]
        assert w[begin + length - 1] == 1 and (begin + length == case.ns or w[begin + length] == 1)      # the range cuts the right box
    for begin, length in xt.RANGES_SHORT:
        case = xt.range_case_short(begin, length)
        assert case.blend[0][begin + length:].sum() >= 3 and case.blend[0][begin:begin + length].sum() >= 4
