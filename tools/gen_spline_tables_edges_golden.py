"""Fixture of the edge cases of cp_spline_tables (csrc/cp_spline_tables.hip): tests/golden/spline_tables_edges.npz, the natural cubic spline and the
linear interpolant of every case of tests/spline_tables_cases.py evaluated in extended precision (numpy only; no test imports this file).

    python tools/gen_spline_tables_edges_golden.py [--check-only]

Truth.  scipy's ``CubicSpline(bc_type='natural')`` solves in float64 and is itself off by 3e2 - 5e4 tolerances on tables whose spacings jump by factors
of 4^19, so it cannot be the yardstick here.  The truth is the same system -- 2 s_0 + s_1 = 3 slope_0; dx_i s_{i-1} + 2 (dx_{i-1} + dx_i) s_i +
dx_{i-1} s_{i+1} = 3 (dx_i slope_{i-1} + dx_{i-1} slope_i); s_{n-2} + 2 s_{n-1} = 3 slope_{n-2} -- solved by the Thomas algorithm over the whole row
in ``np.longdouble`` (64-bit mantissa required: asserted), and the piecewise polynomial evaluated in longdouble, rounded to float64 once.

Stored per size n: ``q_<n>`` (families, NQ) the queries of every family and ``t<order>_<n>`` their truths; ``qs_<n>`` (NQ_SHARED,) the queries shared
by the families and ``ts<order>_<n>`` (families, NQ_SHARED).  The knots are not stored: the test rebuilds them from tests/spline_tables_cases.py.

Condition on the inputs (not a measurement of the kernel).  ``emulate_build`` is the kernel's own scheme in numpy float64, recurrence by recurrence:
every lane eliminates from ``halo`` knots below its run and from ``halo`` knots above it as if the spline began / ended there.  With the halo that the
kernel ships (TAB_HALO, read from the source) every committed case must lie within 0.25 of the tolerance of the truth, which leaves a factor 4 for what the
device does differently in the last bits (contracted multiply-adds, its division).  The table printed at the end shows the same figure for other halos."""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import spline_tables_cases as stc  # noqa: E402

LD = np.longdouble
CONDITION = 0.25


def shipped_halo():
    with open(os.path.join(ROOT, 'cosmoprimo_amd', 'csrc', 'cp_spline_tables.hip')) as file:
        return int(re.search(r'constexpr int TAB_HALO = (\d+);', file.read()).group(1))


def interval_of(x, q):
    """The interval the kernels evaluate a query in: the last knot <= q, the last interval for the last knot."""
    return np.clip(np.searchsorted(x, q, side='right') - 1, 0, len(x) - 2)


def truth_cubic(x, y, q):
    n = len(x)
    k = interval_of(x, q)
    x, y, q = x.astype(LD), y.astype(LD), q.astype(LD)
    dx = np.diff(x)
    sl = np.diff(y) / dx
    lower, diag, upper, rhs = (np.zeros(n, dtype=LD) for _ in range(4))
    diag[0], upper[0], rhs[0] = 2, 1, 3 * sl[0]
    for i in range(1, n - 1):
        lower[i], diag[i], upper[i], rhs[i] = dx[i], 2 * (dx[i - 1] + dx[i]), dx[i - 1], 3 * (dx[i] * sl[i - 1] + dx[i - 1] * sl[i])
    lower[n - 1], diag[n - 1], rhs[n - 1] = 1, 2, 3 * sl[-1]
    for i in range(1, n):
        w = lower[i] / diag[i - 1]
        diag[i] -= w * upper[i - 1]
        rhs[i] -= w * rhs[i - 1]
    s = np.zeros(n, dtype=LD)
    s[-1] = rhs[-1] / diag[-1]
    for i in range(n - 2, -1, -1):
        s[i] = (rhs[i] - upper[i] * s[i + 1]) / diag[i]
    h = dx[k]
    t = (s[k] + s[k + 1] - 2 * sl[k]) / h
    u = q - x[k]
    return (y[k] + u * (s[k] + u * ((sl[k] - s[k]) / h - t + u * (t / h)))).astype('f8')


def truth_linear(x, y, q):
    k = interval_of(x, q)
    x, y, q = x.astype(LD), y.astype(LD), q.astype(LD)
    return (y[k] + (q - x[k]) * ((y[k + 1] - y[k]) / (x[k + 1] - x[k]))).astype('f8')


def emulate_build(xs, ys, halo):
    """spline_tables_build_kernel for order 3, lane by lane, in float64: the (n - 1, 4) coefficients as the kernel stores them."""
    n = len(xs)
    run = stc.table_run(n)
    coef = np.full((n - 1, 4), np.nan)
    cs, ds = np.zeros(n), np.zeros(n)
    for lane in range(64):
        a = lane * run
        b = min(a + run, n - 1)
        if a >= b:
            continue
        f0, f1 = max(a - halo, 0), min(b + halo, n - 1)
        dxm = xs[f0 + 1] - xs[f0]
        slm = (ys[f0 + 1] - ys[f0]) / dxm
        c, d = 0.5, 1.5 * slm
        if f0 >= a:
            cs[f0], ds[f0] = c, d
        for i in range(f0 + 1, b):
            dxp = xs[i + 1] - xs[i]
            slp = (ys[i + 1] - ys[i]) / dxp
            inv = 1. / (2. * (dxm + dxp) - dxp * c)
            c, d = dxm * inv, (3. * (dxp * slm + dxm * slp) - dxp * d) * inv
            if i >= a:
                cs[i], ds[i] = c, d
            dxm, slm = dxp, slp
        dxp = xs[f1] - xs[f1 - 1]
        slp = (ys[f1] - ys[f1 - 1]) / dxp
        e, g = 0.5, 1.5 * slp
        for i in range(f1 - 1, b - 1, -1):
            dxl = xs[i] - xs[i - 1]
            sll = (ys[i] - ys[i - 1]) / dxl
            inv = 1. / (2. * (dxl + dxp) - dxl * e)
            e, g = dxp * inv, (3. * (dxp * sll + dxl * slp) - dxl * g) * inv
            dxp, slp = dxl, sll
        s_hi = (g - e * ds[b - 1]) / (1. - e * cs[b - 1])
        for k in range(b - 1, a - 1, -1):
            s_lo = ds[k] - cs[k] * s_hi
            h = xs[k + 1] - xs[k]
            slope = (ys[k + 1] - ys[k]) / h
            t = (s_lo + s_hi - 2. * slope) / h
            if k == n - 2:      # the last interval holds the values of both its knots (table_last of the kernel)
                dy = ys[k + 1] - ys[k]
                A = h * s_lo - dy
                coef[k] = [ys[k], A, (dy - h * s_hi) - A, ys[k + 1]]
            else:
                coef[k] = [ys[k], s_lo, (slope - s_lo) / h - t, t / h]
            s_hi = s_lo
    return coef


def emulate_apply(xs, coef, q):
    k = interval_of(xs, q)
    u, c = q - xs[k], coef[k]
    t = u / (xs[-1] - xs[-2])
    last = (1. - t) * c[:, 0] + t * c[:, 3] + t * (1. - t) * (c[:, 1] + t * c[:, 2])
    return np.where(k == len(xs) - 2, last, c[:, 0] + u * (c[:, 1] + u * (c[:, 2] + u * c[:, 3])))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--check-only', action='store_true', help='print the table of the condition and write nothing')
    args = parser.parse_args()
    assert np.finfo(LD).eps <= 2.**-63, 'np.longdouble is no wider than float64 on this platform: no extended-precision truth here'
    halo = shipped_halo()
    halos = sorted(set([8, 16, 24, 32, 40, 48, 64, 10**6, halo]))
    out, worst, failures = {}, {}, []
    for n in stc.SIZES + stc.LARGE_SIZES:
        names = stc.families(n)
        y = stc.zgrid(n)
        qs = stc.shared_queries(n)
        q = np.array([stc.queries(name, n) for name in names])
        out['q_%d' % n], out['qs_%d' % n] = q, qs
        for order, truth in ((3, truth_cubic), (1, truth_linear)):
            out['t%d_%d' % (order, n)] = np.array([truth(stc.knots(name, n), y, q[i]) for i, name in enumerate(names)])
            out['ts%d_%d' % (order, n)] = np.array([truth(stc.knots(name, n), y, qs) for name in names])
        for i, name in enumerate(names):
            x = stc.knots(name, n)
            for h in halos:
                coef = emulate_build(x, y, h)
                err = max(stc.excess(emulate_apply(x, coef, q[i]), out['t3_%d' % n][i]), stc.excess(emulate_apply(x, coef, qs), out['ts3_%d' % n][i]))
                worst[name, h] = max(worst.get((name, h), 0.), err)
                worst[n, h] = max(worst.get((n, h), 0.), err)
                if h == halo and not err <= CONDITION:
                    failures.append('(%s, n = %d): %.3g' % (name, n, err))
    print('float64 emulation of the build against the truth, largest |d| / (1e-13 + 1e-11 |truth|) over the cases (shipped TAB_HALO = %d, condition <= %.2f)' % (halo, CONDITION))
    print('%-10s' % 'halo' + ''.join('%10s' % ('full' if h == 10**6 else h) for h in halos))
    for key in stc.FAMILIES + stc.SIZES + stc.LARGE_SIZES:
        print('%-10s' % (key if isinstance(key, str) else 'n = %d' % key) + ''.join('%10.2e' % worst[key, h] for h in halos))
    smallest = min(h for h in halos if h % 8 == 0 and all(worst[name, h] <= CONDITION for name in stc.FAMILIES))
    print('smallest multiple of 8 that meets the condition on every case: %d' % smallest)
    assert not failures, 'with TAB_HALO = %d these cases are further than %.2f of the tolerance from the truth, outside the guarantee: %s' % (halo, CONDITION, ', '.join(failures))
    if args.check_only:
        return
    path = os.path.join(ROOT, 'tests', 'golden', 'spline_tables_edges.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1e3))


if __name__ == '__main__':
    main()
