"""CPU: tests/spline_truth.py, the longdouble truth of the halo-truncated spline kernels, before the device tests rely on it.
(a) against ``scipy.interpolate.CubicSpline`` for the three end conditions, values (inside and with the end cubics continued) and second
derivatives: 1e-13 and 1e-12 of the row's largest entry (1e-10 and 1e-9 on ``alt1e3``, whose spacing ratio of 1e3 costs scipy's banded float64
solve three digits); this check is there to catch a wrong equation, the next one to hold the digits;
(b) against the spline's defining conditions evaluated in longdouble: the cubic of every interval ends on the next knot's value, the second
derivative is continuous at every interior knot, and the end condition holds -- to 32 longdouble ulps of the row's largest term of each expression;
(c) the rounding level of the float64 restatement, at most CAP = 32 x FLOOR for every (family, size, end condition, output) that
test_spline_rows_edges_gpu.py, test_spline_columns_gpu.py and test_gap_spline_gpu.py use, as tests/test_jvp_host.py does for its cases.  What is over
the cap is listed in ``spline_truth.ROWS_OVER_CAP`` and not used on the device; this test also holds every entry of that list to being over the cap,
so that the list cannot outlive its reason;
(d) the restated plan of the rows kernel (``rows_halo``, ``rows_layout``) at the values the issue of the kernel's design quotes.
Measured: the truth 2 to 4 longdouble ulps from its defining conditions; levels of the cases in use at most 30 FLOOR (rows), 19.3 (columns), 17.1 (gap).
Over the cap, with their levels, in ``spline_truth.ROWS_OVER_CAP`` and beside ``spline_truth.COLUMN_FAMILIES``: all second derivatives and the not-a-knot
values of ``alt1e3`` (1352 to 5682 FLOOR), ``sigma_r`` with fewer than 10 knots (up to 1822), four single not-a-knot second-derivative cases (32.8 to
91.1), and for the columns ``alt1e3`` (34), ``jitter100`` (36.3), ``saw1.5x16`` (32.9).  ``saw2x40`` stays within the cap everywhere."""
import numpy as np
import pytest
from scipy import interpolate

import spline_truth as st

LD = np.longdouble
EPS = float(np.finfo(LD).eps)
SMALL = [5, 8, 9, 40, 433]


@pytest.mark.parametrize('bc', st.BCS)
def test_truth_against_scipy(bc):
    worst = [0., 0., 0.]
    for n in SMALL:
        for name in st.families(n):
            x, y = st.knots(name, n), st.base_rows(name, n)
            s = st.slopes(x, y, bc)
            assert s.dtype == LD and s.shape == y.shape
            xq = st.rows_queries(x)
            tol_v, tol_m = (1e-10, 1e-9) if name == 'alt1e3' else (1e-13, 1e-12)
            ref = interpolate.CubicSpline(x, y, axis=-1, bc_type=bc)
            for k, (got, want, tol) in enumerate([(st.evaluate(x, y, s, xq), ref(xq), tol_v), (st.evaluate(x, y, s, st.rows_beyond(x), True), ref(st.rows_beyond(x)), tol_v),
                                                  (st.second_derivatives(x, y, s), ref(x, nu=2), tol_m)]):
                assert np.array_equal(np.isnan(got), np.isnan(want))
                d = float((np.nanmax(np.abs(got - want), axis=-1) / np.nanmax(np.abs(want), axis=-1)).max())
                worst[k] = max(worst[k], d)
                assert d <= tol, (name, n, k, d)
            outside = st.evaluate(x, y, s, st.rows_beyond(x), False)
            assert np.isnan(outside[:, :3]).all() and np.isnan(outside[:, -3:]).all() and np.isnan(outside).sum() == 7 * len(y)
    print('%s: values %.3g, continued %.3g, second derivatives %.3g from scipy' % (bc, *worst))


@pytest.mark.parametrize('bc', st.BCS)
def test_truth_defining_conditions(bc):
    tol = 32. * EPS
    worst = 0.
    for n in SMALL + [1889]:
        for name in st.families(n):
            x, y = st.knots(name, n).astype(LD), st.base_rows(name, n).astype(LD)
            s = st.slopes(x, y, bc)
            h = np.diff(x)
            delta = np.diff(y, axis=-1) / h
            c2 = (3 * delta - 2 * s[:, :-1] - s[:, 1:]) / h
            c3 = (s[:, :-1] + s[:, 1:] - 2 * delta) / h**2
            # interpolation: the cubic of interval j, taken to its upper end, arrives at y_{j+1}
            end = y[:, :-1] + h * (s[:, :-1] + h * (c2 + h * c3))
            scale = (np.abs(y[:, :-1]) + h * (np.abs(s[:, :-1]) + np.abs(s[:, 1:]) + np.abs(delta))).max(axis=-1)
            r = [np.abs(end - y[:, 1:]).max(axis=-1) / scale]
            # continuity of the second derivative at the interior knots
            left, right = st.second_derivatives(x, y, s, 'left'), st.second_derivatives(x, y, s, 'right')
            mscale = ((6 * np.abs(delta) + 4 * np.abs(s[:, :-1]) + 4 * np.abs(s[:, 1:])) / h).max(axis=-1)
            r.append(np.abs(left[:, 1:] - right[:, :-1]).max(axis=-1) / mscale)
            if bc == 'natural':
                r.append(np.maximum(np.abs(left[:, 0]), np.abs(right[:, -1])) / mscale)
            elif bc == 'clamped':
                assert not s[:, 0].any() and not s[:, -1].any()
            else:
                third = st.third_derivatives(x, y, s)
                tscale = (6 * (np.abs(s[:, :-1]) + np.abs(s[:, 1:]) + 2 * np.abs(delta)) / h**2)
                r.append(np.abs(third[:, 0] - third[:, 1]) / tscale[:, :2].max(axis=-1))
                r.append(np.abs(third[:, -1] - third[:, -2]) / tscale[:, -2:].max(axis=-1))
            used = float(np.max(r))
            worst = max(worst, used)
            assert used <= tol, (name, n, [float(v.max() / EPS) for v in r])
    print('%s: residuals at most %.3g longdouble ulps of the row\'s scale' % (bc, worst / EPS))


def _level(truth, f64):
    top, level = st.levels(truth, f64)
    assert (top > 0).all()
    return float(level.max() / st.FLOOR)


def _rows_uses():
    """Every (family, n, end condition, output, queries, extrapolate) of tests/test_spline_rows_edges_gpu.py."""
    uses = []
    for bc in st.BCS:
        for name in st.FAMILIES:
            for n in st.ROWS_SIZES:
                uses += [(name, n, bc, 'values', None, False), (name, n, bc, 'm', None, False)]
            for n, first, last in st.ROWS_EDGES:
                uses.append((name, n, bc, 'values', (first, last), False))
            for n in st.ROWS_EXTRAPOLATED:
                uses.append((name, n, bc, 'values', 'beyond', True))
    for name, n, nrows, group in st.ROWS_TRIPS:
        uses += [(name, n, 'natural', 'values', None, False), (name, n, 'natural', 'm', None, False)]
    return uses


def _rows_level(name, n, bc, what, queries, extrapolate):
    case = st.rows_case(name, n, bc)
    if what == 'm':
        return _level(case['m_ld'], case['m_f8'])
    x = case['x']
    xq = st.rows_beyond(x) if isinstance(queries, str) else st.rows_queries(x, *(queries or ()))
    return _level(*st.rows_values(case, xq, extrapolate))


@pytest.mark.parametrize('bc', st.BCS)
def test_levels_of_the_rows_cases(bc):
    over = {}
    for name, n, bc_, what, queries, extrapolate in _rows_uses():
        if bc_ != bc or (name == 'logk_pad' and n < 6):
            continue
        level = _rows_level(name, n, bc, what, queries, extrapolate)
        if not st.rows_used(name, n, bc, what):
            continue
        if level > st.CAP:
            over[(name, n, bc, what, queries)] = round(level, 1)
    assert not over, 'over the cap of {:.0f} FLOOR and still used: {}'.format(st.CAP, over)


def test_rows_over_cap_entries_are_over_the_cap():
    for (name, n, bc, what), quoted in st.ROWS_OVER_CAP.items():
        sizes = st.ROWS_SIZES if n == '*' else [n]
        bcs = st.BCS if bc == '*' else [bc]
        whats = ['values', 'm'] if what == '*' else [what]
        levels = [_rows_level(name, size, b, w, None, False) for size in sizes for b in bcs for w in whats if not (name == 'logk_pad' and size < 6)]
        print(name, n, bc, what, 'levels up to %.1f FLOOR (quoted %s)' % (max(levels), quoted))
        assert max(levels) > st.CAP, (name, n, bc, what, levels)


def test_rows_lds_bound_case():
    n, x = st.rows_largest()
    assert n == 2496 and st.rows_halo(x, 'natural') == 32
    for name in st.ROWS_LARGEST_FAMILIES:
        case = st.rows_case(name, n, 'natural')
        assert st.rows_halo(case['x'], 'natural') == 32
        assert _level(case['m_ld'], case['m_f8']) <= st.CAP and _level(*st.rows_values(case, st.rows_queries(case['x']))) <= st.CAP


@pytest.mark.parametrize('n', st.COLUMN_SIZES)
def test_levels_of_the_column_cases(n):
    case = st.column_case(n)
    parts = st.COLUMN_PARTS[st.COLUMN_SIZES.index(n)]
    assert parts == min(max((n - 1) // 80, 1), 8)
    xq, x0 = case['xq'], case['x'][0]
    assert (np.diff(xq) > 0).all()
    for part in range(1, parts):      # the knots of column 0 at which a part begins are queries, exactly
        assert x0[part * st.column_run(n, parts)] in xq
    assert x0[0] in xq and x0[-1] in xq
    assert (xq[:2] < case['x'].min()).all() and (xq[-2:] > case['x'].max()).all() and np.isnan(case['ld'][:, [0, 1, -2, -1]]).all()
    level = _level(case['ld'], case['f8'])
    print('n = %d: level at most %.3g FLOOR' % (n, level))
    assert level <= st.CAP


@pytest.mark.parametrize('n', sorted(st.GAP_BOXES))
def test_levels_of_the_gap_cases(n):
    y = st.gap_rows(n)
    x = 1. + np.arange(n)
    for a, b in st.GAP_BOXES[n]:
        truth, f64 = st.gap_case(n, a, b)
        assert truth.shape == (st.NBASE, b - a + 1) and truth.dtype == LD
        level = _level(truth, f64)
        print('n = %d, box (%d, %d): level %.3g FLOOR' % (n, a, b, level))
        assert level <= st.CAP
        keep = np.concatenate([np.arange(a), np.arange(b + 1, n)])
        ref = interpolate.CubicSpline(x[keep], (y * x**2)[:, keep], axis=-1, bc_type='clamped')(x[a:b + 1]) / x[a:b + 1]**2
        assert float((np.abs(ref - truth).max(axis=-1) / np.abs(ref).max(axis=-1)).max()) <= 1e-12


def test_rows_plan_restated():
    assert st.rows_halo(np.linspace(0., 1., 1000), 'natural') == 32      # 0.268^32 = 5e-19
    assert st.rows_halo(np.linspace(0., 1., 5), 'natural') == 8 and st.rows_halo(np.linspace(0., 1., 8), 'clamped') == 8
    assert [st.rows_layout(nw, 32)[0] for nw in st.ROWS_SIZES] == [st.ROWS_R[nw] for nw in st.ROWS_SIZES]
    assert st.rows_layout(1632, 32)[2] <= 160 * 1024 < (((8 * (1888 + 67) + 3) & ~3) + 4 * (1888 + 33)) * 8      # R = 2 at 1888 knots: 186 592 bytes
    assert [st.rows_layout(nw, 8)[1] for nw in (5, 8, 9)] == [1, 1, 1]
    assert st.rows_layout(2496, 32)[2] <= 160 * 1024 < st.rows_layout(2497, 32)[2]
    batch = st.batch(st.base_rows('uniform', 9), 30)
    assert np.array_equal(st.unscale(batch), st.base_rows('uniform', 9).astype(LD)[np.arange(30) % 7])
