"""GPU: ``spline_rows_kernel`` (csrc/cp_spline_rows.hip; ``SplineRows``: cp_spline_rows_apply / _second_derivatives / _pairs) against the longdouble truth
of tests/spline_truth.py -- a full solve of the first-derivative system, with no window, no halo and no lanes -- where the kernel's pieces meet:
(a) all-knots windows at the sizes where the layout changes (R = 4 -> 2 between 432 and 433 knots, 2 -> 1 between 1632 and 1633 by the LDS its row
    buffers need; 1888 and 1889, where the lanes of R = 2 end) and at 5, 8 and 9
    knots (one knot per lane, the halo as long as the row), values and second derivatives, ``pairs=True`` bit for bit;
(b) windows that end inside the row on both sides, on the left only and on the right only, with queries on the outermost knots they reach;
(c) ``extrapolate=True``: the end cubics continued, a NaN query, and NaN outside without it;
(d) more rows than the grid takes in one trip (the restaging of a wave's buffers behind ``wave_lds_phase``), R = 1 and R = 4, with a partly dead
    last group, root, scale and the grouped store, and a NaN row that stays alone;
(e) the largest window that fits the 160 KiB of LDS, and the refusal one knot later.
Every case asserts the R, halo, window and rows-per-trip it relies on, restated in ``spline_truth.rows_halo`` / ``rows_layout``.
Tolerance: the rule of tests/spline_truth.py, 16 levels of the float64 restatement per row; each test prints the largest fraction it used.
Measured on an MI355X, largest fraction of the allowance used (cp_spline_rows_apply / _second_derivatives together): layout thresholds 0.58 (432 knots;
<= 0.25 at 5, 8, 9 knots, <= 0.24 at 433 to 1889), window edges 0.24, extrapolate 0.26, more rows than one trip 0.086 (R = 1, 1034 rows, 1024 per
trip) and 0.076 (R = 4, 8203 rows, 8192 per trip), the LDS bound (2496 knots) 0.12.  With the run-ins of both sweeps cut to 4 knots in a scratch copy of the
kernel every test but the 5-knot ones fails, at 1e10 allowances.
These tests found that a window of 1633 to 1888 knots was refused: R = 2 by the length of its lanes, whose row buffers exceed the LDS from 1633 knots on
(halo 32), while R = 1 serves up to 2496; the plan now halves R until the buffers fit.
"""
import numpy as np
import pytest

import spline_truth as st

pytestmark = pytest.mark.gpu
NROWS = 23      # 23 mod 4 = 3, 23 mod 2 = 1: the last group of a wave is partly dead


def _env():
    import torch
    from cosmoprimo_amd.spline import SplineRows
    return torch, SplineRows, torch.device('cuda', 0)


def _plan(x, xq, bc, window, extrapolate=False):
    """The plan, held to the window (first knot, knots) and to the R and halo that the restated rules give for it."""
    torch, SplineRows, dev = _env()
    op = SplineRows(x, xq, bc=bc, extrapolate=extrapolate, device=dev)
    halo = st.rows_halo(x, bc)
    first, last = window
    w0, w1 = max(0, first - halo), min(x.size, last + 2 + halo)
    R, S, lds = st.rows_layout(w1 - w0, halo)
    assert op.window == (w0, w1 - w0, R, halo), (op.window, (w0, w1 - w0, R, halo))
    return op, R, S, lds


def _families(n, bc, what):
    return [name for name in st.FAMILIES if st.rows_used(name, n, bc, what)]


@pytest.mark.parametrize('bc', st.BCS)
@pytest.mark.parametrize('n', st.ROWS_SIZES)
def test_layout_thresholds(n, bc):
    torch, SplineRows, dev = _env()
    worst = 0.
    for name in st.FAMILIES:
        if not (st.rows_used(name, n, bc, 'values') or st.rows_used(name, n, bc, 'm')):
            continue
        case = st.rows_case(name, n, bc)
        x, xq = case['x'], st.rows_queries(case['x'])
        op, R, S, lds = _plan(x, xq, bc, (0, n - 1))
        assert op.window[3] != 32 or R == st.ROWS_R[n]
        if n < 10:
            assert S == 1 and op.window[3] >= n - 1
        y = torch.as_tensor(st.batch(case['y'], NROWS), device=dev)
        if st.rows_used(name, n, bc, 'values'):
            worst = max(worst, st.assert_within(op(y).cpu().numpy(), *st.rows_values(case, xq), what='%s %d %s values' % (name, n, bc), scaled=True))
        m = op.second_derivatives(y)
        pairs = op.second_derivatives(y, pairs=True)
        assert tuple(pairs.shape) == (NROWS, n, 2) and torch.equal(pairs[..., 0], y) and torch.equal(pairs[..., 1], m)
        if st.rows_used(name, n, bc, 'm'):
            worst = max(worst, st.assert_within(m.cpu().numpy(), case['m_ld'], case['m_f8'], what='%s %d %s second derivatives' % (name, n, bc), scaled=True))
    print('layout thresholds, %d knots, %s: largest fraction %.3g' % (n, bc, worst))


@pytest.mark.parametrize('bc', st.BCS)
@pytest.mark.parametrize('edge', st.ROWS_EDGES, ids=['n%d_%d_%d' % edge for edge in st.ROWS_EDGES])
def test_window_edges(edge, bc):
    torch, SplineRows, dev = _env()
    n, first, last = edge
    worst = 0.
    for name in _families(n, bc, 'values'):
        case = st.rows_case(name, n, bc)
        x = case['x']
        xq = st.rows_queries(x, first, last)
        assert xq[0] == x[first] and xq[-1] == x[last]      # queries on the outermost knots they reach, x[0] / x[n - 1] where the window touches an end
        op, R, S, lds = _plan(x, xq, bc, (first, last))
        w0, nw = op.window[:2]
        assert (w0 > 0) == (first > 0) and (w0 + nw < n) == (last < n - 1) and R == (2 if n == 2000 else 4)
        y = torch.as_tensor(st.batch(case['y'], NROWS), device=dev)
        worst = max(worst, st.assert_within(op(y).cpu().numpy(), *st.rows_values(case, xq), what='%s %s %s' % (name, edge, bc), scaled=True))
        assert nw < n
        with pytest.raises(NotImplementedError):      # the plan does not solve all knots
            op.second_derivatives(y)
    print('window edges %s, %s: largest fraction %.3g' % (edge, bc, worst))


@pytest.mark.parametrize('bc', st.BCS)
@pytest.mark.parametrize('n', st.ROWS_EXTRAPOLATED)
def test_extrapolate(n, bc):
    torch, SplineRows, dev = _env()
    worst = 0.
    for name in _families(n, bc, 'values'):
        case = st.rows_case(name, n, bc)
        x = case['x']
        xq = st.rows_beyond(x)
        outside = ~((xq >= x[0]) & (xq <= x[-1]))
        assert outside[:3].all() and outside[-3:].all() and outside.sum() == 7 and np.isnan(xq).sum() == 1
        y = torch.as_tensor(st.batch(case['y'], NROWS), device=dev)
        op, R, S, lds = _plan(x, xq, bc, (0, n - 1), extrapolate=True)      # the end intervals serve the queries beyond: all knots
        got = op(y).cpu().numpy()
        assert np.isnan(got[:, np.isnan(xq)]).all()
        worst = max(worst, st.assert_within(got, *st.rows_values(case, xq, True), what='%s %d %s continued' % (name, n, bc), scaled=True))
        op, R, S, lds = _plan(x, xq, bc, (0, n - 1), extrapolate=False)
        got = op(y).cpu().numpy()
        assert np.isnan(got[:, outside]).all()
        worst = max(worst, st.assert_within(got, *st.rows_values(case, xq, False), what='%s %d %s inside' % (name, n, bc), scaled=True))
    print('extrapolate, %d knots, %s: largest fraction %.3g' % (n, bc, worst))


@pytest.mark.parametrize('trip', st.ROWS_TRIPS, ids=['%s_n%d_rows%d' % trip[:3] for trip in st.ROWS_TRIPS])
def test_more_rows_than_one_trip(trip):
    torch, SplineRows, dev = _env()
    name, n, nrows, group = trip
    bc = 'natural'
    case = st.rows_case(name, n, bc)
    x = case['x']
    xq = st.rows_queries(x)[::17]
    xq = np.unique(np.concatenate([x[:2], xq, x[-2:]]))
    op, R, S, lds = _plan(x, xq, bc, (0, n - 1))
    assert R == (1 if n == 2000 else 4)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    blocks = ((nrows + R - 1) // R + 3) // 4
    grid = min(blocks, cus * min(max(160 * 1024 // lds, 1), 8))
    rows_per_trip = grid * 4 * R
    assert nrows > rows_per_trip, (nrows, rows_per_trip, cus, lds)      # some wave restages its buffers for a second group
    assert nrows % group == 0 and (R == 1 or nrows % R != 0) and nrows * n * 8 < 32e6
    y = torch.as_tensor(st.batch(case['y'], nrows), device=dev)
    truth, f64 = st.rows_values(case, xq)
    plain = op(y)
    worst = st.assert_within(plain.cpu().numpy(), truth, f64, what='%s plain' % (trip,), scaled=True)
    # root, scale and the grouped store: row i = base row i % 7 times 2**e_i, so the expected root is formed row by row
    scale = 0.3
    index, factor = np.arange(nrows) % st.NBASE, np.ldexp(st.LD(1), st.exponents(nrows))[:, None]
    root_ld = np.sqrt(st.LD(scale) * truth[index] * factor)
    root_f8 = np.sqrt(scale * f64[index] * factor.astype('f8'))
    rooted = op(y.reshape(nrows // group, group, n), sqrt=True, scale=scale, last_axis_first=True)
    assert tuple(rooted.shape) == (nrows // group, xq.size, group)
    rooted = rooted.transpose(-1, -2).reshape(nrows, xq.size).cpu().numpy()
    worst = max(worst, st.assert_within(rooted, root_ld, root_f8, what='%s root' % (trip,)))
    if R == 4:
        worst = max(worst, st.assert_within(op.second_derivatives(y).cpu().numpy(), case['m_ld'], case['m_f8'], what='%s second derivatives' % (trip,), scaled=True))
    # a NaN in a row of the first trip and in one of the second leaves every other row as it was
    bad = y.clone()
    hit = [5, nrows - 1]
    for row in hit:
        bad[row, n // 2] = float('nan')
    got = op(bad)
    keep = torch.ones(nrows, dtype=torch.bool, device=dev)
    keep[hit] = False
    assert torch.equal(got[keep], plain[keep]) and torch.isnan(got[~keep]).any(dim=-1).all()
    print('more rows than one trip %s: %d rows, %d per trip, largest fraction %.3g' % (trip, nrows, rows_per_trip, worst))


def test_lds_bound():
    torch, SplineRows, dev = _env()
    n, x = st.rows_largest(32)
    assert n == 2496 and st.rows_layout(n, 32)[2] <= 160 * 1024 < st.rows_layout(n + 1, 32)[2]
    worst = 0.
    for name in st.ROWS_LARGEST_FAMILIES:
        case = st.rows_case(name, n, 'natural')
        x, xq = case['x'], st.rows_queries(case['x'])
        op, R, S, lds = _plan(x, xq, 'natural', (0, n - 1))
        assert (R, op.window[3]) == (1, 32) and lds > 64 * 1024      # beyond the default LDS of a workgroup: the full-LDS opt-in
        y = torch.as_tensor(st.batch(case['y'], NROWS), device=dev)
        worst = max(worst, st.assert_within(op(y).cpu().numpy(), *st.rows_values(case, xq), what='%s %d values' % (name, n), scaled=True))
        worst = max(worst, st.assert_within(op.second_derivatives(y).cpu().numpy(), case['m_ld'], case['m_f8'], what='%s %d second derivatives' % (name, n), scaled=True))
        longer = st.knots(name, n + 1)
        assert st.rows_halo(longer, 'natural') == 32
        with pytest.raises(NotImplementedError):
            SplineRows(longer, longer, bc='natural', device=dev)
    print('LDS bound, %d knots: largest fraction %.3g' % (n, worst))
