"""CPU: csrc/cp_spline_system.h (compiled with g++: tests/host_emu/emu_spline_system.cpp), the host arithmetic that cp_spline_rows_plan_create,
cp_splice_plan_create and cpsu::build share -- the system for the second derivatives and its elimination factors, the halo search, a query's
interval and weights:
(a) factors and halo bit for bit against the restatements the GPU tests trust -- ``splice_truth.factors`` / ``elimination_plan`` (clamped) and
    ``spline_truth.rows_halo`` (the three end conditions).  c of the last knot is 0 in the header (the last row has no super-diagonal; no sweep
    reads it) where ``splice_truth.factors`` holds h inv: every other entry is compared;
(b) a sequential solve with the factors -- forward sweep, back substitution, the not-a-knot end fixes, then the queries' weights -- against the
    longdouble truth of tests/spline_truth.py under its own rule (16 levels of the float64 restatement per row), second derivatives and values,
    wherever ``spline_truth.rows_used`` takes the case;
(c) intervals and weights bit for bit against numpy for queries on the knots, ``nextafter`` on either side of them, outside the knots and NaN, with and
    without ``extrapolate``; a query on a knot weighs that knot alone;
(d) the predicate for increasing knots."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import splice_truth as sp
import spline_truth as st
from conftest import ROOT

FAMILIES = ['uniform', 'geom1.05', 'saw2x40', 'alt1e3']
SIZES = [5, 9, 65, 433, 700]
ENDS = {'natural': 0, 'clamped': 1, 'not-a-knot': 2}


def _lib():
    src = os.path.join(ROOT, 'tests', 'host_emu', 'emu_spline_system.cpp')
    out = os.path.join(ROOT, 'tests', 'host_emu', 'libemu_spline_system.so')
    dep = os.path.join(ROOT, 'cosmoprimo_amd', 'csrc', 'cp_spline_system.h')
    if not os.path.isfile(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(dep)):
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', out, src])
    return ctypes.CDLL(out)


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def factors(x, bc):
    """dict(h, inv, c, q (n,), fix (4,), halo) of the header for these knots."""
    x = np.ascontiguousarray(x, dtype='f8')
    out = {key: np.zeros(x.size) for key in ('h', 'inv', 'c', 'q')}
    out['fix'] = np.zeros(4)
    out['halo'] = _lib().emu_spline_factors(x.size, _dp(x), ENDS[bc], *(_dp(out[key]) for key in ('h', 'inv', 'c', 'q', 'fix')))
    return out


def queries(x, xq, extrapolate):
    x, xq = np.ascontiguousarray(x, dtype='f8'), np.ascontiguousarray(xq, dtype='f8')
    qj, qw = np.zeros(xq.size, dtype=np.int32), np.zeros((xq.size, 4))
    _lib().emu_spline_queries(x.size, _dp(x), xq.size, _dp(xq), int(extrapolate), qj.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dp(qw))
    return qj, qw


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype='f8').view('i8'), np.asarray(b, dtype='f8').view('i8'))


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', FAMILIES)
def test_factors_and_halo(name, n):
    x = st.knots(name, n)
    for bc in st.BCS:
        if bc == 'not-a-knot' and n < 5:
            continue
        got = factors(x, bc)
        expected = st.rows_halo(x, bc)
        assert got['halo'] == expected if expected is not None else got['halo'] > 128, (name, n, bc, got['halo'], expected)
        assert _same(got['h'], np.append(np.diff(x), x[-1] - x[-2])) and got['q'][0] == 0.
        if bc != 'not-a-knot':
            assert not got['fix'].any()
        if bc != 'clamped':
            assert got['inv'][0] == 0. and got['inv'][-1] == 0.      # the outermost rows are not equations of the system
    got = factors(x, 'clamped')
    h, inv, c = sp.factors(x)
    assert _same(got['h'], h) and _same(got['inv'], inv) and _same(got['c'][:-1], c[:-1]) and got['c'][-1] == 0.
    assert _same(got['q'], np.append(0., h[:-1] * inv[1:]))      # what cp_splice_plan_create wrote as h[i - 1] * inv[i]
    plan = sp.elimination_plan(x)
    assert got['halo'] == plan['halo'] if plan is not None else got['halo'] > 128


def solve(f, y):
    """The second derivatives (rows, n) of the splines through y by the factors f, one knot after the other as the kernels' sweeps go, and the end
    fixes of the not-a-knot condition."""
    n = y.shape[-1]
    sigma = np.zeros((len(y), n + 1))      # sigma[:, i + 1] = 6 (y_{i+1} - y_i) / h_i; zero slopes beyond either end
    sigma[:, 1:n] = np.diff(y, axis=-1) * (6. / f['h'][:-1])
    d = np.zeros_like(y)
    prev = np.zeros(len(y))
    for i in range(n):
        prev = d[:, i] = f['inv'][i] * (sigma[:, i + 1] - sigma[:, i]) - f['q'][i] * prev
    m = d.copy()
    for i in range(n - 2, -1, -1):
        m[:, i] = d[:, i] - f['c'][i] * m[:, i + 1]
    if f['fix'].any():
        m[:, 0] = f['fix'][0] * m[:, 1] + f['fix'][1] * m[:, 2]
        m[:, -1] = f['fix'][2] * m[:, -2] + f['fix'][3] * m[:, -3]
    return m


@pytest.mark.parametrize('bc', st.BCS)
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', FAMILIES)
def test_sequential_solve_meets_the_truth(name, n, bc):
    use_m, use_values = st.rows_used(name, n, bc, 'm'), st.rows_used(name, n, bc, 'values')
    if not (use_m or use_values):
        return      # over the cap of the tolerance rule in both outputs (spline_truth.ROWS_OVER_CAP): no device test uses the case either
    case = st.rows_case(name, n, bc)
    x, y = case['x'], case['y']
    f = factors(x, bc)
    assert f['halo'] <= 128
    m = solve(f, y)
    if use_m:
        st.assert_within(m, case['m_ld'], case['m_f8'], what='%s %d %s second derivatives' % (name, n, bc))
    if use_values:
        xq = st.rows_queries(x)
        qj, qw = queries(x, xq, False)
        assert (qj >= 0).all()
        values = qw[:, 0] * y[:, qj] + qw[:, 1] * y[:, qj + 1] + (qw[:, 2] * m[:, qj] + qw[:, 3] * m[:, qj + 1])
        st.assert_within(values, *st.rows_values(case, xq), what='%s %d %s values' % (name, n, bc))


@pytest.mark.parametrize('extrapolate', [False, True])
@pytest.mark.parametrize('n', [5, 65, 433])
@pytest.mark.parametrize('name', FAMILIES)
def test_intervals_and_weights(name, n, extrapolate):
    x = st.knots(name, n)
    h0, h1 = x[1] - x[0], x[-1] - x[-2]
    beyond = [x[0] - h0, np.nextafter(x[0], -np.inf), np.nextafter(x[-1], np.inf), x[-1] + 0.5 * h1]
    xq = np.concatenate([x, np.nextafter(x, -np.inf)[1:], np.nextafter(x, np.inf)[:-1], beyond, [np.nan], 0.5 * (x[:-1] + x[1:])])
    qj, qw = queries(x, xq, extrapolate)
    inside = (xq >= x[0]) & (xq <= x[-1])
    used = inside | (extrapolate & ~np.isnan(xq))
    assert (~inside & used).sum() == (4 if extrapolate else 0) and (~used).sum() == (1 if extrapolate else 5)
    j = np.clip(np.searchsorted(x, np.where(np.isnan(xq), x[0], xq), side='right') - 1, 0, n - 2)
    assert np.array_equal(qj, np.where(used, j, -1))
    assert not qw[~used].any()
    j, v = j[used], xq[used]
    h = x[j + 1] - x[j]
    a, b = (x[j + 1] - v) / h, (v - x[j]) / h
    expected = np.stack([a, b, (a * a * a - a) * (h * h) / 6., (b * b * b - b) * (h * h) / 6.], axis=-1)
    assert _same(qw[used], expected)
    # a query on a knot weighs that knot alone: the first n queries are the knots
    assert np.array_equal(qj[:n], np.minimum(np.arange(n), n - 2))
    assert np.array_equal(qw[:n - 1], np.tile([1., 0., 0., 0.], (n - 1, 1))) and np.array_equal(qw[n - 1], [0., 1., 0., 0.])


def test_increasing():
    lib = _lib()
    for name in FAMILIES:
        x = np.ascontiguousarray(st.knots(name, 65))
        assert lib.emu_spline_increasing(x.size, _dp(x)) == 1
        for spoil in (lambda a: a.__setitem__(31, a[30]), lambda a: a.__setitem__(31, np.nan), lambda a: a.__setitem__(64, a[0]), lambda a: a.__setitem__(0, np.inf)):
            bad = x.copy()
            spoil(bad)
            assert lib.emu_spline_increasing(bad.size, _dp(bad)) == 0
    x = np.ascontiguousarray(st.knots('uniform', 65)[::-1])
    assert lib.emu_spline_increasing(x.size, _dp(x)) == 0
