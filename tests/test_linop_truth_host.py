"""CPU: tests/linop_truth.py, the longdouble truth of the operator kernels of csrc/cp_spline.hip, before tests/test_linop_truth_gpu.py relies on it.
(a) the truth against ``scipy.interpolate.CubicSpline(...)(xq, nu)`` for nu = 0, 1, 2, the three end conditions, the end cubics continued or NaN outside:
1e-13, 1e-12 and 1e-11 of the row's largest entry; this check is there to catch a wrong equation (measured: 1.5e-14, 1.1e-14, 1.1e-14);
(b) ``dense_operator`` (cp_spline_operator, host only) entry by entry against the longdouble spline of the unit rows, for every case of the grid:
ALLOW x FLOOR x sum_j |W_true[q, j]| and the float64 restatement's own distance; NaN rows where the truth has them; ``inside_out`` through the ABI --
the first independent check of the weights themselves.  A row that the end condition makes zero (the second derivative of a natural, the first of a clamped
spline at the two end knots) is given the sum of its interval's midpoint; a query on a knot at nu = 0 must be the unit vector exactly.  With float64
throughout, cp_spline_operator missed this rule on saw1.5x16 from 100 and on logk_pad from 100 knots, by up to 14 times at single entries: its weights, like
those of both float64 restatements, lay 400 to 900 floors of the row's sum from the truth there (second derivatives where neighbouring spacings differ by a
factor 438), and two float64 solves of that distance do not agree to 16 floors.  It now works in extended precision on such knots, for derivatives and for
continued end cubics (csrc/cp_spline.hip) and stays inside the allowance everywhere;
(c) the level of every (case, query set) the device tests use, at most CAP = 32 floors; what is over the cap is in ``linop_truth.OVER_CAP``, at most a tenth
of the grid, every entry held to being over the cap; the dense, middle-axis and outer cases likewise (measured: at most 7.7 floors);
(d) the restated plan (``plan_of``) against layouts computed by hand;
(e) the mutations of the float64 restatements that the device cases must catch: each is applied and must leave the allowance (fraction above 1, printed).
"""
import ctypes

import numpy as np
import pytest
from scipy import interpolate

import linop_truth as lt
import spline_truth as st

LD = np.longdouble


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bc', st.BCS)
def test_truth_against_scipy(bc):
    worst = [0., 0., 0.]
    for name in lt.SPLINE_FAMILIES:
        for n in (5, 16, 17, 100, 481):
            if (name == 'logk_pad' and n < 6) or (name == 'sigma_r' and n < 100):
                continue
            x, y = st.knots(name, n), st.base_rows(name, n)
            s = st.slopes(x, y, bc)
            ref = interpolate.CubicSpline(x, y, axis=-1, bc_type=bc)
            for nu, tol in ((0, 1e-13), (1, 1e-12), (2, 1e-11)):
                for xq, extrapolate in ((st.rows_queries(x), False), (st.rows_beyond(x), True), (st.rows_beyond(x), False)):
                    got, want = st.evaluate(x, y, s, xq, extrapolate, nu), ref(xq, nu)
                    if not extrapolate:
                        want[:, ~((xq >= x[0]) & (xq <= x[-1]))] = np.nan
                    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, n, nu)
                    d = float((np.nanmax(np.abs(got - want), axis=-1) / np.nanmax(np.abs(want), axis=-1)).max())
                    worst[nu] = max(worst[nu], d)
                    assert d <= tol, (name, n, nu, extrapolate, d)
    print('%s: nu = 0 %.3g, nu = 1 %.3g, nu = 2 %.3g from scipy' % (bc, *worst))


def test_truth_of_the_values_is_unchanged_by_the_derivative_order():
    """nu = 0 is the expression it was: the cubic in Horner form from the interval's lower knot; a query on a knot returns the sample exactly, the last
    knot from the last interval."""
    x, y = st.knots('geom1.05', 17), st.base_rows('geom1.05', 17)
    s = st.slopes(x, y)
    assert np.array_equal(st.evaluate(x, y, s, x[:-1]), y[:, :-1].astype(LD))      # t = 0
    assert (np.abs(st.evaluate(x, y, s, x[-1:]) - y[:, -1:]) <= 4 * np.finfo(LD).eps * np.abs(y).max()).all()      # t = h of the last interval
    h = x[-1] - x[-2]
    last = st.evaluate(x, y, s, x[-1:], nu=2)[:, 0]      # natural: zero at the last knot, taken from the last interval
    assert (np.abs(last) <= 1e-17 * np.abs(st.second_derivatives(x, y, s)).max(axis=-1)).all() and h > 0


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------------
def _library_operator(x, xq, bc, nu, extrapolate):
    from cosmoprimo_amd import _lib
    x, xq = np.ascontiguousarray(x, dtype='f8'), np.ascontiguousarray(xq, dtype='f8')
    w = np.empty((xq.size, x.size))
    inside = np.full(xq.size, -7, dtype=np.int32)
    _lib.check(_lib.load().cp_spline_operator(x.size, _lib.as_double_p(x), xq.size, _lib.as_double_p(xq), lt.BC[bc], int(nu), int(extrapolate), _lib.as_double_p(w),
                                              inside.ctypes.data_as(ctypes.POINTER(ctypes.c_int))))
    return w, inside


@pytest.mark.parametrize('n', lt.SIZES)
def test_dense_operator_against_the_unit_rows(n):
    from cosmoprimo_amd.spline import dense_operator
    worst = 0.
    for key in lt.spline_grid():
        name, n_, bc, nu = key
        if n_ != n:
            continue
        case = lt.spline_case(name, n, bc)
        x = case['x']
        for kind in ('knots', 'beyond', 'outside'):
            xq, extrapolate = lt.queries(x, kind)
            if kind == 'outside':      # the same queries without the end cubics: NaN rows outside, inside the truth and the allowance of 'beyond'
                got = dense_operator(x, xq, bc=bc, nu=nu, extrapolate=False)
                inside = (xq >= x[0]) & (xq <= x[-1])
                assert np.isnan(got[~inside]).all() and (~inside).sum() == 7 and np.isfinite(got[inside]).all(), key
                used = np.asarray(np.abs(got[inside].astype(LD) - true[inside]) / allowed[inside], dtype='f8')
                worst = max(worst, float(used.max()))
                assert used.max() <= 1., (key, kind, float(used.max()))
                continue
            if kind == 'knots' and n > 100:      # every fifth (tenth at 1000 knots) of them, the first and the last knot included
                xq = np.unique(np.concatenate([xq[::5 if n < 1000 else 10], x[[0, -1]]]))
            true = lt.operator_truth(name, n, bc, nu, xq, extrapolate)
            own = np.abs(lt.operator_f8(case, nu, xq, extrapolate).astype(LD) - true)
            got = dense_operator(x, xq, bc=bc, nu=nu, extrapolate=extrapolate)
            nan = np.isnan(true)
            assert np.array_equal(np.isnan(got), nan), key
            assert nan.all(axis=1).sum() == nan.any(axis=1).sum() == (kind == 'beyond')      # the NaN query: a whole row
            rowsum = np.where(nan, 0, np.abs(true)).sum(axis=1)
            # a row that the end condition makes zero (the second derivative of a natural, the first of a clamped spline at the two end knots) has no
            # scale of its own: its entries are differences of terms of the size of its interval's other rows; it is given the sum of the interval's midpoint
            if (bc, nu) in (('natural', 2), ('clamped', 1)):
                mid = np.abs(lt.operator_truth(name, n, bc, nu, np.array([0.5 * (x[0] + x[1]), 0.5 * (x[-2] + x[-1])]), False)).sum(axis=1)
                for end, scale in ((x[0], mid[0]), (x[-1], mid[1])):
                    assert (rowsum[xq == end] < 1e-3 * scale).all() and (xq == end).any()
                    rowsum[xq == end] = scale
            assert (rowsum[~nan[:, 0]] > 0).all(), (key, kind)
            allowed = lt.ALLOW * lt.FLOOR * rowsum[:, None] + np.where(nan, 0, own)
            used = np.asarray(np.where(nan, 0, np.abs(got.astype(LD) - true)) / np.where(nan, 1, allowed), dtype='f8')
            worst = max(worst, float(used.max()))
            assert used.max() <= 1., (key, kind, float(used.max()))
            if nu == 0 and kind == 'knots':      # a query on a knot (but the last, which the last interval serves from its far end): u = 0, the unit vector exactly
                on, at = np.flatnonzero(np.isin(xq, x[:-1])), np.searchsorted(x, xq[np.isin(xq, x[:-1])])
                assert on.size >= (n - 1) // 10 and np.array_equal(got[on], np.eye(n)[at]) and np.array_equal(true[on], np.eye(n)[at].astype(LD)), key
    print('n = %d: cp_spline_operator at most %.3g of its allowance from the longdouble operator' % (n, worst))


def test_inside_out_through_the_abi():
    x = st.knots('saw1.5x16', 17)
    xq = st.rows_beyond(x)
    for extrapolate in (False, True):
        w, inside = _library_operator(x, xq, 'natural', 0, extrapolate)
        want = ((xq >= x[0]) & (xq <= x[-1])).astype(np.int32)
        assert np.array_equal(inside, want) and want.sum() == xq.size - 7
        assert np.array_equal(np.isnan(w).all(axis=1), np.isnan(w).any(axis=1))      # whole rows
        if extrapolate:      # the end cubics continued: finite for every query that is a number
            assert np.isfinite(w[xq == xq]).all()
        else:
            assert np.isnan(w[want == 0]).all() and np.isfinite(w[want == 1]).all()


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------------------
def _main_level(key):
    name, n, bc, nu = key
    case = lt.spline_case(name, n, bc)
    return max(lt.spline_level(*lt.spline_values(case, nu, *lt.queries(case['x'], kind))) for kind in lt.MAIN_KINDS)


@pytest.mark.parametrize('n', lt.SIZES)
def test_levels_of_the_spline_cases(n):
    over, worst = {}, {}
    for key in lt.spline_used():
        name, n_, bc, nu = key
        if n_ != n:
            continue
        case = lt.spline_case(name, n, bc)
        for label, xq, extrapolate in lt.query_sets(key):
            level = lt.spline_level(*lt.spline_values(case, nu, xq, extrapolate))
            worst[(bc, nu)] = max(worst.get((bc, nu), 0.), level)
            if level > lt.CAP:
                over[key + (label,)] = round(level, 1)
    print('n = %d: levels at most %s FLOOR' % (n, {k: round(v, 1) for k, v in sorted(worst.items())}))
    assert not over, 'over the cap of {:.0f} FLOOR and still used: {}'.format(lt.CAP, over)


def test_over_cap_entries_are_over_the_cap_and_few():
    grid = lt.spline_grid()
    assert set(lt.OVER_CAP) <= set(grid) and 10 * len(lt.OVER_CAP) <= len(grid), (len(lt.OVER_CAP), len(grid))
    assert set(lt.extra_cases()) <= set(lt.spline_used())
    for key, quoted in lt.OVER_CAP.items():
        level = _main_level(key)
        print(key, 'level %.1f FLOOR (quoted %s)' % (level, quoted))
        assert level > lt.CAP, (key, level)


def test_levels_of_the_dense_cases():
    worst = 0.
    for name in lt.dense_cases():
        for signed, scale in ((True, 1.), (False, 1.), (True, 3.)):
            case = lt.dense_case(name, signed, scale)
            worst = max(worst, float(case['level'].max() / lt.FLOOR))
            finite = ~np.isnan(case['true'])
            assert (np.asarray(case['scale'])[finite] > 0).all()
            zero = (np.nan_to_num(case['w']) == 0).all(axis=1) & ~np.isnan(case['w'][:, 0])
            assert not (case['true'][:, ~zero & finite[0]] == 0).any() and not case['true'][:, zero].any()      # nothing identically zero but the rows of zeros
    for shape in lt.MID_SHAPES:
        for signed in (True, False):
            worst = max(worst, float(lt.mid_case(shape, signed)['level'].max() / lt.FLOOR))
    for nq in lt.OUTER_NQ:
        xq, g, truth, f64 = lt.outer_values(nq, 3)
        assert (truth[~np.isnan(truth)] > 0).all()      # the root is taken of positive values
        worst = max(worst, lt.spline_level(truth, f64))
    print('dense, middle-axis and outer cases: levels at most %.3g FLOOR' % worst)
    assert worst <= lt.CAP


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_restated_by_hand():
    # one query, three weights from knot 4 of 20
    w = np.zeros((1, 20))
    w[0, 4:7] = [1., -2., 0.5]
    p = lt.plan_of(w)
    assert (p['bw'], p['span_max'], p['n_pad'], p['nq_pad']) == (3, 3, 32, 64) and p['tiles'].tolist() == [[0, 1, 4, 3]]
    assert p['win64'].tolist() == [[0, 16]] and p['win16'].tolist() == [[0, 16], [0, 0], [0, 0], [0, 0]]
    assert p['sub_windows'] and not p['prefer_dense'] and (p['col_first'], p['col_last']) == (0, 16)      # work 1024 > 3.5 x 1 x 3; 256 <= 0.67 x 1024
    # 257 queries on 1000 knots, query q with the two knots 3 q and 3 q + 1: tiles of 256 and 1 queries, spans 767 > SPAN_CAP cut at 480
    w = np.zeros((257, 1000))
    for q in range(257):
        w[q, 3 * q:3 * q + 2] = [1., 1.]
    p = lt.plan_of(w)
    # a tile grows while (3 q + 2) - 3 q0 <= 480: 160 queries (span 479), then 97
    assert p['tiles'].tolist() == [[0, 160, 0, 479], [160, 97, 480, 290]] and p['span_max'] == 479 and p['bw'] == 2
    assert p['win64'][:2].tolist() == [[0, 192], [192, 384]] and p['win64'][4].tolist() == [768, 784] and p['win16'][1].tolist() == [48, 96]
    assert p['sub_windows'] and (p['col_first'], p['col_last']) == (0, 784)      # 16 queries: 64 of the 192 knots of their 64
    # the SPAN_CAP cut on 481 knots: two queries whose bands together cover 481 knots do not share a tile, 480 do
    w = np.zeros((2, 481))
    w[0, 0], w[1, 479:481] = 1., [1., 1.]
    assert lt.plan_of(w)['tiles'].tolist() == [[0, 1, 0, 2], [1, 1, 479, 2]]
    w = np.zeros((2, 481))
    w[0, 0], w[1, 478:480] = 1., [1., 1.]
    assert lt.plan_of(w)['tiles'].tolist() == [[0, 2, 0, 480]]
    # a row of zeros between banded rows takes the first knot of the row before it; in front of all, that of the next one
    w = np.zeros((4, 40))
    w[1, 10:13], w[3, 30:32] = 1., 1.
    p = lt.plan_of(w)
    assert p['j0'].tolist() == [10, 10, 10, 30] and p['j1'].tolist() == [10, 12, 10, 31] and p['bw'] == 3
    assert p['tiles'].tolist() == [[0, 4, 10, 23]] and p['wb'][:, 0].tolist() == [0., 0., 0.] and p['wb'][:, 3].tolist() == [1., 1., 0.]
    assert p['win64'].tolist() == [[0, 32]]
    # a NaN query first and last: no band, no share in tiles and windows
    w = np.zeros((3, 40))
    w[0], w[2], w[1, 17:20] = np.nan, np.nan, 2.
    p = lt.plan_of(w)
    assert p['j0'].tolist() == [-1, 17, -1] and p['tiles'].tolist() == [[0, 3, 17, 3]] and p['win64'].tolist() == [[16, 32]]
    assert (p['col_first'], p['col_last']) == (16, 32)
    # rows per work item
    assert [lt.apply_rows(dict(span_max=100), r) for r in (1, 4, 5, 8, 9, 16)] == [4, 4, 8, 8, 16, 16]
    assert [lt.apply_rows(dict(span_max=s), 100) for s in (512, 513, 1024, 1025)] == [16, 8, 8, 4]
    assert [lt.outer_rows(dict(span_max=100), 3, r) for r in (1, 2, 3, 4, 5, 9)] == [2, 2, 4, 4, 8, 8]
    assert [lt.outer_rows(dict(span_max=257), nz, 9) for nz in (510, 511, 512)] == [8, 8, 4]      # (257 + 256 + nz) x 8 x 8 bytes against 64 KB


# ---- (e) -------------------------------------------------------------------------------------------------------------------------------------------
def _dense_mutated(name, restated, mutation, rows=None):
    case = lt.dense_case(name)
    y = case['y'] if rows is None else rows
    try:
        return lt.dense_fraction(restated(case['plan'], y, mutation), case['true'], case['scale'], case['level'], what='%s on %s' % (mutation, name))
    except AssertionError:      # NaN in other places than the truth has them
        return np.inf


def test_the_restatements_hold_without_a_mutation():
    """The float64 contractions in the kernels' order are restatements: inside the allowance on every dense case."""
    for name in lt.dense_cases():
        assert _dense_mutated(name, lt.band_sum, None) <= 1. and _dense_mutated(name, lt.window_sum, None) <= 1.
    for key in [k for k in lt.spline_used() if k[1] in (17, 100)]:
        case = lt.spline_case(*key[:3])
        xq, extrapolate = lt.queries(case['x'], 'knots')
        truth, f64 = lt.spline_values(case, key[3], xq, extrapolate)
        assert lt.spline_fraction(lt.restated_spline(case, key[3], xq, extrapolate), truth, f64, what=str(key)) <= 1.


@pytest.mark.parametrize('mutation,restated,names', [('shift', lt.band_sum, ['random_bw9', 'sweep_bw17', 'full_100x65']),
                                                     ('last_chunk', lt.band_sum, ['random_bw9', 'random_bw17', 'full_100x65']),
                                                     ('round_up', lt.window_sum, ['random_bw7', 'sweep_bw9', 'full_17x64']),
                                                     ('previous_window', lt.window_sum, ['sweep_bw9', 'sweep_bw17'])])
def test_mutations_of_the_contractions(mutation, restated, names):
    caught = {name: _dense_mutated(name, restated, mutation) for name in names}
    print('MUTATION %-16s fractions of the allowance %s' % (mutation, caught))
    assert max(caught.values()) > 1.


def test_mutation_next_row():
    """The entries behind knot n of the partial last chunk taken from the next row: the weights there are zero, a NaN sample at the head of the next row
    shows it (the device cases carry one in knot 0 of a row)."""
    caught = {}
    for name in ('random_bw9', 'full_17x64'):
        case = lt.dense_case(name)
        assert case['plan']['n'] % 16
        rows = case['y'].copy()
        rows[3, 0] = np.nan
        clean = lt.window_sum(case['plan'], rows)
        assert np.array_equal(np.isnan(clean[[0, 1, 2, 4, 5, 6]]), np.isnan(case['true'][[0, 1, 2, 4, 5, 6]]))
        mutated = lt.window_sum(case['plan'], rows, 'next_row')
        extra = int((np.isnan(mutated[2]) & ~np.isnan(case['true'][2])).sum())
        caught[name] = np.inf if extra else 0.
    print('MUTATION next_row         fractions of the allowance %s' % caught)
    assert max(caught.values()) > 1.


def test_mutation_swapped_strides():
    caught = {}
    for name, nrows, group in (('random_bw9', 128, 64), ('full_17x64', 128, 128)):
        case = lt.dense_case(name)
        true, level = lt.tile(case['true'], nrows), case['level']
        values = lt.tile(case['f64'], nrows)
        for mutation in (None, 'swap_strides'):
            stored = lt.ungroup(lt.grouped_store(values, group, mutation), nrows, values.shape[1], group)
            try:
                used = lt.dense_fraction(stored, true, lt.tile(case['scale'], nrows), level, what='%s, group %d, %s' % (name, group, mutation))
            except AssertionError:
                used = np.inf
            if mutation is None:
                assert used <= 1.
        caught[name] = used
    print('MUTATION swap_strides     fractions of the allowance %s' % caught)
    assert max(caught.values()) > 1.


def test_mutation_without_the_factor_2():
    caught = {}
    for key in lt.spline_used():
        if key[3] != 1 or key[1] not in (16, 17, 100):
            continue
        case = lt.spline_case(*key[:3])
        xq, extrapolate = lt.queries(case['x'], 'knots')
        truth, f64 = lt.spline_values(case, 1, xq, extrapolate)
        caught[key] = lt.spline_fraction(lt.restated_spline(case, 1, xq, extrapolate, 'no_factor_2'), truth, f64, what='no_factor_2 on %s' % (key,))
    print('MUTATION %-16s largest fraction of the allowance %.3g on %s' % ('no_factor_2', max(caught.values()), max(caught, key=caught.get)))
    assert max(caught.values()) > 1.


def test_mutation_knot_assigned_to_the_interval_below():
    """A cubic spline and its first two derivatives are continuous at the knots: taken from the interval below, a query on a knot differs by rounding
    only and stays inside the allowance (measured: at most 0.22 of it, at nu = 2).  What the assignment does fix is exactness: from the interval that begins
    at the knot u = 0, the row of the operator is the unit vector and the value the sample, bit for bit -- which (b) above holds for cp_spline_operator and
    tests/test_linop_truth_gpu.py for the kernels (``on_knots_exact``).  That allowance is zero, and the mutation leaves it on every case."""
    by_allowance, caught = {}, {}
    for key in lt.spline_used():
        if key[1] not in (16, 17, 100):
            continue
        case = lt.spline_case(*key[:3])
        xq, extrapolate = lt.queries(case['x'], 'knots')
        mutated = lt.restated_spline(case, key[3], xq, extrapolate, 'knot_below')
        truth, f64 = lt.spline_values(case, key[3], xq, extrapolate)
        by_allowance[key] = lt.spline_fraction(mutated, truth, f64, what='knot_below on %s' % (key,))
        if key[3] == 0:
            on = np.flatnonzero(np.isin(xq, case['x'][:-1]))
            assert np.array_equal(lt.restated_spline(case, 0, xq, extrapolate)[:, on], case['y'][:, :-1])
            distance = np.abs(mutated[:, on] - case['y'][:, :-1]).max()
            caught[key] = np.inf if distance > 0. else 0.
    print('MUTATION %-16s largest fraction of the allowance %.3g; of the zero allowance of a query on a knot at nu = 0: %s on %d of %d cases'
          % ('knot_below', max(by_allowance.values()), max(caught.values()), sum(v > 1. for v in caught.values()), len(caught)))
    assert max(caught.values()) > 1.
