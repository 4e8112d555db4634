"""CPU: tests/wallish_truth.py before tests/test_wallish_truth_gpu.py relies on it -- the truth against scipy and its own argmax, every case on the edge it is
named for (lane, place in the segment, where the second range starts, the branch of remove_box*, masked_argmax or the walk), the lead of every planted
decision over its runner-up in float64 and in longdouble, the levels against the cap, the launch plans against numbers worked out by hand for 256 CUs, and
the mutations of the restatements with the case that rejects each.

Measured here (printed by the tests): the largest |M_f64 - M_ld| over all cases (1.15e-12 at n = 1024, 2.59e-12 at 2048) and the smallest lead of a planted
decision (7.2: 6e12 and 3e12 times that); the levels of M (1 to 5.6 FLOOR) and of the rewritten boxes (1 to 23.5 FLOOR; three blocks over the cap of 32,
wallish_truth.OVER_CAP); the halo of 32 knots in longdouble against the longdouble solve (8e-20 of the largest |M|); where the tables of c_i reach their
limit (knot 15 from 1/2, knot 14 from 0).

One mutation of the issue's list cannot be rejected in float64 and is held to that instead: a sweep that starts inside the sequence started as clamped
(slope 0 where the centred difference belongs).  Such a sweep always has its full 64 knots in front of the box, and a sweep forgets its start at 0.268 per
knot -- 1e-36 of it arrives: the mutated restatement has the bits of the unmutated one (test_start_inside_is_forgotten).  The reverse, a sweep from the true
end started on a centred difference, is rejected by the boxes next to the end."""
import numpy as np
import pytest

import spline_truth as st
import wallish_truth as wt

LD = np.longdouble


def finite_rows(g):
    return np.flatnonzero(g['finite'])


def rows_of(g, case):
    return [r for r, lab in enumerate(g['labels']) if lab[0] == case]


@pytest.mark.parametrize('n', wt.SIZES)
def test_truth_against_scipy(n):
    """M against scipy's CubicSpline(bc_type='clamped')(x, nu=2) within the rule's allowance, the boxes against the argmax written as in
    tests/test_fused_kernels_gpu.py::test_wallish_dd_box."""
    from scipy import interpolate
    x = 1. + np.arange(n)
    for name in ('m20_5', 'm0_0'):
        g = wt.group(n, name)
        mf, ms = g['margins']
        for r in finite_rows(g)[::5]:
            i = g['index'][r]
            ref = interpolate.CubicSpline(x, g['y'][r], bc_type='clamped')(x, nu=2)
            allowed = wt.allowance(g['m_ld'][i:i + 1], g['m_f8'][i:i + 1])[0]
            assert np.abs(ref.astype(LD) - g['m_ld'][i]).max() <= allowed, (name, r)
            first = ref[mf:n - mf].argmax() + mf
            second = first + ms + ref[first + ms:n - mf].argmax() if first + ms < n - mf else 0
            assert (first, second) == tuple(g['found_ld'][i]), (name, g['labels'][r])
    with pytest.raises(ValueError):      # a sequence that is not finite has no reference
        interpolate.CubicSpline(x, wt.group(n, 'm20_5')['y'][rows_of(wt.group(n, 'm20_5'), 'one_nan')[0]], bc_type='clamped')


def planted(n, name, case):
    """(first, second or None) as the dips of a case place them."""
    mf, ms, _, _ = wt.settings(n, name)
    dips = dict((c, d) for c, _, d, _ in wt.cases(n, name))[case]
    if not dips:
        return None
    first = dips[0][0]
    seconds = [knot for knot, weight in dips[1:] if weight in (wt.SECOND, wt.SECOND / 2, 2 * wt.SECOND)]
    if seconds:
        return first, seconds[0]
    if first + ms >= n - mf:
        return first, 0
    return first, first if ms == 0 else None


# what ``wallish_truth.describe`` must say of a case: (group, case) -> predicate of (description, n, S)
EDGES = {
    ('m0_0', 'knot_0'): lambda d, n, S: d['lane_first'] == 0 and d['place_first'] == 0 and d['box'][0] == 0 and not d['valid'],
    ('m0_0', 'knot_last'): lambda d, n, S: d['lane_first'] == 63 and d['place_first'] == S - 1 and d['box'][1] == n - 1 and not d['valid'],
    ('m0_0', 'box_1_1'): lambda d, n, S: d['box'] == (1, 1) and d['left_trivial'] and d['length'] == 1,
    ('m0_0', 'box_last'): lambda d, n, S: d['box'] == (n - 2, n - 2) and d['right_trivial'] and d['length'] == 1,
    ('m0_0', 'nl_0'): lambda d, n, S: d['nl'] == 0 and not d['left_trivial'] and d['left_clamped'],
    ('m0_0', 'nr_0'): lambda d, n, S: d['nr'] == 0 and not d['right_trivial'] and d['right_clamped'],
    ('m0_0', 'nl_1'): lambda d, n, S: d['nl'] == 1 and d['left_clamped'],
    ('m0_0', 'nr_1'): lambda d, n, S: d['nr'] == 1 and d['right_clamped'],
    ('m0_0', 'end_l0'): lambda d, n, S: d['lane_first'] == 0 and d['place_first'] == S - 1,
    ('m0_0', 'start_l1'): lambda d, n, S: d['lane_first'] == 1 and d['place_first'] == 0,
    ('m0_0', 'end_l1'): lambda d, n, S: d['lane_first'] == 1 and d['place_first'] == S - 1,
    ('m0_0', 'start_l31'): lambda d, n, S: d['lane_first'] == 31 and d['place_first'] == 0,
    ('m0_0', 'end_l31'): lambda d, n, S: d['lane_first'] == 31 and d['place_first'] == S - 1,
    ('m0_0', 'start_l63'): lambda d, n, S: d['lane_first'] == 63 and d['place_first'] == 0,
    ('m0_0', 'zero'): lambda d, n, S: d['first'] == 0 and d['second'] == 0,
    ('m1_0', 'at_margin'): lambda d, n, S: d['first'] == 1,
    ('m1_0', 'at_upper'): lambda d, n, S: d['first'] == n - 2,
    ('m1_0', 'decoys'): lambda d, n, S: 1 < d['first'] < n - 2,
    ('m1_0', 'decoy_below'): lambda d, n, S: d['first'] == 1,
    ('m1_0', 'decoy_above'): lambda d, n, S: d['first'] == n - 2,
    ('m1_0_wide', 'box_all'): lambda d, n, S: d['box'] == (1, n - 2) and d['left_trivial'] and d['right_trivial'] and d['length'] > 128,
    ('m1_0_wide', 'box_beyond'): lambda d, n, S: d['box'][1] > n - 2 and not d['valid'],
    ('mhalf_0', 'low'): lambda d, n, S: d['first'] == n // 2 - 1 and d['lane_first'] == 31 and d['place_first'] == S - 1,
    ('mhalf_0', 'high'): lambda d, n, S: d['first'] == n // 2 and d['lane_first'] == 32 and d['place_first'] == 0,
    ('mhalf_0', 'zero'): lambda d, n, S: d['first'] == n // 2 - 1 and d['second'] == n // 2 - 1,
    ('m20_5', 'at_margin'): lambda d, n, S: d['first'] == 20,
    ('m20_5', 'at_upper'): lambda d, n, S: d['first'] == n - 21 and d['empty'] and d['second'] == 0 and d['box'][1] < d['box'][0] and not d['valid'],
    ('m20_5', 'decoys'): lambda d, n, S: 20 < d['first'] < d['second'] < n - 21,
    ('m20_5', 'second_at_lower'): lambda d, n, S: d['second'] == d['lower'] and d['straddling'],
    ('m20_5', 'lower_start'): lambda d, n, S: d['place_lower'] == 0 and d['straddling'],
    ('m20_5', 'lower_start_later'): lambda d, n, S: d['place_lower'] == 0 and not d['straddling'],
    ('m20_5', 'lower_end'): lambda d, n, S: d['place_lower'] == S - 1 and d['straddling'] and d['second'] == d['lower'],
    ('m20_5', 'lower_end_later'): lambda d, n, S: d['place_lower'] == S - 1 and not d['straddling'] and d['second'] == d['lower'] + 1,
    ('m20_5', 'lower_mid'): lambda d, n, S: 0 < d['place_lower'] < S - 1 and d['straddling'],
    ('m20_5', 'lower_mid_later'): lambda d, n, S: 0 < d['place_lower'] < S - 1 and not d['straddling'],
    ('m20_5', 'empty'): lambda d, n, S: d['empty'] and d['second'] == 0 and d['first'] < n - 21 and not d['valid'],
    ('m20_5', 'L_64'): lambda d, n, S: d['L'] == 64 and d['i0'] == 0 and d['left_clamped'] and d['nl'] == 63,
    ('m20_5', 'L_65'): lambda d, n, S: d['L'] == 65 and d['i0'] == 1 and not d['left_clamped'] and d['nl'] == 63,
    ('m20_5', 'R_64'): lambda d, n, S: d['R'] + 64 == n - 1 and d['right_clamped'] and d['nr'] == 63 and 64 < d['length'] <= 128,
    ('m20_5', 'R_63'): lambda d, n, S: d['R'] + 64 == n - 2 and not d['right_clamped'] and d['nr'] == 63 and 64 < d['length'] <= 128,
    ('m20_5', 'long'): lambda d, n, S: d['length'] > 128 and not d['left_clamped'] and not d['right_clamped'],
    ('m20_5', 'zero'): lambda d, n, S: d['first'] == 20 and d['second'] == 25 and d['valid'],
    ('m20_far', 'straddle'): lambda d, n, S: d['lower'] - d['first'] > S and d['straddling'],
    ('m20_far', 'later'): lambda d, n, S: d['lower'] - d['first'] > S and not d['straddling'],
    ('m20_far', 'on_start'): lambda d, n, S: d['place_lower'] == 0 and d['second'] == d['lower'],
}


@pytest.mark.parametrize('n', wt.SIZES)
def test_cases_hold_their_edges(n):
    S = n // 64
    seen = set()
    for name in wt.GROUPS:
        g = wt.group(n, name)
        others = dict((c, o) for c, _, _, o in wt.cases(n, name))
        for r, (case, copy, edge, finite) in enumerate(g['labels']):
            y = g['y'][r:r + 1]
            with np.errstate(invalid='ignore'):
                restated = wt.m_recursive(y) if n == 2048 else wt.m_elimination(y)
            if not finite:      # the sum that decides between masked_argmax and the walk is poisoned: the restated M holds a NaN or an infinity
                assert isinstance(others[case], list) and not np.isfinite(restated).all(), (name, case)
                seen.add((name, case))
                continue
            assert np.isfinite(restated).all(), (name, case)
            found = g['found_ld'][g['index'][r]]
            want = planted(n, name, case)
            if want is not None:
                assert found[0] == want[0] and (want[1] is None or found[1] == want[1]), (name, case, tuple(found), want)
            m, (mf, ms) = g['m_ld'][g['index'][r]], g['margins']
            for knot, weight in dict((c, d) for c, _, d, _ in wt.cases(n, name))[case]:      # every decoy is larger than the maximum it stands beside
                if not mf <= knot < n - mf:
                    assert m[knot] > m[found[0]], (name, case, knot)
                elif knot < found[0] + ms and knot != found[0]:
                    assert m[knot] > m[found[1]], (name, case, knot)
            d = wt.describe(n, g['margins'], g['offsets'], found)
            if (name, case) in EDGES:
                assert EDGES[(name, case)](d, n, S), (name, case, d)
                seen.add((name, case))
            else:
                assert case == 'plain', (name, case)
    # every case of every group is held to something, and no edge has lost all its cases to the cap
    for name in wt.GROUPS:
        for case, _, _, other in wt.cases(n, name):
            assert case == 'plain' or (name, case) in seen, (name, case)


def lead(row, lo, hi, at):
    """row[at] minus the largest other value of row[lo:hi] (inf for a range of one knot or none)."""
    if hi - lo < 2:
        return np.inf
    seg = np.array(row[lo:hi])
    top = seg[at - lo]
    seg[at - lo] = -np.inf
    return float(top - seg.max())


@pytest.mark.parametrize('n', wt.SIZES)
def test_leads_and_types_decide_alike(n):
    worst_err, least_lead, leads = 0., np.inf, []
    for name in wt.GROUPS:
        g = wt.group(n, name)
        mf, ms = g['margins']
        assert np.array_equal(g['found_ld'], g['found_f8']), name      # float64 and longdouble decide every box alike, planted or not
        fy = g['y'][g['finite']]
        restated = wt.m_recursive(fy) if n == 2048 else wt.m_elimination(fy)
        assert np.array_equal(wt.box_rule(restated, mf, ms), g['found_ld']), name      # ... and so does the restatement of the scheme that runs
        worst_err = max(worst_err, float(np.abs(g['m_plain'].astype(LD) - g['m_ld']).max()))
        for r in finite_rows(g):
            case = g['labels'][r][0]
            if case in ('plain', 'zero'):
                continue
            i = g['index'][r]
            first, second = g['found_ld'][i]
            for m in (g['m_ld'][i], g['m_plain'][i]):
                leads.append((lead(m, mf, n - mf, first), name, case))
                if first + ms < n - mf:
                    leads.append((lead(m, first + ms, n - mf, second), name, case))
    least_lead, where = min((v, (name, case)) for v, name, case in leads)
    print('n = %d: largest |M_f64 - M_ld| %.3g, smallest lead of a planted decision %.3g (%s): %.3g times' % (n, worst_err, least_lead, where, least_lead / worst_err))
    assert least_lead >= wt.LEAD_FACTOR * worst_err


@pytest.mark.parametrize('n', wt.SIZES)
def test_exact_ties(n):
    """An all-zero sequence: first = margin_first, second = first + margin_second; two NaN or two +inf: the first one wins (numpy's rule on a row that
    holds them, which is what the device's own M is held to)."""
    for name in ('m0_0', 'mhalf_0', 'm20_5'):
        g = wt.group(n, name)
        mf, ms = g['margins']
        for r in rows_of(g, 'zero'):
            assert not g['m_ld'][g['index'][r]].any() and tuple(g['found_ld'][g['index'][r]]) == (mf, mf + ms)
    row = np.zeros(n)
    row[[300, 700]] = np.nan
    assert tuple(wt.box_rule(row, 20, 5)[0]) == (300, 700)
    row[[300, 700]] = np.inf
    row[500] = 1.
    assert tuple(wt.box_rule(row, 20, 5)[0]) == (300, 700) and wt.box_rule(row, 20, 5, last=True)[0][0] == 700


@pytest.mark.parametrize('n', wt.SIZES)
def test_levels_and_cap(n):
    top_m, top_gap, over = 0., 0., {}
    edges_left = set()
    for name in wt.GROUPS:
        full = wt.group(n, name, False)
        _, level = st.levels(full['m_ld'], full['m_f8'])
        top_m = max(top_m, float(level.max() / wt.FLOOR))
        assert level.max() <= wt.CAP * wt.FLOOR, name
        for r in finite_rows(full):
            case, copy = full['labels'][r][:2]
            figure = 1.
            if r in full['gap_ld']:
                figure = float(st.levels(full['gap_ld'][r][None], full['gap_f8'][r][None])[1][0] / wt.FLOOR)
            if figure > wt.CAP:
                over[(n, name, case, copy)] = figure
            else:
                top_gap = max(top_gap, figure)
                edges_left.add((name, case))
        sent = wt.group(n, name)
        assert len(sent['y']) == len(full['y']) - sum(1 for key in wt.OVER_CAP if key[:2] == (n, name))
    listed = dict((key, v) for key, v in wt.OVER_CAP.items() if key[0] == n)
    print('n = %d: levels of M up to %.1f FLOOR, of the rewritten boxes up to %.1f FLOOR; over the cap: %s' % (n, top_m, top_gap, over))
    assert sorted(over) == sorted(listed) and all(abs(over[key] - listed[key]) <= 0.1 * listed[key] for key in over)
    for name in wt.GROUPS:      # no edge has lost all its cases
        for case, _, _, other in wt.cases(n, name):
            assert (name, case) in edges_left or isinstance(other, list), (name, case)


def test_launch_plans_by_hand():
    """256 CUs.  cp_wallish_dd_box: (4 (n + 64) + 80) doubles of LDS = 35 456 bytes at n = 1024, 4 workgroups per CU, 1024 resident, 4096 sequences a trip;
    68 224 bytes at n = 2048, 2 per CU, 512 resident, 2048 sequences a trip.  cp_wallish_tail: 512 resident workgroups, a pair of rows each."""
    assert wt.dd_box_lds(1024) == 35456 and wt.dd_box_lds(2048) == 68224
    assert wt.dd_box_plan(1, 1024) == (1, 1) and wt.dd_box_plan(5, 1024) == (2, 1) and wt.dd_box_plan(4096, 1024) == (1024, 1)
    assert wt.dd_box_plan(4101, 1024) == (1024, 2) and wt.dd_box_plan(8193, 1024) == (1024, 3)
    assert wt.dd_box_plan(2048, 2048) == (512, 1) and wt.dd_box_plan(2053, 2048) == (512, 2) and wt.dd_box_plan(4097, 2048) == (512, 3)
    assert wt.dd_box_counts(1024) == [1, 3, 4, 5, 4101, 8193] and wt.dd_box_counts(2048) == [1, 3, 4, 5, 2053, 4097]
    assert wt.tail_plan(1) == (1, 1) and wt.tail_plan(5) == (3, 1) and wt.tail_plan(1024) == (512, 1)
    assert wt.tail_plan(1029) == (258, 2) and wt.tail_plan(2049) == (342, 3)      # 515 pairs in 2 trips, 1025 pairs in 3
    assert wt.tail_counts() == [1, 3, 4, 5, 1029, 2049]
    assert max(8193 * 1024, 4097 * 2048, 2049 * 4096) * 8 < 70e6      # the largest launch
    base = np.arange(6.).reshape(3, 2) + 1.
    rows = wt.cyclic(base, 7)
    assert np.array_equal(wt.uncycled(rows, 3), wt.cyclic(base, 3)[np.arange(7) % 3])


def restated(n, g, rows, search=None, solve=None, remove=None):
    """The scheme that runs at n, restated in float64, on the finite sequences ``rows`` of a group: (M, boxes, rewritten)."""
    y = g['y'][rows]
    mf, ms = g['margins']
    m = wt.m_recursive(y, **(solve or {})) if n == 2048 else wt.m_elimination(y, **(solve or {}))
    boxes = wt.box_rule(m, mf, ms, **(search or {})) + np.array(g['offsets'])
    rewritten = np.array([wt.remove_windowed(y[k:k + 1], int(a), int(b), composed=n == 2048, **(remove or {}))[0] for k, (a, b) in enumerate(boxes)])
    return m, boxes, rewritten


# (mutation, sizes, which stage, arguments, the (group, case) that rejects it)
MUTATIONS = [
    ('the second range starts at lower + 1', wt.SIZES, 'search', dict(lower_shift=1), ('m20_5', 'second_at_lower')),
    ('the upper end one knot further', wt.SIZES, 'search', dict(upper_shift=1), ('m20_5', 'decoys')),
    ('the upper end one knot short', wt.SIZES, 'search', dict(upper_shift=-1), ('m20_5', 'at_upper')),
    ('the last index on ties', wt.SIZES, 'search', dict(last=True), ('m20_5', 'zero')),
    ('the mirror term of knot 1 left out', [2048], 'solve', dict(mirror_first=False), ('m0_0', 'knot_0')),
    ('the mirror term of knot n - 2 left out', [2048], 'solve', dict(mirror_last=False), ('m0_0', 'knot_last')),
    ('a halo of 4 knots', [1024], 'solve', dict(halo=4), ('m20_5', 'plain')),
    ('a sweep from the true end started on a centred difference', wt.SIZES, 'remove', dict(start='centred'), ('m0_0', 'nl_0')),
    ('gtab[nl - 1] for gtab[nl]', wt.SIZES, 'remove', dict(gtab_shift=-1), ('m0_0', 'nl_1')),
    ('gtab[nr - 1] for gtab[nr]', wt.SIZES, 'remove', dict(gtab_shift=-1), ('m0_0', 'nr_1')),
    ('the rewrite loop stopped at 64 knots', wt.SIZES, 'remove', dict(loop_stop=64), ('m20_5', 'R_64')),
    ('the rewrite loop stopped at 64 knots', wt.SIZES, 'remove', dict(loop_stop=64), ('m20_5', 'long')),
    ('an invalid box clipped', wt.SIZES, 'remove', dict(clip_invalid=True), ('m1_0_wide', 'box_beyond')),
]


@pytest.mark.parametrize('n', wt.SIZES)
def test_restatement_passes(n):
    """The unmutated restatement of the scheme that runs is within the rule on every finite sequence of every group."""
    for name in wt.GROUPS:
        g = wt.group(n, name)
        rows = finite_rows(g)
        fails, worst_m, worst_gap = wt.judge(g, rows, *restated(n, g, rows))
        print('n = %d, %s: the restatement uses %.3g of the allowance of M, %.3g of the rewritten boxes' % (n, name, worst_m, worst_gap))
        assert not fails, (name, fails[:4])


@pytest.mark.parametrize('mutation', MUTATIONS, ids=lambda m: '%s [%s %s]' % (m[0], m[4][0], m[4][1]))
def test_mutations_are_rejected(mutation):
    what, sizes, stage, arguments, (name, case) = mutation
    for n in sizes:
        g = wt.group(n, name)
        rows = rows_of(g, case)
        assert rows, (n, name, case)
        assert not wt.judge(g, rows, *restated(n, g, rows))[0]
        fails = wt.judge(g, rows, *restated(n, g, rows, **{stage: arguments}))[0]
        assert fails, '%s is not rejected by %s %s at n = %d' % (what, name, case, n)
        print('n = %d: %s: rejected by %s %s: %s' % (n, what, name, case, fails[:3]))


@pytest.mark.parametrize('n', wt.SIZES)
def test_start_inside_is_forgotten(n):
    """A sweep that starts inside the sequence has 64 knots to the box: started on slope 0 instead of the centred difference it gives the same bits
    (0.268^63 = 1e-36 of the start arrives).  No case can reject that mutation; L_65 and R_63 are the ones that take those starts."""
    g = wt.group(n, 'm20_5')
    for case in ('L_65', 'R_63', 'long'):
        rows = rows_of(g, case)
        plain, mutated = restated(n, g, rows)[2], restated(n, g, rows, remove=dict(start='clamped'))[2]
        assert np.array_equal(plain, mutated), case
    assert float((2. - np.sqrt(3.))**63) < 1e-35


def test_comments_of_the_header():
    """Figures the comments of csrc/cp_wallish_dd.h state, measured: c_i = 1 / (4 - c_{i-1}) has its limit 2 - sqrt 3 to the last bit from knot 14 on
    (from 1/2) and knot 15 on (from 0), far inside the 40 entries of the tables; 0.268^32 = 5e-19 is what a halo of 32 knots leaves of a sweep's start,
    and the halo scheme in longdouble lies that far from the longdouble solve (relative to the largest |M|)."""
    ctab, gtab, c_last = wt.tables()
    limit = 2. - np.sqrt(3.)
    first_c = next(i for i in range(wt.DD_NTAB) if (ctab[i:] == ctab[-1]).all())
    first_g = next(i for i in range(wt.DD_NTAB) if (gtab[i:] == gtab[-1]).all())
    print('tables: c_i constant from knot %d (from 1/2) and %d (from 0); limit %.17g, last entries %.17g %.17g' % (first_c, first_g, limit, ctab[-1], gtab[-1]))
    assert first_c <= 16 and first_g <= 16 and abs(ctab[-1] - limit) <= 1.2e-16 and gtab[-1] == ctab[-1]
    assert 4e-19 < limit**32 < 6e-19
    y = st.gap_rows(1024)
    truth = wt.m_truth(y)
    halo = wt.m_elimination(y, dtype=LD)
    left = float((np.abs(halo - truth).max(axis=-1) / np.abs(truth).max(axis=-1)).max())
    print('halo of 32 knots in longdouble against the longdouble solve: %.3g of the largest |M|' % left)
    if np.finfo(LD).eps < 1e-18:      # (where longdouble is wider than double)
        assert left < 5e-18
    assert float((np.abs(wt.m_elimination(y, halo=4, dtype=LD) - truth).max(axis=-1) / np.abs(truth).max(axis=-1)).max()) > 1e-5
