"""CPU: the cases of tests/splice_truth.py exercise what they claim -- every S of the uniform-stretch kernel at 64 S and 64 (S - 4) + 1 knots, the last
knot of the stretch in a lane's first and last place, windows of 0, 1 and 44 knots, one and eight blocks of spline queries, the constant slot of the
elimination kernel on both sides of its threshold, halos of 8 to 48 knots, S = 1 to 61, the LDS bound of every family --, every block stays under its cap
in the float64 restatement of either scheme, and the tolerance rule notices the mistakes these kernels can make (made in the restatements, through their
``mistake`` keyword, never in the library)."""
import numpy as np
import pytest

import splice_truth as sp
import spline_truth as st

P = np.sqrt(3.) - 2.


def test_every_listed_case_is_there():
    sizes = {case[0] for case in sp.STRETCH.values()}
    assert {256, 1320, 1321, 2112, 2113, 2368, 2369, 2624, 2625, 2880, 2881, 3136, 3137, 3392, 3393, 3648, 257, 258, 400} <= sizes
    outside = {case[1:3] for case in sp.STRETCH.values() if case[0] == 300}
    assert {(10, 5), (1, 1), (2, 44), (45, 2), (0, 30), (50, 0), (0, 0)} <= outside
    assert all(case[1:3] == (50, 30) for name, case in sp.STRETCH.items() if name.startswith('nm') and '_' not in name)
    assert {case[0] for case in sp.ELIMINATION_ONLY.values()} == {3649, 255, 300}
    for S, sizes in sp.UNIFORM_S.items():
        assert 64 * S in sizes and (S == 33 or 64 * (S - 4) + 1 in sizes)
        assert all(sp.pick_S(nm) == S and 'nm%d' % nm in sp.STRETCH for nm in sizes)
    assert sorted(sp.UNIFORM_S) == [33, 37, 41, 45, 49, 53, 57] and sp.EPS == [0., 0., 1e-6, 1e-6, 1e-3, 1e-3, 1e-3]
    assert set(sp.GAPS) == {'nm300_1_1'} and all(front <= 2.5 and behind <= 3.5 for front, behind in sp.GAPS.values())
    assert sp.IRREGULAR_SIZES == [4, 5, 63, 64, 65, 128, 129, 192, 193, 700] and sp.BATCH_ROWS == [1, 3, 4, 5]


@pytest.mark.parametrize('name', list(sp.STRETCH) + list(sp.ELIMINATION_ONLY))
def test_stretch_cases(name):
    case = sp.stretch_case(name)
    nm, nl, nr, ni = case['nm'], case['nl'], case['nr'], case['ni']
    knots, xq, T, plan = case['knots'], case['xq'], case['tables'], case['plan']
    h = np.diff(knots)
    assert knots.size == nl + nm + nr and xq.size == nl + ni + nr and ni <= 513
    assert (h[nl:nl + nm - 1] == sp.H).all()      # exactly uniform
    if nl:
        assert h[nl - 1] == case['gaps'][0] * sp.H and np.allclose(h[:nl - 1][::-1], case['gaps'][0] * sp.H * 1.3**np.arange(1, nl))
    if nr:
        assert h[nl + nm - 1] == case['gaps'][1] * sp.H and np.allclose(h[nl + nm:], case['gaps'][1] * sp.H * 1.3**np.arange(1, nr))
    u = knots[nl:nl + nm]
    q = xq[case['interior']]
    assert set(case['blocks']) == {'stretch'} | ({'front'} if nl else set()) | ({'behind'} if nr else set())
    assert all(index.size >= 6 for index in case['blocks'].values())
    assert u[0] in q and u[-1] in q and np.nextafter(u[0], np.inf) in q and np.nextafter(u[-1], -np.inf) in q
    assert (not nl or np.nextafter(u[0], -np.inf) in q) and (not nr or np.nextafter(u[-1], np.inf) in q)
    assert np.isin(u[1:-1], q).sum() >= 5 and q.min() >= knots[max(nl - 1, 0)] and q.max() <= knots[min(nl + nm, knots.size - 1)]
    assert set(np.unique(case['tophat'][[0, 1]])) == {0., 1.} and ((case['tophat'] > 0.) & (case['tophat'] < 1.)).sum() > ni // 4
    # the plan of the elimination kernel: the constant slot of the stretch only past 256 equal spacings
    assert plan is not None and plan['S'] == ((knots.size + 63) // 64) | 1 and plan['run'] == (nl, nl + nm - 1)
    slot = plan['ntab_left'] < knots.size
    assert slot == (nm - 1 > 256)
    if slot:
        assert plan['uniform_end'] - plan['ntab_left'] > 128 and nl < plan['ntab_left'] <= nl + 12 and plan['uniform_end'] == nl + nm - 1
        assert plan['h0'] == sp.H
    # the uniform-stretch scheme
    if name in sp.ELIMINATION_ONLY:
        assert T is None and (sp.pick_S(nm) == 0 or nm < 256 or ni == 513)
    else:
        assert T is not None and T['S'] == sp.pick_S(nm) and T['nm'] == nm and (T['wl'], T['wr']) == (min(nl, 44), min(nr, 44))
        assert (T['gb0'], T['gfirst'], T['gend']) == (nl // 64, nl, nl + ni) and T['ngb'] == (nl + ni + 63) // 64 - nl // 64 <= 8
        tb = (nm - 1) - T['S'] * T['lane_b']
        assert 0 <= tb < T['S'] and np.isclose(T['mb0'], P**(tb - T['S']), rtol=1e-12) and np.isclose(T['mb1'], P**tb, rtol=1e-12)
        expect = {'nm256': dict(lane_b=7), 'nm1320': dict(tb=32, S=33), 'nm1321': dict(tb=0, S=33), 'gb0': dict(gb0=1, gfirst=70, ngb=7),
                  'generic512': dict(gb0=1, gfirst=64, ngb=8), 'generic60': dict(ngb=1), 'nm300_1_1': dict(wl=1, wr=1), 'nm300_0_0': dict(wl=0, wr=0)}
        for key, value in expect.get(name, {}).items():
            assert (tb if key == 'tb' else T[key]) == value, (name, key)
        if nm == 64 * T['S']:
            assert T['lane_b'] == 63 and tb == T['S'] - 1
    # the cap: a condition on the inputs
    worst = 0.
    for scheme in case['scheme']:
        for what in ('spline', 'damped'):
            for key, (columns, top, level) in sp.block_levels(case, scheme, what).items():
                worst = max(worst, level.max() / st.FLOOR)
                assert level.max() <= sp.STRETCH_CAP * st.FLOOR, (name, scheme, what, key, level.max() / st.FLOOR)
    print('%s: level at most %.3g FLOOR' % (name, worst))


def test_every_uniform_kernel_is_launched():
    assert {sp.stretch_case('nm%d' % nm)['tables']['S'] for sizes in sp.UNIFORM_S.values() for nm in sizes} == set(sp.UNIFORM_S)


@pytest.mark.parametrize('name', sp.IRREGULAR_FAMILIES)
def test_irregular_cases(name):
    largest = sp.largest_irregular(name)
    seen = {}
    for n in sp.IRREGULAR_SIZES + [largest]:
        case = sp.irregular_case(name, n)
        plan = case['plan']
        seen[n] = (plan['S'], plan['halo'])
        assert plan['S'] == ((n + 63) // 64) | 1 and (plan['halo'] < n or plan['halo'] == 8 * ((n + 7) // 8))
        xq, x = case['xq'], case['x']
        assert np.isnan(xq[1]) and xq[0] < x[0] and xq[2] > x[-1] and x[0] in xq and x[-1] in xq and np.isin(x[::plan['S']][:40], xq).all()
        top, level = st.levels(case['truth'], case['f8'])
        over = sp.IRREGULAR_OVER_CAP.get((name, n))
        if over is None:
            assert level.max() <= st.CAP * st.FLOOR, (name, n, level.max() / st.FLOOR)
        else:
            assert level.max() > st.CAP * st.FLOOR and abs(level.max() / st.FLOOR / over - 1.) < 0.05, (name, n, level.max() / st.FLOOR)
    assert sp.elimination_plan(sp.stc.knots(name, largest + 1)) is None
    assert [seen[n][0] for n in sp.IRREGULAR_SIZES] == [1, 1, 1, 1, 3, 3, 3, 3, 5, 11]
    expect = {'uniform': (3840, 61, 40), 'geom1.05': (3840, 61, 40), 'saw1.5x16': (2496, 39, 32), 'saw2x40': (2368, 37, 48), 'alt1e3': (2496, 39, 16),
              'jitter100': (2496, 39, 32)}[name]
    assert (largest,) + seen[largest] == expect
    assert seen[4] == seen[5] == (1, 8) and seen[63][1] == expect[2]      # fewer knots than the halo; the family's halo from 63 knots on
    if expect[0] < 3840:      # the LDS of a CU is what ends the family; more than 64 KiB: one workgroup per CU
        assert sp.irregular_case(name, largest)['plan']['lds_bytes'] > 150 * 1024
        assert sp.elimination_plan(sp.stc.knots(name, 2300)) is not None and sp.elimination_plan(sp.stc.knots(name, 2500)) is None
    if name == 'saw2x40':
        assert sp.elimination_plan(sp.stc.knots(name, 2400)) is None


def test_pieces_from_two_arrays():
    whole = sp.irregular_case('jitter100', 193)
    for key in sp.PIECES:
        case = sp.irregular_case('jitter100', 193, key)
        assert [p[0] for p in case['pieces']] == ([1, 0] if key == 'two' else [1, 0, 1])
        gathered = np.concatenate([case['rows'][src][:, start:start + count] for src, start, count in case['pieces']], axis=-1)
        assert np.array_equal(gathered, whole['y']) and np.array_equal(case['truth'], whole['truth'], equal_nan=True)


SEES = {'mb_exchanged': (1, ['nm256', 'nm1320', 'nm1321', 'nm3648', 'nm300_0_0']), 'carry_from_1': (1, ['nm256', 'nm1320', 'nm1321', 'nm3648', 'nm300_0_0']),
        'end_value': (1, ['nm256', 'nm1320', 'nm3648', 'nm300_1_1']), 'halo8': (0, ['nm256', 'nm1320', 'nm300_0_0', 'nm300_1_1', 'nm400']),
        'slot_early': (0, ['nm2112', 'nm300_0_0', 'nm300_1_1'])}


@pytest.mark.parametrize('mistake', list(SEES))
def test_the_rule_notices(mistake):
    """(slot_early is the faintest: the factor of the knot in front of the slot is 2e-10 from the constant, and the rule sees it at 1.1 to 1.2 allowances in
    the rows with 1e-3 noise of three cases; the others leave the allowance by factors of 1e5 and more.)"""
    scheme, names = SEES[mistake]
    for name in names:
        case = sp.stretch_case(name)
        right = sp.fraction_used(case, scheme, 'spline', case['scheme'][scheme]['spline'])
        assert max(f.max() for f in right.values()) <= 1. / st.ALLOW + 1e-12
        wrong = sp.fraction_used(case, scheme, 'spline', sp.restate(case, scheme, mistake=mistake))
        worst = max(f.max() for f in wrong.values())
        assert worst > 1., (mistake, name, worst)
        if mistake == 'end_value':
            assert wrong['behind'].min() > 1. and wrong['stretch'].max() < 1.      # every row, and only behind the stretch
        if mistake not in ('slot_early',):
            assert worst > 1e3


def test_irregular_rule_notices_a_short_halo():
    for name, n in (('saw2x40', 700), ('jitter100', 193), ('geom1.05', 700)):
        case = sp.irregular_case(name, n)
        top, level = st.levels(case['truth'], case['f8'])
        wrong = sp.eliminate(case['x'], case['y'], case['plan'], case['xq'], mistake='halo8')
        dist = np.nanmax(np.abs(wrong.astype(st.LD) - case['truth']), axis=-1)
        assert (np.asarray(dist / (st.ALLOW * level * top), dtype='f8') > 1.).all()


def test_levels_on_the_grids_of_wallish2018():
    """No cap: the levels the device test uses, printed.  The interval behind the stretch is about 1000 h long: the second derivatives of the uniform
    scheme, rounded to 1e-16 of the SECOND DIFFERENCES' scale, weigh (H / h)^2 there."""
    case = sp.production_case()
    assert case['tables'] is not None and case['tables']['S'] == 49 and case['nm'] == 3051 and case['plan']['S'] == 59
    for scheme in (1, 0):
        for what in ('spline', 'damped'):
            levels = {key: level.max() / st.FLOOR for key, (columns, top, level) in sp.block_levels(case, scheme, what).items()}
            print('wallish2018 grids, scheme %d, %s: levels (FLOOR) %s' % (scheme, what, {key: float('%.3g' % value) for key, value in levels.items()}))
            if what == 'damped':
                assert levels['behind'] < 2.      # the tophat is 0 there: the output is P itself
    behind = sp.block_levels(case, 1, 'spline')['behind'][2].max() / st.FLOOR
    assert behind > 1e3
