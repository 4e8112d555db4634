"""CPU: the cases of tests/brieden_truth.py exercise what they claim (every S = 3 .. 8, the last lane full, owning one knot, straddling; queries on the
knots, a hair off them and in the four extrapolated intervals; both sides of the OPLDS threshold), every row's level stays under CAP = 32 FLOOR, and the
tolerance rule notices the mistakes this kernel can make -- made in the numpy restatement, through its ``mistake`` keyword, never in the library."""
import numpy as np
import pytest

import brieden_truth as bt
import spline_truth as st


def _levels(case):
    top, level = st.levels(case['truth'], case['f8'])
    assert (top > 1.).all()      # v = log10 P: a scale of its own, no cancellation
    return level / st.FLOOR


def test_the_sizes_cover_every_lane_shape():
    assert sorted({bt.samples_per_lane(n) for n in bt.SIZES}) == [3, 4, 5, 6, 7, 8]
    kinds = {n: bt.last_lane(n) for n in bt.SIZES}
    assert kinds == {129: 'full', 191: 'straddle', 192: 'full', 193: 'one', 256: 'full', 257: 'straddle', 320: 'full', 321: 'straddle', 384: 'full', 385: 'full',
                     448: 'full', 449: 'one', 511: 'straddle', 512: 'full'}
    for S in range(3, 9):      # 64 S: lane 63 full; 64 (S - 1) + 1: the smallest n of this S
        assert 64 * S in bt.SIZES and 64 * (S - 1) + 1 in bt.SIZES
    assert [bt.samples_per_lane(n) for n in bt.UNSUPPORTED] == [2, 9]
    assert sorted(bt.samples_per_lane(n) for n in bt.BENT) == [5, 7]
    assert {bt.samples_per_lane(n) for n, npk in bt.SMOOTH} == {3, 4, 5, 6, 7, 8}
    counts = [npk for n, npk in bt.SMOOTH]
    assert {1, 2, 23, 24, 63, 64, 32, 33} <= set(counts)
    # the operator's columns in LDS or not: (341, 32) and (341, 33) both lie beyond the threshold of launch_resample, (341, 31) is the last that fits
    assert [bt.oplds(341, npk)[0] for npk in (31, 32, 33)] == [True, False, False]
    assert not bt.oplds(512, 23)[0] and bt.oplds(129, 64)[0] and bt.oplds(129, 64)[1] > 64 * 1024
    assert all(bt.oplds(n, npk)[1] <= 160 * 1024 - 2048 for n, npk in bt.SMOOTH)
    assert bt.RESCALE[0] == 1. and bt.RESCALE.min() == 0.85 and bt.RESCALE.max() == 1.2 and np.unique(bt.RESCALE).size == bt.NRESCALE


def _where(case):
    """Per distinct row, how many queries fall in each of the four extrapolated intervals and on the uniform stretch."""
    counts = []
    for r in case['rescale']:
        x = np.log10(case['k_fid'] / r)
        xq = case['log_k_fid']
        counts.append(((xq < x[0]).sum(), (xq > x[-1]).sum()))
    return np.array(counts)


@pytest.mark.parametrize('n', bt.SIZES)
def test_resample_cases_stay_under_the_cap(n):
    case = bt.resample_case(n)
    level = _levels(case)
    print('cp_brieden_resample, %d samples: level at most %.3g FLOOR' % (n, level.max()))
    assert level.max() <= bt.CAP
    where = _where(case)
    assert where[3, 0] > 0 and where[3, 1] == 0 and where[4, 1] > 0 and where[4, 0] == 0      # 0.85: knots moved up, queries below them; 1.2: above
    assert np.isfinite(case['truth'].astype('f8')).all()
    # rescale 1: the spline at its own knots
    np.testing.assert_allclose(case['truth'][0].astype('f8'), np.log10(case['samples'][0]), rtol=0, atol=2e-15)


@pytest.mark.parametrize('first', ['zero', 'end'])
@pytest.mark.parametrize('n', [191, 257, 512])
def test_resample_cases_at_the_ends_of_the_rows(n, first):
    for bounds in ((bt.KMIN, bt.KMAX), bt.TIGHT):
        case = bt.resample_case(n, first, bounds)
        assert case['first'] == (0 if first == 'zero' else case['nk'] - n)
        level = _levels(case)
        assert level.max() <= bt.CAP
        if bounds == bt.TIGHT:      # the second argument of fmin / fmax is taken
            if first == 'zero':
                assert (case['k_fid'][0] / case['rescale'] < bounds[0]).all() and (case['rescale'] >= 1.).all()
            else:
                assert (case['k_fid'][-1] / case['rescale'] > bounds[1]).all() and (case['rescale'] <= 1.).all()
        else:
            assert case['k_fid'][0] / case['rescale'].min() > bounds[0] and case['k_fid'][-1] / case['rescale'].max() < bounds[1]


@pytest.mark.parametrize('n,npk', bt.SMOOTH)
def test_smooth_cases_stay_under_the_cap(n, npk):
    case = bt.smooth_case(n, npk)
    level = _levels(case)
    print('cp_brieden_smooth, %d samples, %d extrema: level at most %.3g FLOOR' % (n, npk, level.max()))
    assert level.max() <= bt.CAP
    assert case['peaks'][0] == 0 and (npk == 1 or case['peaks'][-1] == n - 1) and np.unique(case['peaks']).size == npk


def _fraction(case, result):
    """The largest fraction of the device's allowance that a float64 result uses, row by row."""
    top, level = st.levels(case['truth'], case['f8'])
    dist = np.abs(result.astype(st.LD) - case['truth']).max(axis=-1)
    return np.asarray(dist / (st.ALLOW * level * top), dtype='f8')


@pytest.mark.parametrize('n', bt.SIZES)
def test_the_rule_notices_a_missing_A_correction(n):
    case = bt.resample_case(n)
    assert _fraction(case, case['scheme']).max() <= 1. / st.ALLOW + 1e-12
    fraction = _fraction(case, bt.mistaken(case, 'no_A'))
    off_knots = np.abs(case['row_rescale'] - 1.) > 1e-3      # rescale 1 (+- 1e-9): every query on (next to) a knot, where the second derivatives do not enter
    assert (fraction[off_knots] > 1.).all(), fraction[off_knots].min()


@pytest.mark.parametrize('n', bt.SIZES)
def test_the_rule_notices_tlast_in_a_straddling_lane(n):
    case = bt.resample_case(n)
    fraction = _fraction(case, bt.mistaken(case, 'tlast'))
    if bt.last_lane(n) == 'full':      # no lane straddles: the same arithmetic
        assert np.array_equal(bt.mistaken(case, 'tlast'), case['scheme'], equal_nan=True)
    else:
        # the knots moved down: queries in the last intervals of the stretch and beyond it, where B p^(n-1-i) has not died away (moved up by 0.85, the
        # last query lies five intervals below the last knot and the samples, all but a power law there, leave B small: not noticed in every row)
        reach = case['row_rescale'] > 1.01
        assert reach.sum() >= 3 * bt.NBASE and (fraction[reach] > 1.).all(), fraction[reach].min()
