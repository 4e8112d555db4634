"""CPU: the truth of tests/tables_truth.py and the cases tests/test_tables_truth_gpu.py runs on the device.  The truth agrees with scipy's two CubicSpline
passes; every case used on the device has a restatement level of at most CAP x FLOOR (a case above it would be redrawn with another seed, never given a
wider tolerance: OVER_CAP is empty); every exponent case lies on the side of 300 / 308.25 / -323.3 it claims, in longdouble; and the rule itself sees
the defects it is there for."""
import numpy as np
import pytest

import tables_truth as tt
from spline_truth import LD, FLOOR, CAP

OVER_CAP = {}      # case -> level in FLOORs: none


def device_cases():
    """Every case of tests/test_tables_truth_gpu.py but the batches (below) and the exponent route."""
    out = [dict(nq=nq) for nq in tt.NQ]
    out += [dict(nzq=nzq, nq=nq, zq=zq) for nzq in tt.NZQ for nq in tt.NZQ_NQ for zq in ('beyond', 'nan_z')]
    out += [dict(nzin=nzin, nzq=64, nq=80, zq='inside') for nzin in tt.NZIN] + [dict(nzin=nzin) for nzin in tt.NZIN]
    out += [dict(n=n, kq=kq) for n in tt.N_KNOTS for kq in ('inside', 'outside')]
    out += [dict(scale=scale, kind=kind, nzq=64, nq=80, zq='inside') for scale in tt.SCALES for kind in ('plain', 'signed')]
    out += [dict(nzq=64, nq=128, zq='inside')]
    return out


def test_levels_under_the_cap():
    worst = 0.
    for kw in device_cases():
        c = tt.case(**kw)
        assert c['level_floors'] <= CAP, (kw, c['level_floors'])
        assert (c['top'] > 0).all() and np.isfinite(c['t']).all()
        worst = max(worst, c['level_floors'])
    print('levels of the restatement, in FLOORs: at most %.1f over %d cases' % (worst, len(device_cases())))


@pytest.mark.parametrize('kernel,nq', [('direct', 256), ('direct', 513), ('rows', 256), ('rows', 300)])
def test_batch_levels(kernel, nq):
    counts = (tt.DIRECT_BATCHES if kernel == 'direct' else tt.ROWS_BATCHES)[nq]
    c = tt.case(nb=max(counts), nq=nq, **tt.TINY_TABLES)
    print('%s batches of %d tables, nq = %d: level at most %.1f FLOOR' % (kernel, max(counts), nq, c['level_floors']))
    assert c['level_floors'] <= CAP
    short = tt.case(nb=min(counts), nq=nq, **tt.TINY_TABLES)      # a longer batch begins with the tables of a shorter one
    assert np.array_equal(short['t'], c['t'][:min(counts)]) and np.array_equal(short['truth'], c['truth'][:min(counts)])


def test_wide_levels():
    for nq in tt.WIDE_NQ:
        c = tt.wide_case(nq)
        assert c['level_floors'] <= CAP and c['cols'][0] == 0 and c['cols'][-1] == nq - 1 and c['xq'].size == nq and (np.diff(c['xq']) >= 0).all()


@pytest.mark.parametrize('kw', [dict(), dict(nzin=17, nzq=64, nq=80, zq='inside'), dict(n=100, kq='outside'), dict(nzin=3), dict(nzin=2)], ids=str)
def test_truth_against_scipy(kw):
    from scipy.interpolate import CubicSpline, interp1d
    c = tt.case(**kw)
    inside = ~np.isnan(c['truth'][0, 0])
    bc = c['zbc']
    for b in range(c['shape'][0]):
        low = CubicSpline(c['x'], c['t'][b], axis=1, bc_type='not-a-knot')(c['xq'][inside])
        if c['zk'].size == 2:
            two = interp1d(c['zk'], low, axis=0, fill_value='extrapolate')(c['zq'])
        else:
            two = CubicSpline(c['zk'], low, axis=0, bc_type=bc, extrapolate=True)(c['zq'])
        np.testing.assert_allclose(np.asarray(c['truth'][b][:, inside], dtype='f8'), c['scale'] * two, rtol=0, atol=2e-12 * float(c['top'][b]))


@pytest.mark.parametrize('negative_scale', [False, True])
@pytest.mark.parametrize('nq', sorted(tt.BUMP_TILE))
@pytest.mark.parametrize('name', list(tt.EXPONENT_TARGETS))
def test_exponent_cases_lie_where_they_claim(name, nq, negative_scale):
    c = tt.exponent_case(name, nq, negative_scale)
    peak, rest = tt.tile_extremes(c)
    assert rest < 299 and c['level_floors'] <= CAP and (c['scale'] < 0) == negative_scale
    lo = 16 * c['tile']
    a = c['truth'][:, :, lo:lo + 16] * c['sign']      # the arguments of the bump's tile, positive
    assert (a > 0).all() and a.max() == peak
    if name == '299.9':
        assert 299.8 < peak < 299.95
    elif name == '300-':
        assert LD(300) * (1 - LD(2) ** -50) < peak < 300
    elif name == '300':
        assert 300 <= peak < LD(300) * (1 + LD(2) ** -50)
    elif name == '300.1':
        assert 300.05 < peak < 300.2
    elif name == 'inf':      # arguments in (308.25, 308.3]: Inf
        assert c['sign'] > 0 and 308.2547155599168 < peak <= 308.3 and (tt.lt.exp10_truth(a) > tt.DBL_MAX).any()
    elif name == 'subnormal':      # arguments in (-323.3, -307.7): subnormal results, none that rounds to 0
        assert c['sign'] < 0 and ((a > 307.7) & (a < 323.3)).any() and peak < 323.3
    else:                          # below -324: 0, and subnormal results on the way
        assert c['sign'] < 0 and (a > 324).any() and ((a > 307.7) & (a < 323.3)).any()


def test_the_rule_sees_defects():
    """A result with one element off by 20 levels, a NaN missing, an Inf or a 0 where 10^x is finite: fraction() says so."""
    c = tt.case(nzq=64, nq=80, zq='inside')
    arg = np.asarray(c['truth'], dtype='f8')
    assert tt.fraction(arg, c) <= 1. / 16 + 1e-3
    off = arg.copy()
    off[1, 5, 7] += 20 * c['level'][1] * float(c['top'][1])
    assert tt.fraction(off, c) > 1.
    with pytest.raises(AssertionError):
        bad = arg.copy()
        bad[0, 0, 0] = np.nan
        tt.fraction(bad, c)
    ten = 10. ** arg
    assert tt.fraction(ten, c, 'exp10') <= 1.
    for wrong in (np.inf, 0.):
        with pytest.raises(AssertionError):
            bad = ten.copy()
            bad[2, 3, 4] = wrong
            tt.fraction(bad, c, 'exp10')
    e = tt.exponent_case('zero', 64)
    with np.errstate(under='ignore'):
        ten = np.asarray(tt.lt.exp10_truth(e['truth']), dtype='f8')
    assert tt.fraction(ten, e, 'exp10') <= 1. and (ten == 0).any()
    e = tt.exponent_case('subnormal', 64)
    with np.errstate(under='ignore'):
        ten = np.asarray(tt.lt.exp10_truth(e['truth']), dtype='f8')
    assert tt.fraction(ten, e, 'exp10') <= 1. and (ten > 0).all()
    shifted = ten.copy()
    sub = (ten > 0) & (ten < 1e-314)      # (the relative part of the allowance below a twentieth of a unit)
    shifted[sub] += 3 * 4.9406564584124654e-324
    assert sub.any() and tt.fraction(shifted, e, 'exp10') > 1.
    s = tt.case(scale=1., kind='signed', nzq=64, nq=80, zq='inside')
    with np.errstate(invalid='ignore'):
        roots = np.sqrt(np.asarray(s['truth'], dtype='f8'))
    assert np.isnan(roots).any() and tt.fraction(roots, s, 'sqrt') <= 1.
