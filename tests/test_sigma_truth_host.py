"""CPU: tests/sigma_truth.py is what it says before tests/test_sigma_tail_edges_gpu.py and tests/test_sigma_rz_edges_gpu.py judge a kernel by it.
(a) Truths hold.  The tap transform at n = 1024, npad = 2048 against the O(N^2) longdouble DFT of the promise (that of tests/test_fftlog_taps_host.py),
    for the generic and the power-law tables.  The natural spline in longdouble is spline_truth.spline, held to scipy and to an independent Thomas solve by
    tests/test_spline_truth_host.py.  The band truth is a longdouble matrix product, held here to numpy's float64 product.  The two float64 restatements
    of the geometric spline (the CU solve with its carries, the prefiltered transform with its four cubic pieces) against scipy's natural CubicSpline of
    the same float64 rows at float64 level, and the halo: |pL|^33 below FLOOR, and the longdouble spline through the knots of the stretch alone within
    FLOOR of the spline through all 1024.  band_of (plan_from_dense restated) reproduces W, and gives the 1e-18 band of a real natural spline operator.
(b) Cap.  Every shipped case lies below CAP = 32 floors in every block; the levels are printed.
(c) Root.  The truth of every case that takes the root is at least 1/4 of its scale at every finite radius.
(d) Mutations of the float64 restatements leave their allowance in at least one shipped case, named in the output.
(e) Pairs.  The kernels pack two rows into one complex transform and leave a pair unscaled while the exponents of its rows differ by at most 4
    (cp_fftlog_body.h, "Row independence"); rounding is then relative to the larger row.  The packed float64 transform of (row a, row b 2^-d) shows it:
    the smaller row's distance from its truth grows like 2^d, and stays within pair_factors x CAP floors."""
import ctypes

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

import fftlog_taps_truth as tt
import sigma_truth as sg
from test_fftlog_taps_host import direct_dft

LD = sg.LD


@pytest.fixture(scope='module')
def basis():
    from cosmoprimo_amd import _lib
    out = np.zeros(16)
    _lib.check(_lib.load().cp_geospline_basis(ctypes.c_double(sg.RHO), _lib.as_double_p(out)))
    return out.reshape(4, 4)


@pytest.mark.parametrize('kind', ['generic', 'power'])
def test_transform_truth_is_the_promise_at_2048(kind):
    syn, base = sg.tables(kind), sg.base_rows()
    true, f64 = sg.transform(syn, base)
    ref = direct_dft(base, sg.N, sg.NPAD, syn.pre[0], syn.post[0], tt.u_table(sg.NPAD, syn.taps[0], dtype=LD), 0, False)
    # relative to the sample's own postfactor (the power law spans 13 decades over the crop): two sums of Np terms, every term rounded once
    tilt = np.abs(syn.post[0][sg.OUT_LEFT:sg.OUT_LEFT + sg.N]).astype(LD)
    err = float((np.abs(true - ref) / tilt).max() / (np.abs(ref) / tilt).max())
    print('%s tables: truth against the direct DFT %.3g (longdouble eps %.3g)' % (kind, err, float(np.finfo(LD).eps)))
    assert err <= 4 * sg.NPAD * float(np.finfo(LD).eps)
    top, level = tt.levels(true / tilt, f64 / tilt)
    assert float(level.max()) <= sg.CAP * sg.FLOOR


def test_grid_and_halo():
    s = sg.S_GRID
    assert np.abs(s[1:] / (s[:-1] * sg.RHO) - 1.).max() < 1e-14      # the plan asks for 1e-12
    post = sg.tables('power').post[0]
    assert np.abs(post[1:] / (post[:-1] * float(sg.LAMBDA_LD)) - 1.).max() < 1e-14      # ... and for 1e-11 here
    pL, pR, kappa = sg.geo_roots()
    print('|pL| = %.4f, |pR| = %.4f, |pL|^33 = %.3g, |pR|^33 = %.3g' % (abs(pL), abs(pR), abs(pL)**33, abs(pR)**33))
    assert 0.27 < abs(pL) < 0.28 and abs(pL)**33 < sg.FLOOR / 100 and abs(pR)**33 < sg.FLOOR / 100
    # the roots solve the recurrence of the constant tridiagonal system
    a, b, c = sg.RHO_LD**2, 2 * (1 + sg.RHO_LD), 1 / sg.RHO_LD
    assert abs(c * pL**2 + b * pL + a) < 1e-17 and abs(a * pR**2 + b * pR + c) < 1e-17
    # what the stretch forgets: the longdouble natural spline through the knots ws - 1 ... ws + ne alone against the one through all knots
    for name in ('S4_full', 'low_end', 'high_end', 'S8_full'):
        case = sg.cu_case(name)
        ws, ne, S = case['plan']
        inside = np.isfinite(case['true'][0])
        part = sg.spline_truth(s[ws - 1:ws + ne + 1], case['y_true'][:, ws - 1:ws + ne + 1], case['r'])
        forgotten = float((np.abs(part - case['true'])[:, inside] / case['scale'][:, inside]).max())
        print('%s: stretch of %d knots from %d, forgotten %.3g of the scale' % (name, ne, ws, forgotten))
        assert forgotten < sg.FLOOR


def test_band_of_is_plan_from_dense():
    for name, nq, bw, *_ in sg.band_cases():
        case = sg.band_case(name)
        wb, j0, width = sg.band_of(case['w'])
        assert width == bw and wb.shape == (bw, nq)
        back = np.zeros_like(case['w'])
        for q in range(nq):
            if j0[q] < 0:
                back[q] = np.nan
                continue
            for i in range(bw):
                if wb[i, q] != 0.:
                    assert j0[q] + i < sg.N      # padded entries beyond knot 1023 carry no weight
                    back[q, j0[q] + i] = wb[i, q]
        assert np.array_equal(back, case['w'], equal_nan=True)
        if nq >= 16 and bw >= 2:
            assert (j0 + bw > sg.N).any(), 'no band reaches beyond the last knot after padding'
            assert (j0 == 0).any() and ((j0 + bw == sg.N) & (wb[-1] != 0.)).any() and (j0 < 0).any()
        # the truth is the dense product: numpy's float64 product of the rounded truth agrees at float64 level
        plain = sg.band_product(case['w'], np.asarray(case['y_true'], dtype='f8'))
        assert sg.fraction(plain, case['true'], case['scale'], np.full((2, 1), 8 * sg.FLOOR), what=name + ', float64 product of the rounded truth') <= 1.
        # ... and the sum in the kernel's order is the same operator
        assert sg.fraction(sg.band_restated(case['w'], case['y_f64']), case['true'], case['scale'], 4 * case['level'], what=name + ', band order') <= 1.


def test_real_spline_operator_band():
    """The natural spline from the geometric grid as a dense operator: its band at the 1e-18 threshold of plan_from_dense."""
    r = sg.radii(130, 100, 900, seed=11, outside=True)
    w = sg.spline_operator(sg.S_GRID, r)
    wb, j0, bw = sg.band_of(w)
    print('natural spline operator on the geometric grid: bandwidth %d' % bw)
    assert 40 <= bw <= 70      # 0.27^d reaches 1e-18 at d = 32 on either side of the interval
    case = sg.spline_operator_case()
    assert float(case['level'].max()) <= sg.CAP * sg.FLOOR


def test_restatements_are_the_natural_spline(basis):
    for name in ('S4_full', 'S6_first', 'S8_full', 'low_end', 'high_end'):
        case = sg.cu_case(name)
        inside = np.isfinite(case['true'][0])
        ref = CubicSpline(sg.S_GRID, case['y_f64'], axis=-1, bc_type='natural')(case['r'])
        for what, f64 in (('plain', case['plain']), ('CU solve', case['f64'])):
            assert np.isnan(f64[:, ~inside]).all()
            err = float((np.abs(f64 - ref)[:, inside] / np.asarray(case['scale'], dtype='f8')[:, inside]).max())
            print('%s, %s against scipy: %.3g' % (name, what, err))
            assert err < 64 * sg.FLOOR
    for name in ('nq257', 'ne510', 'low_end', 'high_end'):
        case = sg.prefiltered_case(name, basis)
        inside = np.isfinite(case['true'][0])
        ref = CubicSpline(sg.S_GRID, case['y_f64'], axis=-1, bc_type='natural')(case['r'])
        err = float((np.abs(case['f64'] - ref)[:, inside] / np.asarray(case['scale'], dtype='f8')[:, inside]).max())
        print('%s, prefiltered against scipy: %.3g' % (name, err))
        assert err < 64 * sg.FLOOR


def every_case(basis):
    for name, *_ in sg.band_cases():
        yield 'band', sg.band_case(name)
    yield 'band', sg.spline_operator_case()
    for name, *_ in sg.cu_cases():
        yield 'cu', sg.cu_case(name)
    for name, *_ in sg.prefiltered_cases():
        yield 'prefiltered', sg.prefiltered_case(name, basis)


def test_every_case_is_below_the_cap(basis):
    for family, case in every_case(basis):
        level = float(case['level'].max() / sg.FLOOR)
        print('%-12s %-20s level %5.1f FLOOR' % (family, case['name'], level))
        assert level < sg.CAP, (family, case['name'])
    for family in ('cu', 'prefiltered'):
        case = sg.mixed_sign_case(family, basis)
        level = float(case['level'].max() / sg.FLOOR)
        print('%-12s %-20s level %5.1f FLOOR (held squared)' % (family, case['name'], level))
        assert level < sg.CAP and (case['true'][np.isfinite(case['true'])] < 0).any()


def test_root_condition(basis):
    count = 0
    for family, case in every_case(basis):
        if not case['post_sqrt']:
            continue
        count += 1
        finite = np.isfinite(case['true']) & (case['true'] != 0)      # (a row of zeros of the operator: exactly 0, and its root)
        ratio = float((case['true'][finite] / case['scale'][finite]).min())
        print('%-12s %-20s truth at least %.3f of its scale' % (family, case['name'], ratio))
        assert ratio >= 0.25 and (case['base'] > 0).all() and (case['syn'].pre > 0).all() and (case['syn'].post > 0).all()
    assert count >= 4


def caught(case, wrong, what):
    """True when the mutated restatement leaves the allowance of the case."""
    try:
        with np.errstate(invalid='ignore'):
            values = np.sqrt(wrong) if case['post_sqrt'] else wrong
        return sg.fraction(values, case['true'], case['scale'], case['level'], case['post_sqrt'], sg.SQRT_EXTRA if case['post_sqrt'] else 0.,
                           what='%s, %s' % (what, case['name'])) > 1.
    except AssertionError:      # NaN in other places
        return True


def honest(case):
    with np.errstate(invalid='ignore'):
        values = np.sqrt(case['f64']) if case['post_sqrt'] else case['f64']
    return sg.fraction(values, case['true'], case['scale'], case['level'], case['post_sqrt'], what='the restatement itself, ' + case['name'])


@pytest.mark.parametrize('mutation', ['shift', 'last_chunk', 'second_query', 'swap_rows'])
def test_band_mutations(mutation):
    names = []
    for name, nq, bw, *_ in sg.band_cases():
        case = sg.band_case(name)
        assert honest(case) <= 1. / sg.ALLOW
        if caught(case, sg.band_restated(case['w'], case['y_f64'], mutation), mutation):
            names.append(name)
    print('%s caught by: %s' % (mutation, ', '.join(names)))
    assert names
    if mutation == 'second_query':
        assert all(int(name.split('_')[-2][2:]) > 128 for name in names)
    if mutation == 'last_chunk':      # every width catches it, 8 and 16 (whose last chunk is a whole one) included
        assert {'nq257_bw%d' % bw for bw in sg.BAND_WIDTHS if bw != 44} <= set(names)


def test_cu_mutations():
    carry, swap = [], []
    for name, *_ in sg.cu_cases():
        case = sg.cu_case(name)
        assert honest(case) <= 1. / sg.ALLOW
        ws, ne, S = case['plan']
        qj = sg.locate(sg.S_GRID, case['r'])[0]
        lanes = np.unique((qj[qj >= 0] - ws) // S)
        hits = [int(lane) for lane in lanes if caught(case, sg.cu_restated(sg.S_GRID, case['y_f64'], case['r'], ('carry', int(lane))), 'carry of lane %d' % lane)]
        if hits:
            carry.append('%s (S = %d: %d of %d lanes)' % (name, S, len(hits), len(lanes)))
        if caught(case, case['f64'][::-1], 'rows swapped'):
            swap.append(name)
    print('a lane without its first carry caught by: %s' % ', '.join(carry))
    print('rows a and b swapped caught by: %s' % ', '.join(swap))
    assert {c.split()[0] for c in carry} >= {'S%d_full' % S for S in range(sg.SMIN, sg.SMAX + 1)} and swap


def test_prefiltered_mutations(basis):
    interval, x, swap = [], [], []
    for name, *_ in sg.prefiltered_cases():
        case = sg.prefiltered_case(name, basis)
        assert honest(case) <= 1. / sg.ALLOW
        inside = np.flatnonzero(sg.locate(sg.S_GRID, case['r'])[0] >= 0)
        q = int(inside[len(inside) // 2])
        if caught(case, sg.prefiltered_restated(case['syn'], case['base'], sg.S_GRID, case['r'], basis, ('interval', q)), 'interval of radius %d off by one' % q):
            interval.append(name)
        if caught(case, sg.prefiltered_restated(case['syn'], case['base'], sg.S_GRID, case['r'], basis, 'x'), 'x for 1 - x'):
            x.append(name)
        if caught(case, case['f64'][::-1], 'rows swapped'):
            swap.append(name)
    print('interval off by one caught by: %s' % ', '.join(interval))
    print('x where 1 - x belongs caught by: %s' % ', '.join(x))
    assert interval and x and swap


def test_store_mutations():
    """The three store paths of sigma_rz_kernel, thread by thread: every element written once with its own product; q and z transposed, and the
    fixed-factor path taken for an nz that does not divide 256, are caught."""
    rng = np.random.default_rng(3)
    transposed, fixed = [], []
    for nq, nz in sg.RZ_SHAPES:
        vr, gr = rng.uniform(0.5, 1.5, nq), rng.uniform(0.5, 1.5, nz)
        true = vr.astype(LD)[:, None] * gr.astype(LD)[None, :]
        out = sg.store_rows(vr, gr)
        assert np.array_equal(out, vr[:, None] * gr[None, :])      # every element written, with its own product
        wrong = sg.store_rows(vr, gr, 'transpose')
        if float((np.abs(wrong - true) / true).max()) > sg.ALLOW * sg.FLOOR:
            transposed.append((nq, nz))
        if nz % 2 == 0:
            wrong = sg.store_rows(vr, gr, 'dz0')
            if 256 % nz:
                if not np.isfinite(wrong).all() or float((np.abs(wrong - true) / true).max()) > sg.ALLOW * sg.FLOOR:
                    fixed.append((nq, nz))
            else:
                assert np.array_equal(wrong, out)
    print('q and z transposed caught by (nq, nz): %s' % transposed)
    print('the dz == 0 store path for another nz caught by (nq, nz): %s' % fixed)
    assert set(transposed) == {(nq, nz) for nq, nz in sg.RZ_SHAPES if nq > 1 and nz > 1}
    assert {nz for nq, nz in fixed} == {66, 258}


def test_packed_pairs_cost_the_ratio():
    for kind in ('generic', 'power', 'spread'):
        syn, base, y_true, y_f64 = sg._transformed(kind, False)
        tilt = np.abs(syn.post[0][sg.OUT_LEFT:sg.OUT_LEFT + sg.N]).astype(LD)
        top = (np.abs(y_true) / tilt).max(axis=-1)
        alone = float(((np.abs(y_f64 - y_true) / tilt).max(axis=-1) / top).max() / sg.FLOOR)
        line = []
        for d in range(0, sg.ROW_SCALE_SPREAD + 1):
            exps = np.array([0, -d])
            packed = sg.packed_restated(syn, base * np.ldexp(1., exps)[:, None]) * np.ldexp(1., -exps)[:, None]
            factor = sg.pair_factors(syn, base, exps)
            dist = (np.abs(packed - y_true) / tilt).max(axis=-1) / top / sg.FLOOR
            line.append('d = %d: %.1f, %.1f floors (factors %.2f, %.2f)' % (d, dist[0], dist[1], factor[0], factor[1]))
            assert (dist <= factor * sg.CAP).all() and factor[0] <= 2. and 2.**(d - 1) < factor[1] < 2.**(d + 1)
        print('%s tables, a row alone %.1f floors; packed with a partner: %s' % (kind, alone, '; '.join(line)))
    # beyond the spread the kernel scales both rows: no factor
    assert (sg.pair_factors(syn, base, np.array([0, -6, 300, -300, 0])) == 1.).all()
    assert (sg.pair_factors(syn, base, np.array([0, -2]), nan_rows=(1,)) == 1.).all()


def test_rz_cases_are_below_the_cap_and_keep_the_root_condition(basis):
    """Every launch of tests/test_sigma_rz_edges_gpu.py: the level of every (cosmology, radius) block below CAP, the truth at least 1/4 of its scale (its
    square: the variance at least 1/16 ... the condition is on the argument of the root, truth^2 >= scale^2 / 4), the spectra below power_truth's cap, and the
    tilted rows of a pair within 2^4 of each other."""
    import power_truth as pt
    worst = {}
    for engine, form, nq, nz, ncosmo, nan, pk_out in sg.rz_cases():
        case = sg.rz_case(engine, form, nq, nz, ncosmo, basis, nan)
        level, stepped = float(case['level_plain'].max() / sg.FLOOR), float(case['level'].max() / sg.FLOOR)
        finite = np.isfinite(case['true']) & (case['true'] != 0)
        ratio = float(((case['true'][finite] / case['scale'][finite])**2).min())
        key = (engine, form)
        old = worst.get(key, (0., 0., 1e9))
        worst[key] = (max(old[0], level), max(old[1], stepped), min(old[2], ratio))
        assert level < sg.CAP and ratio >= 0.25, (engine, form, nq, nz, ncosmo, level, ratio)
    for (engine, form), (level, stepped, ratio) in worst.items():
        print('sigma(r, z) %-24s %-12s level at most %5.1f FLOOR (%5.1f with the spectra at the kernel\'s stepped k), variance at least %.3f of its scale'
              % (engine, form, level, stepped, ratio))
    k = sg.stepped_k()
    print('stepped k against the table: at most %.3g; per eighth of the grid: %s' % (np.abs(k / sg.K - 1.).max(), ' '.join(
        '%.2g' % np.abs(k[i:i + 128] / sg.K[i:i + 128] - 1.).max() for i in range(0, 1024, 128))))
    assert np.abs(k / sg.K - 1.).max() < 1e-14
    for engine in pt.ENGINES:
        true, f64, x = sg.rz_spectra(engine)
        floors = pt.level_floors(engine, 'matter', sg.K, true, f64, x)
        tilted = np.abs(np.asarray(true, dtype='f8') * sg.rz_tables('generic', engine).pre[0][sg.OUT_LEFT:sg.OUT_LEFT + sg.N]).max(axis=-1)
        spread = float(tilted.max() / tilted.min()) * 4.**np.ptp(sg.RZ_CYCLE[:2])
        stepped = pt.level_floors(engine, 'matter', sg.K, true, sg.rz_spectra_stepped(engine), x)
        print('spectra of %-24s level %5.1f FLOOR (cap %g), %5.1f at the stepped k; tilted rows of a pair within a factor %.1f' % (engine, floors, pt.CAP_SPECTRUM, stepped, spread))
        assert floors < pt.CAP_SPECTRUM and spread <= 16.
    for i in range(0, sg.RZ_CYCLE.size, 2):
        assert abs(sg.RZ_CYCLE[i] - sg.RZ_CYCLE[i + 1]) <= 1


def test_functional_cases_are_below_the_cap():
    import background_truth as bt
    import power_truth as pt
    for engine, nq, nz, nk, ncosmo, nan, pk_out in sg.functional_cases():
        case = sg.functional_case(engine, nq, nz, nk, ncosmo, nan)
        level = float(case['level'].max() / sg.FLOOR)
        print('functional %-24s %d x %d, nk %4d, %3d cosmologies: level %5.1f FLOOR' % (engine, nq, nz, nk, ncosmo, level))
        assert level < sg.CAP
    for engine in pt.ENGINES:
        case = sg.normalise_case(engine, 5, True)
        for name in ('rsigma8', 'amplitude'):
            floors = bt.below_cap(case['norm_true'][name][:, None], case['norm_f64'][name][:, None])
            print('sigma8_normalise %-24s %-10s level %5.1f FLOOR' % (engine, name, floors))
            assert floors < sg.CAP
        d, t, f = pt.prepared(engine, 'matter', sg.K, case['norm_true']['pk_out'], case['norm_true']['pk_out'], case['norm_f64']['pk_out'], case['x'])
        floors = float(bt.pointwise_level(t, f).max() / sg.FLOOR)
        print('sigma8_normalise %-24s %-10s level %5.1f FLOOR (cap %g)' % (engine, 'pk_out', floors, pt.CAP_SPECTRUM))
        assert floors < pt.CAP_SPECTRUM


def test_real_tophat_tables_case_is_below_the_cap(basis):
    """The case of test_fused_real_tophat_tables with the oracle's TophatVariance tables (the device test takes the package's and asserts the cap itself)."""
    import power_truth as pt
    from oracle import fftlog as ofl
    plan = ofl.tophat_variance(sg.K)
    real = (sg.real_tables(plan.pre[0], plan.post[0], plan.u[0]), plan.y[0])
    # longdouble FFTs with the float64 u table against the tap truth with the exact one: they differ by the rounding of that table alone
    syn, base = sg.tables('generic'), sg.base_rows()
    exact = tt.truth(base, sg.N, sg.NPAD, syn.pre[0], syn.post[0], syn.taps[0])
    apart = float(np.abs(sg.fft_truth(syn, base) - exact).max() / np.abs(exact).max())
    print('longdouble FFTs with the float64 u table against the tap truth: %.3g of the largest sample' % apart)
    assert apart < 4 * sg.FLOOR
    for engine in pt.ENGINES:
        for form in ('band', 'prefiltered'):
            case = sg.rz_case(engine, form, 129, 3, 5, basis, seed=2, real=real)
            finite = np.isfinite(case['true'])
            ratio = float(((case['true'][finite] / case['scale'][finite])**2).min())
            print('real tables, %-24s %-12s level %5.1f FLOOR (%5.1f at the stepped k), variance at least %.3f of its scale'
                  % (engine, form, case['level_plain'].max() / sg.FLOOR, case['level'].max() / sg.FLOOR, ratio))
            assert case['level_plain'].max() < sg.CAP * sg.FLOOR and ratio >= 0.25
