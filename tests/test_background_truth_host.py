"""CPU: tests/background_truth.py, the restatement that tests/test_background_edges_gpu.py holds the background kernels to.

1. Its float64 form equals ``oracle.background`` for the cosmologies of DENSITY_PARAMS, NCDM_PARAMS and the batch corners of tests/test_corners_gpu.py,
   evaluated on the oracle's knots.
   Bit for bit (the same expressions on arrays): the physical constants; Omega_g, Omega_ur, Omega_de, K of ``derived``; the 119-knot distance table; every
   density of ``densities`` and E(z); the curvature map and the powers of 1 + z of the derived distances, from the oracle's radial distance; age; ``rs``
   in both forms.
   To rtol = 4e-15 (another operation order): what stands behind a spline -- the radial distance (a Thomas solve for the slopes here, scipy's banded
   solve there), time (in the reference's order, the spline of (T_last - T) / h / Gyr, to 4e-15 of the largest tabulated value within the spline's
   reach, 24 knots, of the redshift's interval: the function falls to exactly 0 at the last knot, and at the corners whose dark energy underflows it rings
   through 0 behind a jump, where a bound relative to the value itself has no meaning) --,
   the species' tables (the prefactors grouped as ncdm_momenta_kernel has them) and their interpolation, E(z), D_C and rs with massive species, the
   derived parameters (T^4 as (T T) (T T); with species the oracle raises scalars to the fourth power, numpy's other code path) and the growth ODE tables
   (the oracle's densities take a scalar redshift: numpy's scalar pow and its array pow differ in the last bit).
2. The library's three knot exports equal the oracle's knots to rtol = 1e-15 (they are host functions: no device is needed).
3. Every case of the device tests is below the cap of 32 floors.
4. The rule tells the truth from a neighbour: ``assert_pointwise`` / ``assert_blocks`` raise when the "device" is the float64 restatement of a nearby
   wrong operation.
   Limit of the rule: closing the backward elimination at k == NK - 2 with a non-zero ``inc_up`` changes no bit of any result -- the right-hand side of
   the last knot is ra inc_k + rb inc_up with rb[NK - 1] = 0 exactly (build_pivots) -- so neither this rule nor any other can see it; the test asserts
   the equality of the bits instead.  The last knot of the growth ODE's grid, eta0 + 200 step, IS 0. in float64 (the kernel's pin changes no bit), so the
   neighbour there is a grid of 200 knots."""
import numpy as np
import pytest

import background_truth as bt
from oracle import background as ob
from oracle.gen_golden import DENSITY_PARAMS, NCDM_PARAMS, corner_params

F8 = np.float64
RTOL = 4e-15
BATCH_CORNERS = ['lambda_exact', 'omega_k_closed', 'wa_overflow', 'w_overflow', 'fluid_near_lambda', 'omega_b_zero', 'omega_k_open', 'phantom', 'omega_cdm_zero',
                 'h_low', 't_cmb_cold', 'n_ur_zero', 'omega_k_minus_tiny', 'w_sum_below_third', 'm_ncdm_heavy']      # those of tests/test_corners_gpu.py
COSMOLOGIES = ([('density%d' % i, par) for i, par in enumerate(DENSITY_PARAMS)] + [('ncdm%d' % i, par) for i, par in enumerate(NCDM_PARAMS)] +
               [(name, par) for name, par in corner_params() if name in BATCH_CORNERS])
Z = np.concatenate([[0., 1e-3], np.linspace(0.05, 3., 10), [10., 100., 1100., 9999., np.nan, -0.1, 2e4]])


@pytest.fixture
def oracle_knots(monkeypatch):
    """The restatement on the oracle's knots (the library's differ from them in the last bit at a few places) while it is compared with the oracle."""
    theirs = dict(distance=ob.z_knots(), time=ob.time_knots(), ncdm=ob.ncdm_knots())
    monkeypatch.setattr(bt, 'knots', lambda which: theirs[which] if which in theirs else bt.library_knots(which))


def same(a, b):
    return np.array_equal(np.asarray(a, dtype='f8'), np.asarray(b, dtype='f8'), equal_nan=True)


def close(a, b, what, atol=0.):
    a, b = np.asarray(a, dtype='f8').ravel(), np.asarray(b, dtype='f8').ravel()
    assert a.shape == b.shape, what
    for special in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(special(a), special(b)), what
    finite = np.isfinite(b)
    np.testing.assert_allclose(a[finite], b[finite], rtol=RTOL, atol=atol, err_msg=what)


def inputs(par):
    """(the oracle's parameters, params (1, 8), second_is_omega_m, m_ncdm, T_ncdm_over_cmb) of a Cosmology parameter dict."""
    par = {k: v for k, v in par.items() if k in ('h', 'Omega_cdm', 'Omega_b', 'Omega_k', 'T_cmb', 'N_eff', 'N_ur', 'w0_fld', 'wa_fld', 'Omega_m', 'm_ncdm', 'T_ncdm_over_cmb')}
    m = list(np.atleast_1d(par.pop('m_ncdm', [])))
    t = par.pop('T_ncdm_over_cmb', None)
    t = [ob.TNCDM_OVER_CMB] * len(m) if t is None else list(np.atleast_1d(t))
    with np.errstate(all='ignore'):
        o = ob.derived_ncdm(m, T_ncdm_over_cmb=np.asarray(t, dtype='f8'), **par)
    second = par['Omega_m'] if 'Omega_m' in par else par.get('Omega_cdm', 0.25)
    params = np.array([[par.get('h', 0.7), second, par.get('Omega_b', 0.05), par.get('Omega_k', 0.), par.get('T_cmb', ob.TCMB), float(o['N_ur']),
                        par.get('w0_fld', -1.), par.get('wa_fld', 0.)]])
    if not m:      # (numpy raises a scalar and an array to the fourth power differently: the oracle on arrays, as the restatement)
        o = ob.derived(Omega_m=params[:, 1] if 'Omega_m' in par else None, **{k: params[:, i] for i, k in enumerate(bt.PARAMS) if not (k == 'Omega_cdm' and 'Omega_m' in par)})
        o = {k: v[0] for k, v in o.items()}
    return o, params, int('Omega_m' in par), m, t


def test_constants():
    from scipy import constants as sc
    assert (bt.C, bt.STEFAN_BOLTZMANN, bt.PARSEC, bt.GRAVITATIONAL, bt.PI, bt.ELECTRON_VOLT, bt.BOLTZMANN) == \
        (sc.c, sc.Stefan_Boltzmann, sc.parsec, sc.gravitational_constant, sc.pi, sc.electron_volt, sc.Boltzmann)
    assert (bt.RHO_CRIT_KG, bt.RHO_CRIT, bt.C_KMS, bt.GIGAYEAR_OVER_MEGAPARSEC) == \
        (ob.rho_crit_over_kgph_per_mph3, ob.rho_crit_over_Msunph_per_Mpcph3, ob.C_KMS, ob.GIGAYEAR_OVER_MEGAPARSEC)
    assert bt.T_UR_OVER_CMB == (4. / 11.)**(1. / 3.) and bt.MPC == ob.megaparsec_over_m and bt.MSUN == ob.msun_over_kg


def test_library_knots():
    np.testing.assert_allclose(bt.library_knots('distance'), ob.z_knots(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(bt.library_knots('time'), ob.time_knots(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(bt.library_knots('ncdm'), ob.ncdm_knots(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(bt.library_knots('growth'), (np.exp(-bt.growth_eta()) - 1.)[::-1], rtol=1e-15, atol=0)
    assert bt.library_knots('growth')[0] == 0. and bt.growth_eta()[-1] == 0. and -6. + 200 * ((0. - -6.) / 200) == 0.
    assert bt.reach(bt.library_knots('distance')) == 24      # the walk of 24 knots above the sample that bg_kernel's comment states


@pytest.mark.parametrize('name', [name for name, _ in COSMOLOGIES])
def test_float64_restatement_equals_oracle(oracle_knots, name):
    o, params, som, m, t = inputs(dict(COSMOLOGIES)[name])
    tab = None
    with np.errstate(all='ignore'):
        if m:
            tab = bt.ncdm_tables(params[:, 0], params[:, 4], np.array([m]), np.array([t]), *bt.laguerre(100), dtype=F8)
            zc, rho, pr = ob.ncdm_tables(o)
            close(tab[0, :, 0], rho, 'rho_ncdm table')
            close(tab[0, :, 2], pr, 'p_ncdm table')
        c = bt.cosmo(params, som, tab, dtype=F8)
        if m:
            for key in ('Omega_g', 'Omega_ur', 'K'):      # (the oracle raises scalars to the fourth power here, the restatement arrays)
                close(c[key], o[key], key)
            close(c['Omega_de'], o['Omega_de'], 'Omega_de')
            close(c['Omega_cdm'], o['Omega_cdm'], 'Omega_cdm')
            zin = np.where((Z >= 0) & (Z <= 9999), Z, 0.5)      # (ncdm_interp takes no NaN)
            for which, out in ((0, 'rho'), (1, 'p')):
                for s in range(len(m)):
                    close(bt.ncdm_eval(c, zin, which, s)[0], ob.ncdm_interp(o, zin, out)[s], 'ncdm_interp')
            close(bt.efunc(c, zin)[0], ob.efunc_ncdm(zin, o), 'efunc_ncdm')
            close(bt.distances(c, Z)['comoving_radial_distance'][0], ob.comoving_radial_distance_ncdm(Z, o), 'comoving_radial_distance_ncdm')
            for cosmomc in (False, True):
                close(bt.rs(c, np.array([1059.94]), cosmomc)[3][0, 0], ob.rs(1059.94, o, efunc_fn=lambda zz: ob.efunc_ncdm(zz, o), cosmomc=cosmomc), 'rs')
            return
        for key in ('Omega_g', 'Omega_ur', 'K', 'Omega_de'):
            assert same(c[key][0], o[key]), key
        zc, table = ob.distance_table(o)
        assert same(bt.scan_table(c, zc)[1][0], table), 'distance_table'
        got = bt.distances(c, Z)
        if not np.isfinite(table).all():      # (the dark-energy factor overflows; the oracle's spline refuses a table that is not finite)
            assert all(np.isnan(got[kind]).all() for kind in bt.DISTANCE_KINDS)
            return
        want = ob.distances(Z, o)
        close(got['comoving_radial_distance'][0], want['comoving_radial_distance'], 'comoving_radial_distance')
        for kind in bt.RADIAL_KINDS:      # the curvature map and the powers of 1 + z, from the oracle's own radial distance
            assert same(bt.from_radial(want['comoving_radial_distance'], Z, c['K'][0], kind, F8), want[kind]), kind
        zin = np.where(np.isnan(Z), 0.5, Z)
        d, want = bt.densities(c, zin), ob.densities(zin, o, T_cmb=params[0, 4], has_fld=True)
        for key in ('rho_g', 'rho_b', 'rho_ur', 'rho_cdm', 'rho_k', 'rho_de', 'rho_fld', 'rho_r', 'rho_m', 'rho_tot', 'rho_crit'):
            assert same(d[key][0], want[key]), key
        assert same(d['rho_Lambda'][0], ob.densities(zin, o, has_fld=False)['rho_Lambda']) and same(bt.efunc(c, zin)[0], ob.efunc(zin, o))
        for key in ('rho_g', 'rho_k', 'rho_m'):
            assert same(bt.elementwise(c, zin, (key, True))[0], want['Omega' + key[3:]]), key
        assert same(bt.elementwise(c, zin, 'T_cmb')[0], want['T_cmb'])
        # time in the reference's order; age
        tknots = ob.time_knots()
        ttab = bt.scan_table(c, tknots, time=True)[1][0]
        # (the oracle's spline refuses a table that is not finite; where the increments underflow to 0 -- w_overflow -- the spline is a ringing behind a
        # jump and nothing else, down to 1e-230: no scale to hold it to)
        if np.isfinite(ttab).all() and (np.diff(ttab) > 0).all():
            zt = np.concatenate([Z, tknots[::7], tknots[:-1] + np.diff(tknots) / 2])
            inside = (zt >= 0) & (zt <= tknots[-1])
            got, age = bt.time(c, zt, order='reference')
            want = ob.time(zt, o)
            assert np.isnan(got[0][~inside]).all() and np.isnan(want[~inside]).all()
            at_knots = np.abs(bt.time(c, tknots, order='reference')[0][0])      # the largest tabulated value within the spline's reach of z's interval
            j = np.clip(np.searchsorted(tknots, zt[inside], side='right') - 1, 0, tknots.size - 2)
            reach = bt.reach(tknots)
            scale = np.array([at_knots[max(k - reach, 0):k + reach + 2].max() for k in j])
            assert (np.abs(got[0][inside] - want[inside]) <= RTOL * scale).all(), 'time'
            assert same(age[0], ob.age(o)), 'age'
        for cosmomc in (False, True):
            for z in (10., 1059.94, 1089.8):
                assert same(bt.rs(c, np.array([z]), cosmomc)[3][0, 0], ob.rs(z, o, cosmomc=cosmomc)), ('rs', z, cosmomc)
        for mass, which in ((0, 'm'), (1, 'cb')):
            D, f = bt.growth_tables(c, mass)
            zg, Dw, fw = ob.growth_ode_tables(o, mass=which)
            close(D[0], Dw, 'growth_ode_tables D ' + which)
            close(f[0], fw, 'growth_ode_tables f ' + which)
        want = ob.derived(**{k: params[0, i] for i, k in enumerate(bt.PARAMS)})
        got = dict(zip(('h2', 'H0', 'Omega_g', 'T_ur', 'Omega_ur', 'Omega_r', 'Omega_m', 'Omega_de', 'K'), bt.derived_parameters(params, F8)[:, 0]))
        for key in ('Omega_g', 'Omega_ur', 'Omega_de', 'K'):
            close(got[key], want[key], 'derived ' + key)
        assert got['Omega_m'] == params[0, 1] + params[0, 2] or som


# ---- the cap --------------------------------------------------------------------------------------------------------------------------------------------

def both(fn, *args, **kwargs):
    return fn(*args, dtype=bt.LD, **kwargs), fn(*args, dtype=F8, **kwargs)


def check_cap(levels, what):
    print('%s: level at most %.3g FLOOR' % (what, levels))
    assert levels < bt.CAP, what


@pytest.mark.parametrize('nsp', [0, 2])
@pytest.mark.parametrize('mix', bt.MIXES)
def test_cap_distances(mix, nsp):
    for cfg in bt.distance_configs(mix, nsp):
        ld, f8 = both(bt.config_truth, cfg, bt.distances)
        check_cap(max(bt.below_cap(ld[k], f8[k]) for k in ld), 'distances %s %d %s' % (mix, nsp, cfg['z'].shape))


def test_cap_time_elementwise_rs():
    for nsp in (0, 1):
        for cfg in bt.time_configs(nsp):
            (tl, al), (t8, a8) = both(bt.config_truth, cfg, bt.time)
            check_cap(bt.below_cap(tl, t8, 'block', top=np.where(np.isnan(al), 1, al)), 'time')
            check_cap(bt.below_cap(al[:, None], a8[:, None]), 'age')
        for cfg in bt.rs_configs(nsp):
            for cosmomc in (False, True):
                (rl, el, tl, _), (r8, e8, t8, _) = both(bt.config_truth, cfg, bt.rs, cosmomc=cosmomc)
                check_cap(bt.below_cap(rl.reshape(-1, 1), r8.reshape(-1, 1)), 'rs')
                for err, thr in ((el, tl), (e8, t8)):      # every verdict a factor 10 from its threshold, in both restatements
                    ratio = np.asarray(err / thr, dtype='f8')[~np.isnan(np.asarray(err, dtype='f8'))]
                    assert ((ratio < 0.1) | (ratio > 10.)).all(), ratio
                if cfg['z_shared'] == 0:
                    assert np.isnan(rl[0, 1]) and np.isnan(rl[2, 0]) and not np.isnan(rl[0, 0])      # z = 0: the rule misses its 1e-7
    for nsp in (0, 3):
        cfg = bt.elementwise_config(nsp)
        for kind in bt.ELEMENTWISE_KINDS:
            for species in ((-1, 0, nsp - 1) if kind[0] in ('rho_ncdm', 'p_ncdm') and nsp else (-1,)):
                ld, f8 = both(bt.config_truth, cfg, bt.elementwise, kind=kind, species=species)
                check_cap(bt.below_cap(ld, f8), 'elementwise %s species %d' % (kind, species))


@pytest.mark.parametrize('nsp', [0, 2])
def test_cap_growth(nsp):
    for n in bt.GROWTH_COUNTS:
        for mass in (0, 1):
            ld, f8 = both(bt.growth_truth, bt.growth_config(n, nsp), mass)
            check_cap(bt.below_cap(ld.reshape(-1, bt.NK_GROWTH), f8.reshape(-1, bt.NK_GROWTH), 'block'), 'growth %d %d' % (n, mass))


def test_cap_ncdm_derived_radial():
    for shape in bt.NCDM_SHAPES:
        cfg = bt.ncdm_config(*shape)
        ld, f8 = both(bt.ncdm_truth, cfg)
        values = [t[..., 0::2, :].reshape(-1, bt.NK_NCDM) for t in (ld, f8)]
        check_cap(bt.below_cap(*values, 'block'), 'species tables, values against the largest entry')
        check_cap(bt.below_cap(*values), 'species tables, values pointwise')
        check_cap(bt.below_cap(*[bt.midpoint_values(t).reshape(-1, bt.NK_NCDM - 1) for t in (ld, f8)]), 'species tables, midpoints of the splines')
        second = [t[..., 1::2, :].reshape(-1, bt.NK_NCDM) for t in (ld, f8)]      # the module's docstring: no case of these is below the cap
        assert bt.below_cap(*second, 'block') > 1e6 * bt.CAP
        if cfg['nan_member'] is not None:      # the member with the NaN: its own tables (all of them, or those of its species 0) and no others
            nan = np.isnan(ld).any(axis=(2, 3))
            want = np.zeros(nan.shape, dtype='?')
            want[cfg['nan_member'], slice(None) if np.isnan(cfg['h']).any() else 0] = True
            assert np.array_equal(nan, want) and np.array_equal(np.isnan(ld), np.isnan(f8))
            assert np.isfinite(bt.ncdm_truth(bt.ncdm_without_nan(cfg), F8)).all()
    for n in bt.DERIVED_COUNTS:
        p = bt.derived_config(n)['p']
        check_cap(bt.below_cap(*[t.T for t in both(bt.derived_parameters, p)]), 'derived')
    for n in bt.RADIAL_COUNTS:
        chi, z = bt.radial_config(n)
        for K in bt.RADIAL_K:
            for kind in bt.RADIAL_KINDS:
                check_cap(bt.below_cap(*[t[None] for t in both(bt.from_radial, chi, z, K, kind)]), 'from_radial')


# ---- neighbours -----------------------------------------------------------------------------------------------------------------------------------------

def rejected(rule, dev, truth, f64, what, **kwargs):
    rule(f64, truth, f64, what + ', the restatement itself', **kwargs)
    with pytest.raises(AssertionError, match='of its allowance'):
        rule(dev, truth, f64, what, **kwargs)


def test_the_rule_rejects_the_neighbours_of_the_distances():
    cfg = bt.distance_configs('alternating', 0)[-1]
    z = cfg['z']
    cl, c8 = (bt.take(bt.cosmo(cfg['p'], dtype=dtype), slice(0, 2)) for dtype in (bt.LD, F8))
    truth, f64 = (bt.distances(c, z)['comoving_radial_distance'] for c in (cl, c8))
    P = bt.pivots(bt.knots('distance'))
    inc = bt.scan_table(c8, bt.knots('distance'))[0]
    for ic in range(2):      # a cosmological constant and a fluid
        rows = slice(ic, ic + 1)
        route = bt.kernel_spline(P, inc[ic], z)
        # the kernel's route (24 knots of reach) in float64 fits the rule, with and without the 1e-14 it documents
        bt.assert_pointwise(route[None], truth[rows], f64[rows], 'the truncated elimination in float64', extra=bt.DISTANCE_EXTRA)
        bt.assert_pointwise(route[None], truth[rows], f64[rows], 'the truncated elimination in float64, extra = 0')
        rejected(bt.assert_pointwise, bt.kernel_spline(P, inc[ic], z, reach=P['reach'] - 8)[None], truth[rows], f64[rows], 'reach - 8', extra=bt.DISTANCE_EXTRA)
        closed = bt.kernel_spline(P, inc[ic], z, inc_up_last=inc[ic][-1])
        assert closed.tobytes() == route.tobytes()      # the limit of the rule that the module's docstring states: rb[NK - 1] = 0
    assert P['rb'][-1] == 0.
    for what, kwargs in (('Simpson on a displaced midpoint', dict(mid_shift=1e6 * np.finfo('f8').eps, simpson=True)), ('not-a-knot', dict(bc='not-a-knot'))):
        rejected(bt.assert_pointwise, bt.distances(c8, z, **kwargs)['comoving_radial_distance'], truth, f64, what, extra=bt.DISTANCE_EXTRA)


def test_the_rule_rejects_the_other_neighbours():
    cfg = bt.rs_configs(1)[1]      # with a massive species the rule is 1e-10 from its limit at z = 10 (without, it has converged to the last bit)
    truth, f64 = (r[0].reshape(-1, 1) for r in both(bt.config_truth, cfg, bt.rs))
    rejected(bt.assert_pointwise, bt.config_truth(cfg, bt.rs, dtype=F8, divmax=14)[0].reshape(-1, 1), truth, f64, 'Romberg with divmax = 14')
    cfg = bt.growth_config(1, 0)
    truth, f64 = both(bt.growth_truth, cfg, 0)
    D, f = bt.growth_tables(bt.cosmo(cfg['p'], cfg['second_is_omega_m'], dtype=F8), 0, eta=np.linspace(-6., 0., 200))
    dev = f64.copy()
    dev[:, 0, 0], dev[:, 1, 0] = D[:, 0], f[:, 0]      # z = 0 is on both grids
    rejected(bt.assert_blocks, dev.reshape(-1, bt.NK_GROWTH), truth.reshape(-1, bt.NK_GROWTH), f64.reshape(-1, bt.NK_GROWTH), 'RK4 on 200 knots')
    cfg = bt.elementwise_config(3)
    for kind, mutation in (('rho_ncdm', dict(leave_out=1)), ('rho_m', dict(drop_pressure=True))):
        truth, f64 = both(bt.config_truth, cfg, bt.elementwise, kind=kind)
        rejected(bt.assert_pointwise, bt.config_truth(cfg, bt.elementwise, dtype=F8, kind=kind, **mutation), truth, f64, '%s with %s' % (kind, mutation))
