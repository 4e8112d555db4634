"""The oracle on the hand-placed corner cosmologies (zero baryons / cold dark matter, flat to rounding, strongly curved, a cosmological constant and a
fluid next to it, an overflowing dark-energy exponent, extreme neutrinos, h and T_cmb) against the reference's own outputs for them
(tests/golden/corners.npz, `python -m oracle.gen_golden corners`): analytic engines and background, NaN and Inf where the reference has them."""
import numpy as np
import pytest

from oracle import background as ob, power as op
from oracle.gen_golden import corner_params

ENGINES = ['eisenstein_hu', 'eisenstein_hu_nowiggle', 'bbks']
NAMES = [name for name, _ in corner_params()]
REFUSED = ['w_sum_above_third']     # w0 + wa > 1/3: the reference raises CosmologyInputError (recorded as the class name)


def assert_same(got, ref, rtol, msg=''):
    """Equal to rtol where the reference is finite; NaN, +Inf and -Inf at the same places as the reference."""
    got, ref = np.asarray(got, dtype='f8'), np.asarray(ref, dtype='f8')
    assert got.shape == ref.shape, msg
    for special in (np.isnan, np.isposinf, np.isneginf):
        np.testing.assert_array_equal(special(got), special(ref), err_msg='%s: positions of %s' % (msg, special.__name__))
    np.testing.assert_allclose(got, ref, rtol=rtol, equal_nan=True, err_msg=msg)


def oracle_params(g, name):
    par = {p: float(g['%s_par_%s' % (name, p)]) for p in ['h', 'Omega_cdm', 'Omega_b', 'Omega_k', 'T_cmb', 'N_ur', 'w0_fld', 'wa_fld']}
    m = g[name + '_par_m_ncdm']
    return ob.derived_ncdm(m, T_ncdm_over_cmb=g[name + '_par_T_ncdm_over_cmb'], **par)


def test_golden_holds_every_case(golden):
    g = golden('corners')
    assert len(NAMES) >= 25 and len(set(NAMES)) == len(NAMES)
    for name in REFUSED:
        assert str(g[name + '_error']) == 'CosmologyInputError'
        for eng in ENGINES + ['eisenstein_hu_nowiggle_variants']:
            assert str(g[name + '_' + eng + '_error']) == 'CosmologyInputError'
    for name in NAMES:
        if name in REFUSED:
            continue
        for eng in ENGINES:
            assert g[name + '_' + eng + '_pkz'].shape == (g['k'].size, g['z'].size), (name, eng)
        assert g[name + '_comoving_radial_distance'].shape == g['zb'].shape


@pytest.mark.parametrize('name', [name for name in NAMES if name not in REFUSED])
def test_background_of_corner_cosmologies(golden, name):
    g = golden('corners')
    p = oracle_params(g, name)
    zb = g['zb']
    with np.errstate(all='ignore'):
        assert_same(p['Omega_de'], g[name + '_par_Omega_de'], 1e-12, 'Omega_de')
        assert_same(ob.efunc_ncdm(zb, p), g[name + '_efunc'], 1e-12, 'efunc')
        assert_same(ob.comoving_radial_distance_ncdm(zb, p), g[name + '_comoving_radial_distance'], 1e-10, 'comoving_radial_distance')


@pytest.mark.parametrize('engine', ENGINES)
@pytest.mark.parametrize('name', [name for name in NAMES if name not in REFUSED])
def test_engines_on_corner_cosmologies(golden, name, engine):
    g = golden('corners')
    k, z = g['k'], g['z']
    p = oracle_params(g, name)
    prim = {q: float(g['%s_par_%s' % (name, q)]) for q in ['n_s', 'alpha_s', 'beta_s', 'k_pivot']}
    key = name + '_' + engine + '_'
    with np.errstate(all='ignore'):
        assert_same(op.growth_factor_ncdm(z, p), g[key + 'growth_factor'], 1e-11, 'growth_factor')
        assert_same(op.growth_rate_ncdm(z, p), g[key + 'growth_rate'], 1e-11, 'growth_rate')
        _, pk0 = op.pk_z0_ncdm(k, p, engine=engine, A_s=float(g[key + 'A_s']), rsigma8=float(g[key + 'rsigma8']), **prim)
        g2 = op.growth_factor_ncdm(z, p, znorm=0.)**2
        assert_same(pk0[:, None] * g2, g[key + 'pkz'], 1e-10, 'pkz')
        if engine != 'bbks':
            s = op.eh_scalars(p['h'], p['Omega_cdm'], p['Omega_b'], p['T_cmb'])
            assert_same(s['rs_drag'] * p['h'], g[key + 'rs_drag'], 1e-12, 'rs_drag')
            assert_same(s['z_drag'], g[key + 'z_drag'], 1e-12, 'z_drag')
