"""GPU parity at the corners of the parameter space (tests/golden/corners.npz, `python -m oracle.gen_golden corners`): zero baryons or cold dark
matter, flat to rounding, strongly curved, a cosmological constant and a fluid a few ulp from it, a dark-energy exponent that overflows at the top
knots, extreme neutrinos, h and T_cmb -- where the short math forms and the wave-level specialisations of the kernels change behaviour.

Two parts: every corner on its own through ``Cosmology`` against the reference's outputs (NaN and Inf at the same places), and the batch entries
(``background.distance``, ``power.analytic``) with corners at lane 0, at the wave boundary 63 / 64 and at the workgroup boundary 255 / 256: every
other member of the batch must come out bit for bit as in the same batch without the corners (bg_kernel's wave-uniform branches -- wave_fld,
wave_lambda, wave_safe -- and its counting sort promise the same arithmetic whatever wave a sample lands in), the corners as the oracle has them."""
import functools
import warnings

import numpy as np
import pytest

from oracle import background as ob, power as op
from oracle.gen_golden import corner_params, FUZZ_ENGINES

pytestmark = pytest.mark.gpu
NAMES = [name for name, _ in corner_params()]
PARAMS = dict(corner_params())
BACKGROUND = ['efunc', 'comoving_radial_distance', 'angular_diameter_distance', 'luminosity_distance', 'time', 'Omega_m', 'Omega_de', 'rho_ncdm_tot']


@pytest.fixture(scope='module')
def cp():
    import torch
    assert torch.cuda.is_available()
    import cosmoprimo_amd
    warnings.simplefilter('ignore')
    return cosmoprimo_amd


def assert_same(got, ref, rtol, msg=''):
    """Equal to rtol where the reference is finite; NaN, +Inf and -Inf at the same places as the reference."""
    got, ref = np.asarray(got, dtype='f8'), np.asarray(ref, dtype='f8')
    assert got.shape == ref.shape, '%s: shape %s, reference %s' % (msg, got.shape, ref.shape)
    for special in (np.isnan, np.isposinf, np.isneginf):
        np.testing.assert_array_equal(special(got), special(ref), err_msg='%s: positions of %s (got %r, reference %r)' % (msg, special.__name__, got, ref))
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=0, equal_nan=True, err_msg=msg)


def check(g, key, fn, rtol):
    """The package's ``fn()`` against the golden ``key``: the same values, or the same exception class where the reference raised."""
    ref = g[key]
    if ref.dtype.kind != 'f':
        with pytest.raises(Exception) as info:
            fn()
        assert type(info.value).__name__ == str(ref), key
        return
    with np.errstate(all='ignore'):
        assert_same(fn(), ref, rtol, key)


# ---- every corner on its own ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('engine', FUZZ_ENGINES)
@pytest.mark.parametrize('name', NAMES)
def test_engines_one_corner_at_a_time(cp, golden, name, engine):
    g = golden('corners')
    k, z = g['k'], g['z']
    key = name + '_' + engine + '_'
    if key + 'error' in g:
        with pytest.raises(Exception) as info:
            cp.Cosmology(engine=engine, **PARAMS[name]).get_fourier()
        assert type(info.value).__name__ == str(g[key + 'error'])
        return
    cosmo = cp.Cosmology(engine=engine, **PARAMS[name])
    fo, ba = cosmo.get_fourier(), cosmo.get_background()
    check(g, key + 'pkz', lambda: fo.pk_interpolator()(k, z), 1e-10)
    # (w_overflow through eisenstein_hu_nowiggle_variants: P(k, z = 0.8) is 0 as in the reference, and so is sigma8 -- until the fused kernel stored a row of zeros
    # as zeros, the rounding of its pair partner came back in it, 4.9e-9: DESIGN.md section 6, the fused FFTLog truth entry)
    check(g, key + 'sigma8_z', lambda: fo.sigma8_z(z), 1e-10)
    check(g, key + 'growth_factor', lambda: ba.growth_factor(z), 1e-10)
    check(g, key + 'growth_rate', lambda: ba.growth_rate(z), 1e-10)
    if engine != 'bbks':
        check(g, key + 'rs_drag', lambda: cosmo.get_thermodynamics().rs_drag, 1e-12)
        check(g, key + 'z_drag', lambda: cosmo.get_thermodynamics().z_drag, 1e-12)


@pytest.mark.parametrize('name', NAMES)
def test_background_one_corner_at_a_time(cp, golden, name):
    g = golden('corners')
    zb, zg = g['zb'], g['zg']
    if name + '_error' in g:        # the reference refuses the parameters
        check(g, name + '_error', lambda: cp.Cosmology(engine='eisenstein_hu', **PARAMS[name]).get_background(), 0)
        return
    cosmo = cp.Cosmology(engine='eisenstein_hu', **PARAMS[name])
    ba = cosmo.get_background()
    for q in BACKGROUND:
        if q == 'time':     # T_last - T(z): the cancellation at high z costs digits -- held to 1e-15 of the age (1e-9 relative at z = 9999)
            ref = g[name + '_time']
            with np.errstate(all='ignore'):
                got = ba.time(zb)
                np.testing.assert_array_equal(np.isnan(got), np.isnan(ref), err_msg='time')
                np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-15 * abs(float(g[name + '_age'])), equal_nan=True, err_msg='time')
            continue
        check(g, name + '_' + q, lambda: getattr(ba, q)(zb), 1e-10)
    check(g, name + '_age', lambda: ba.age, 1e-10)
    for q in ['Omega_m', 'Omega_de', 'N_ur']:
        check(g, name + '_par_' + q, lambda: cosmo[q], 1e-13)
    # the linear growth from its ODE (cp_growth_ode_tables)
    from cosmoprimo_amd.cosmology import DefaultBackground
    bd = DefaultBackground(cosmo.engine)
    check(g, name + '_growth_factor_ode', lambda: bd.growth_factor(zg), 1e-10)
    check(g, name + '_growth_factor_ode_cb', lambda: bd.growth_factor(zg, mass='cb'), 1e-10)
    check(g, name + '_growth_rate_ode', lambda: bd.growth_rate(zg), 1e-10)


@pytest.mark.parametrize('name', NAMES)
def test_filters_one_corner_at_a_time(cp, golden, name):
    g = golden('corners')
    if name + '_wallish2018' not in g:      # recorded where the reference's spectrum is finite
        assert name + '_error' in g or not np.isfinite(g[name + '_eisenstein_hu_pkz']).all()
        return
    fid = cp.Cosmology(engine='eisenstein_hu')
    cosmo = cp.Cosmology(engine='eisenstein_hu', **PARAMS[name])
    interp = cosmo.get_fourier().pk_interpolator().to_1d(z=0.)
    for filt in ['wallish2018', 'brieden2022']:
        check(g, name + '_' + filt, lambda: np.asarray(cp.PowerSpectrumBAOFilter(interp, engine=filt, cosmo=cosmo, cosmo_fid=fid).pknow)[::8], 1e-9)


# ---- corners inside batches ------------------------------------------------------------------------------------------------------------------------------

BG_NAMES = ['h', 'Omega_cdm', 'Omega_b', 'Omega_k', 'T_cmb', 'N_ur', 'w0_fld', 'wa_fld']
BG_DEFAULTS = dict(Omega_k=0., T_cmb=2.7255, N_ur=3.044, w0_fld=-1., wa_fld=0.)      # a corner's parameters it does not set (Cosmology's defaults)
SIZES = [1, 63, 64, 65, 257, 3072]
POSITIONS = [0, 63, 64, 255, 256]
# the corners a batch of the raw entries can hold (background parameters and, with massive neutrinos, one species)
BATCH_CORNERS = ['lambda_exact', 'omega_k_closed', 'wa_overflow', 'w_overflow', 'fluid_near_lambda', 'omega_b_zero', 'omega_k_open', 'phantom', 'omega_cdm_zero',
                 'h_low', 't_cmb_cold', 'n_ur_zero', 'omega_k_minus_tiny', 'w_sum_below_third', 'm_ncdm_heavy']
Z_SHARED = np.array([0., 0.02, 0.3, 1.2, 2.9, 10., 1100., 9999.])


def normal_cosmologies(n, kind, safe, seed):
    """n ordinary cosmologies: ``kind`` 'lambda' (w0 = -1, wa = 0), 'fluid' or 'mixed' (every other one a fluid); ``safe``: every density parameter
    >= 0, else one member (the sixth, or the only one) closed."""
    rng = np.random.default_rng(seed)
    p = dict(h=rng.uniform(0.6, 0.8, n), Omega_cdm=rng.uniform(0.2, 0.3, n), Omega_b=rng.uniform(0.04, 0.06, n), Omega_k=rng.uniform(0., 0.05, n),
             T_cmb=rng.uniform(2.6, 2.8, n), N_ur=rng.uniform(2., 3.5, n), w0_fld=rng.uniform(-1.2, -0.8, n), wa_fld=rng.uniform(-0.3, 0.3, n))
    m = rng.uniform(0.05, 0.15, n)
    lam = np.ones(n, dtype=bool) if kind == 'lambda' else (np.zeros(n, dtype=bool) if kind == 'fluid' else np.arange(n) % 2 == 0)
    p['w0_fld'][lam], p['wa_fld'][lam] = -1., 0.
    if not safe:
        p['Omega_k'][min(5, n - 1)] = -0.05
    return p, m


def with_corners(p, m, positions, names):
    p, m = {q: v.copy() for q, v in p.items()}, m.copy()
    for pos, name in zip(positions, names):
        c = PARAMS[name]
        for q in BG_NAMES:
            p[q][pos] = c[q] if q in c else BG_DEFAULTS[q]
        if 'm_ncdm' in c:
            m[pos] = c['m_ncdm'][0]
    return p, m


def corner_placement(n, shift, ncdm):
    names = [name for name in BATCH_CORNERS if ncdm or 'm_ncdm' not in PARAMS[name]]
    positions = [pos for pos in POSITIONS if pos < n]
    return positions, [names[(j + shift) % len(names)] for j in range(len(positions))]


def z_rows(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0., 3., (n, 6))
    z[:, 0], z[::7, 1], z[::11, 2] = 0., 9999., 150.
    return z


@functools.lru_cache(maxsize=None)
def oracle_distance(kind, bg, m, z):
    p = ob.derived_ncdm(list(m), T_ncdm_over_cmb=[ob.TNCDM_OVER_CMB] * len(m), **dict(bg))
    with np.errstate(all='ignore'):
        e = ob.efunc_ncdm(np.array(z), p)
        return e if kind == 'efunc' else ob.comoving_radial_distance_ncdm(np.array(z), p)


def run_distance(cp, kind, p, m, z, per_cosmology_z, ncdm):
    import torch
    from cosmoprimo_amd import background as bgm
    n = p['h'].size
    tables = bgm.NcdmTables([m], [np.full(n, ob.TNCDM_OVER_CMB)], h=p['h'], T_cmb=p['T_cmb'], ncosmo=n) if ncdm else None
    return bgm.distance(kind, torch.as_tensor(z, device='cuda'), params=p, per_cosmology_z=per_cosmology_z, ncdm=tables)


@pytest.mark.parametrize('ncdm', [False, True], ids=['massless', 'ncdm'])
@pytest.mark.parametrize('safe', [True, False], ids=['safe', 'closed'])
@pytest.mark.parametrize('kind', ['lambda', 'fluid', 'mixed'])
def test_background_batches_keep_their_neighbours(cp, kind, safe, ncdm):
    import torch
    for n in SIZES:
        seed = n + 1000 * (kind == 'fluid') + 2000 * (kind == 'mixed') + 4000 * safe + 8000 * ncdm
        p, m = normal_cosmologies(n, kind, safe, seed)
        zr = z_rows(n, seed)
        for shift in range(0, len(BATCH_CORNERS), 3 if n < 3000 else 7):
            positions, names = corner_placement(n, shift, ncdm)
            pc, mc = with_corners(p, m, positions, names)
            others = np.ones(n, dtype=bool)
            others[positions] = False
            for per_cosmology_z, z in ((True, zr), (False, Z_SHARED)):
                for what in ['comoving_radial_distance', 'efunc']:
                    got = run_distance(cp, what, pc, mc, z, per_cosmology_z, ncdm)
                    ref = run_distance(cp, what, p, m, z, per_cosmology_z, ncdm)
                    msg = '%s n=%d corners %s at %s, per_cosmology_z=%s' % (what, n, names, positions, per_cosmology_z)
                    assert torch.equal(got[torch.as_tensor(others, device=got.device)], ref[torch.as_tensor(others, device=ref.device)]), msg
                    for pos, name in zip(positions, names):
                        bg = tuple((q, float(pc[q][pos])) for q in BG_NAMES)
                        zz = tuple(z[pos] if per_cosmology_z else z)
                        expect = oracle_distance(what, bg, (float(mc[pos]),) if ncdm else (), zz)
                        assert_same(got[pos].cpu().numpy(), expect, 1e-10, '%s: corner %s at %d' % (msg, name, pos))


PK_CORNERS = ['omega_b_zero', 'omega_cdm_zero', 'h_low', 'h_high', 't_cmb_cold', 'omega_b_large', 'omega_k_closed', 'wa_overflow', 'omega_b_tiny']


@pytest.mark.parametrize('engine', ['eisenstein_hu', 'eisenstein_hu_nowiggle', 'bbks'])
def test_power_batches_keep_their_neighbours(cp, engine):
    """power.analytic (cp_power_eval: workgroups of four cosmologies for small batches, one wave per cosmology from 3072 on) with corners at lane 0
    and at the wave and workgroup boundaries: the other members bit for bit as without the corners, the corners as the oracle has them."""
    import torch
    from cosmoprimo_amd import power as pw
    k = np.geomspace(1e-4, 10., 70)
    z = np.array([0., 0.8, 2.5])
    for n in SIZES:
        p, _ = normal_cosmologies(n, 'mixed', True, n + 77)
        rng = np.random.default_rng(n)
        pk = dict(A_s=rng.uniform(1.5e-9, 2.5e-9, n), n_s=rng.uniform(0.9, 1., n))
        for shift in range(0, len(PK_CORNERS), 2):
            positions = [pos for pos in POSITIONS if pos < n]
            names = [PK_CORNERS[(j + shift) % len(PK_CORNERS)] for j in range(len(positions))]
            pc, _ = with_corners(p, np.zeros(n), positions, names)
            others = torch.ones(n, dtype=torch.bool, device='cuda')
            others[positions] = False
            with np.errstate(all='ignore'):
                got = pw.analytic(engine, 'matter', k, z=z, bg=pc, pk=pk)
                ref = pw.analytic(engine, 'matter', k, z=z, bg=p, pk=pk)
            msg = '%s n=%d corners %s at %s' % (engine, n, names, positions)
            assert torch.equal(got[others], ref[others]), msg
            for pos, name in zip(positions, names):
                par = {q: float(pc[q][pos]) for q in BG_NAMES}
                o = ob.derived_ncdm([], T_ncdm_over_cmb=[], **par)
                with np.errstate(all='ignore'):
                    _, pk0 = op.pk_z0_ncdm(k, o, engine=engine, A_s=float(pk['A_s'][pos]), n_s=float(pk['n_s'][pos]))
                    expect = (pk0[:, None] * op.growth_factor_ncdm(z, o, znorm=0.)**2).T
                assert_same(got[pos].cpu().numpy(), expect, 1e-10, '%s: corner %s at %d' % (msg, name, pos))
