"""Restatement of the analytic power-spectrum kernels (csrc/cp_power.hip, csrc/cp_power_eval.h) for tests/test_power_truth_host.py and
tests/test_power_truth_gpu.py: every operation in numpy, in any floating-point type.  ``np.longdouble`` is the truth, float64 the reference
implementation that is not the code under test.  numpy only.

Operation order: that of the reference as oracle/power.py cites it (file:line there) -- ``eh_scalars`` with ``alpha_gamma``, ``bbks_gamma``,
``transfer_eh``, ``transfer_nowiggle``, ``transfer_bbks``, ``primordial_pk``, ``pk_callable``, log(k P), ``variants_scalars`` and
``variants_transfer_kz`` with the matter spectrum of its ``pk_callable`` -- with a ``dtype``.  The literal constants of the fits, ``np.e``, ``np.pi`` and
the physical constants are float64 values, exact inputs of the truth.  The cosmology (``Omega_cdm`` from ``Omega_m``, the species' tables), the CPT92
growth factor and the species' densities of today come from tests/background_truth.py (``cosmo``, ``elementwise(c, z, 'growth_cpt')``), which
tests/test_background_edges_gpu.py pins; ``kscale`` is applied as the kernel applies it, ``k * kscale[ic]`` in the restatement's own type.

Tolerance rule (tests/jacobian_reference.py, tests/background_truth.py): ``level`` is the float64 restatement's distance from
the longdouble truth, floored at FLOOR = 1.1e-16; the device must lie within ALLOW = 16 levels + ``extra`` of the truth, entry by entry, relative to
the entry (``background_truth.assert_pointwise``).  A row is one (cosmology, decade of k) block of a quantity with all its redshifts, so that a loose
decade does not loosen the others; a scalar of a cosmology is a row of its own.  Adaptations, each a scale the entry is held against in place of
|truth| (:func:`against`):
  log_k_matter   crosses zero: max(1, |truth|), the rule of tests/test_math_gpu.py for log_tab.
  BBKS           takes log(1 + x) / x with x = 2.34 q as the reference codes it: one float64 rounding of 1 + x costs 2^-53 / x of the result in any
                 float64 arithmetic.  The entry's scale is w |truth| with w = 1 + p / x, p = 1 for the transfer function and 2 for the spectra (log(k P):
                 w max(1, |truth|)).  Unweighted the restatement is thousands of floors from the truth below k = 1e-4 h/Mpc
                 (tests/test_power_truth_host.py measures both).
  alpha_b        (cp_eh_scalars) is y G(y) with G = -6 sqrt(1 + y) + (2 + 3 y) log(...): at y_drag of 2 to 3 the two terms are 140 to 850 times their sum, and
                 each carries a float64 rounding.  Scale: w |truth| with w = (|6 sqrt(1 + y)| + |(2 + 3 y) log(...)|) / |G|, the condition of that sum.
  frac_ncdm      (cp_variants_scalars) is 1 - frac_cb: it carries the absolute rounding of frac_cb ~ 1, and without species it is that rounding and
                 nothing else.  Scale: 1.
``extra`` is what the headers state and nothing else: EXTRA_EH = 1e-14 (the comment over ``transfer_eh`` in cp_power_eval.h: "within 1e-14 of the
operation-for-operation form"), EXTRA_NOWIGGLE = 1e-15 (the comment over ``pow_short``: "1e-15 at most over the powers of the fits"; the no-wiggle
constants reach rs_drag through it), zero for BBKS and the primordial spectrum, twice the transfer function's for ``matter`` and ``log_k_matter``
(P ~ T^2), zero for ``cp_eh_scalars``, ``cp_variants_scalars`` and ``cp_power_eval_variants`` (the library's pow, log and exp).
Caps (conditions on the cases, not tolerances): a block is used on the device only while the level of its restatement is below CAP = 32 floors
(transfer functions, primordial spectra, scalars: ``background_truth.CAP``) or CAP_SPECTRUM = 64 floors (``matter``, ``log_k_matter``: P ~ T^2 doubles
the transfer function's relative error).  tests/test_power_truth_host.py holds every block of every case to them; no case drops a block.  One draw was changed for its cap: the pre-kernel
batches were first drawn with the seeds 1001, 1063, 1064, 1065, and one cosmology of the 63 had an EH98 transfer function at 36.8 floors (72.3 for
its spectrum) in the decade of k = 10 h/Mpc; they are drawn with 1301 to 1365 now (at most 26.6 and 53.7).

``p_c`` and ``p_cb`` of cp_variants_scalars are (5 - sqrt(1 + 24 frac)) / 4 with the root between 4.4 and 5: like ``frac_ncdm`` they are held against
their minuend, 5 / 4, not against themselves (p_cb is 0 to rounding without species).
"""
import functools

import numpy as np

import background_truth as bt
from background_truth import LD, FLOOR, ALLOW, CAP, assert_pointwise

CAP_SPECTRUM = 64.
EXTRA_EH = 1e-14            # cp_power_eval.h, over transfer_eh: "within 1e-14 of the operation-for-operation form"
EXTRA_NOWIGGLE = 1e-15      # cp_power_eval.h, over pow_short: "1e-15 at most over the powers of the fits"
ENGINES = ('eisenstein_hu', 'eisenstein_hu_nowiggle', 'bbks')
WHATS = ('transfer', 'primordial', 'matter', 'log_k_matter')
EXTRA = {'eisenstein_hu': EXTRA_EH, 'eisenstein_hu_nowiggle': EXTRA_NOWIGGLE, 'bbks': 0., 'variants': 0.}
EH_SCALARS = ('rs_drag', 'z_drag', 'z_eq', 'k_eq', 'r_drag', 'r_eq', 'k_silk', 'alpha_c', 'beta_c', 'alpha_b', 'beta_node', 'beta_b', 'alpha_gamma',
              'gamma')      # enum cp_eh_scalar ('gamma': bbks_gamma)
VARIANTS_SCALARS = ('omega_b', 'omega_m', 'frac_b', 'frac_cdm', 'frac_cb', 'frac_ncdm', 'theta_cmb', 'z_eq', 'k_eq', 'z_drag', 'rs_drag', 'p_c', 'p_cb',
                    'gamma_ncdm', 'beta_c')      # enum cp_variants_scalar
PK_PARAMS = ('A_s', 'n_s', 'alpha_s', 'beta_s', 'k_pivot')      # enum cp_pk_param


def _col(v):
    return v[..., None] if np.ndim(v) else v


def extra_of(engine, what):
    return {'transfer': 1., 'primordial': 0., 'matter': 2., 'log_k_matter': 2.}[what] * EXTRA[engine]


def cap_of(what):
    return CAP_SPECTRUM if what in ('matter', 'log_k_matter') else CAP


# ---- the fits ------------------------------------------------------------------------------------------------------------------------------------------

def eh_scalars(h, Omega_cdm, Omega_b, T_cmb, dtype=LD, parts=False):
    """oracle.power.eh_scalars (eisenstein_hu.py:34-92, eisenstein_hu_nowiggle.py:21) in ``dtype``: dict of arrays shaped like the parameters.
    ``parts``: with 'alpha_b_weight', the condition of the sum inside alpha_b_G."""
    dtype = np.dtype(dtype).type
    h, Omega_cdm, Omega_b, T_cmb = (np.asarray(v).astype(dtype) for v in (h, Omega_cdm, Omega_b, T_cmb))
    s = {}
    omega_b = s['omega_b'] = Omega_b * h**2
    omega_m = s['omega_m'] = Omega_cdm * h**2 + Omega_b * h**2
    frac_b = s['frac_b'] = omega_b / omega_m
    theta_cmb = s['theta_cmb'] = T_cmb / 2.7
    z_eq = s['z_eq'] = 2.5e4 * omega_m * theta_cmb ** (-4) - 1.
    k_eq = s['k_eq'] = 0.0746 * omega_m * theta_cmb ** (-2)
    z_drag_b1 = 0.313 * omega_m ** (-0.419) * (1 + 0.607 * omega_m ** 0.674)
    z_drag_b2 = 0.238 * omega_m ** 0.223
    z_drag = s['z_drag'] = 1345 * omega_m ** 0.251 / (1. + 0.659 * omega_m ** 0.828) * (1. + z_drag_b1 * omega_b ** z_drag_b2)
    r_drag = s['r_drag'] = 31.5 * omega_b * theta_cmb ** (-4) * (1000. / (1 + z_drag))
    r_eq = s['r_eq'] = 31.5 * omega_b * theta_cmb ** (-4) * (1000. / (1 + z_eq))
    s['rs_drag'] = 2. / (3. * k_eq) * np.sqrt(6. / r_eq) * np.log((np.sqrt(1 + r_drag) + np.sqrt(r_drag + r_eq)) / (1 + np.sqrt(r_eq)))
    s['k_silk'] = 1.6 * omega_b ** 0.52 * omega_m ** 0.73 * (1 + (10.4 * omega_m) ** (-0.95))
    a1 = (46.9 * omega_m) ** 0.670 * (1 + (32.1 * omega_m) ** (-0.532))
    a2 = (12.0 * omega_m) ** 0.424 * (1 + (45.0 * omega_m) ** (-0.582))
    s['alpha_c'] = a1 ** (-frac_b) * a2 ** (-frac_b**3)
    b1 = 0.944 / (1 + (458 * omega_m) ** (-0.708))
    b2 = 0.395 * omega_m ** (-0.0266)
    s['beta_c'] = 1. / (1 + b1 * ((1 - frac_b) ** b2) - 1)
    y_drag = (1 + z_eq) / (1 + z_drag)
    first, second = -6. * np.sqrt(1 + y_drag), (2. + 3. * y_drag) * np.log((np.sqrt(1 + y_drag) + 1) / (np.sqrt(1 + y_drag) - 1))
    alpha_b_G = y_drag * (first + second)
    s['alpha_b'] = 2.07 * k_eq * s['rs_drag'] * (1 + r_drag)**(-0.75) * alpha_b_G
    s['beta_node'] = 8.41 * omega_m ** 0.435
    s['beta_b'] = 0.5 + frac_b + (3. - 2. * frac_b) * np.sqrt((17.2 * omega_m) ** 2 + 1)
    s['alpha_gamma'] = 1. - 0.328 * np.log(431. * omega_m) * frac_b + 0.38 * np.log(22.3 * omega_m) * frac_b**2
    if parts:
        s['alpha_b_weight'] = (np.abs(first) + np.abs(second)) / np.abs(first + second)
    return s


def transfer_eh(k, h, s, dtype=LD, mutation=None):
    """oracle.power.transfer_eh (eisenstein_hu.py:241-283): k (nk,) or (n, nk) in h/Mpc, h and the scalars (n,) -> (n, nk)."""
    dtype = np.dtype(dtype).type
    g = {n: _col(np.asarray(v).astype(dtype)) for n, v in s.items()}
    k = np.asarray(k).astype(dtype) * _col(np.asarray(h).astype(dtype))
    q = k / (13.41 * g['k_eq'])
    ks = k * g['rs_drag']
    ln_beta = np.log(np.e + 1.8 * (1. if mutation == 'no_beta_c' else g['beta_c']) * q)
    ln_nobeta = np.log(np.e + 1.8 * q)
    p108 = 1.0800001 if mutation == 'q108' else 1.08
    C_alpha = 14.2 / g['alpha_c'] + 386. / (1 + 69.9 * q ** p108)
    C_noalpha = 14.2 + 386. / (1 + 69.9 * q ** p108)
    T_c_f = 1. / (1. + (ks / 5.4) ** 4)

    def T0(a, b):
        return a / (a + b * q**2)

    if mutation == 'weight_swapped':
        T_c = (1 - T_c_f) * T0(ln_beta, C_noalpha) + T_c_f * T0(ln_beta, C_alpha)
    else:
        T_c = T_c_f * T0(ln_beta, C_noalpha) + (1 - T_c_f) * T0(ln_beta, C_alpha)
    s_tilde = g['rs_drag'] * (1 + (g['beta_node'] / ks)**3) ** (-1. / 3.)
    ks_tilde = k * s_tilde
    T_b_T0 = T0(ln_nobeta, C_noalpha)
    T_b_1 = T_b_T0 / (1 + (ks / 5.2)**2)
    T_b_2 = g['alpha_b'] / (1 + (g['beta_b'] / ks)**3) * np.exp(-(k / g['k_silk']) ** 1.4)
    T_b = sinc(ks_tilde if mutation == 'sinc_without_pi' else ks_tilde / np.pi) * (T_b_1 + T_b_2)
    return g['frac_b'] * T_b + (1 - g['frac_b']) * T_c


def sinc(x):
    """numpy.sinc in the type of x: sin(pi x) / (pi x), 1 at 0 (numpy's own takes pi y with y = where(x == 0, 1e-20, x))."""
    y = np.pi * np.where(x == 0, 1.0e-20, x)
    return np.sin(y) / y


def transfer_nowiggle(k, h, s, dtype=LD):
    """oracle.power.transfer_nowiggle (eisenstein_hu_nowiggle.py:45-51)."""
    dtype = np.dtype(dtype).type
    g = {n: _col(np.asarray(v).astype(dtype)) for n, v in s.items()}
    k = np.asarray(k).astype(dtype) * _col(np.asarray(h).astype(dtype))
    ks = k * g['rs_drag']
    gamma_eff = g['omega_m'] * (g['alpha_gamma'] + (1 - g['alpha_gamma']) / (1 + (0.43 * ks) ** 4))
    q = k * g['theta_cmb']**2 / gamma_eff
    L0 = np.log(2 * np.e + 1.8 * q)
    C0 = 14.2 + 731.0 / (1 + 62.5 * q)
    return L0 / (L0 + C0 * q**2)


def bbks_gamma(h, Omega_cdm, Omega_b, Omega_nu_m=0., dtype=LD):
    """oracle.power.bbks_gamma (bbks.py:34-38)."""
    dtype = np.dtype(dtype).type
    h, Omega_cdm, Omega_b, Omega_nu_m = (np.asarray(v).astype(dtype) for v in (h, Omega_cdm, Omega_b, Omega_nu_m))
    Omega_m = Omega_b + Omega_cdm + Omega_nu_m
    return Omega_m * h**2 * np.exp(-Omega_b * (1. + np.sqrt(2. * h) / Omega_m))


def bbks_x(k, h, gamma, dtype=LD):
    """x = 2.34 q of transfer_bbks: what the weight of the BBKS rule is made of."""
    dtype = np.dtype(dtype).type
    q = np.asarray(k).astype(dtype) * _col(np.asarray(h).astype(dtype)) / _col(np.asarray(gamma).astype(dtype))
    return 2.34 * q


def transfer_bbks(k, h, gamma, dtype=LD):
    """oracle.power.transfer_bbks (bbks.py:62-64, as coded)."""
    dtype = np.dtype(dtype).type
    q = np.asarray(k).astype(dtype) * _col(np.asarray(h).astype(dtype)) / _col(np.asarray(gamma).astype(dtype))
    x = 2.34 * q
    return np.log(1 + x) / x * (1. + 3.89 * q * (16.2 * q)**2 + (5.47 * q)**3 + (6.71 * q)**4)**(-0.25)


def primordial_pk(k, h, A_s, n_s, alpha_s, beta_s, k_pivot, dtype=LD, mutation=None):
    """oracle.power.primordial_pk (eisenstein_hu.py:189-215); k in h/Mpc, k_pivot in 1/Mpc."""
    dtype = np.dtype(dtype).type
    h, A_s, n_s, alpha_s, beta_s = (_col(np.asarray(v).astype(dtype)) for v in (h, A_s, n_s, alpha_s, beta_s))
    kp = _col(np.asarray(k_pivot).astype(dtype)) / h
    k = np.asarray(k).astype(dtype)
    lnkkp = np.log(k / kp)
    half = 1. if mutation == 'alpha_s_whole' else 1. / 2.
    return h**3 * A_s * (k / kp) ** (n_s - 1. + half * alpha_s * lnkkp + 1. / 6. * beta_s * lnkkp**2)


def pk_callable(k, transfer, Omega_m, h, pk_prim, dtype=LD):
    """oracle.power.pk_callable (eisenstein_hu.py:321-324)."""
    dtype = np.dtype(dtype).type
    k = np.asarray(k).astype(dtype)
    potential_to_density = (3. * _col(np.asarray(Omega_m).astype(dtype)) * 100**2 / (2. * bt.C_KMS**2 * k**2)) ** (-2)
    curvature_to_potential = 9. / 25. * 2. * np.pi**2 / k**3 / _col(np.asarray(h).astype(dtype)) ** 3
    return transfer ** 2 * potential_to_density * curvature_to_potential * pk_prim


def omega_nu_m(c):
    """(Omega_ncdm (n, nsp), Omega_pncdm (n, nsp)) of today from the first knot of the species' tables of ``background_truth.cosmo`` (cosmology.py:371-376,
    oracle.background.derived_ncdm: rho0 / rho_crit, 3 p0 / rho_crit); (n, 0) without species."""
    if c['tab'] is None:
        empty = np.zeros((c['n'], 0), dtype=c['dtype'])
        return empty, empty
    return c['tab'][:, :, 0, 0] / bt.RHO_CRIT, 3. * c['tab'][:, :, 2, 0] / bt.RHO_CRIT


def sum_species(v):
    """The species summed in their order (load_cosmo, variants_scalars)."""
    tot = np.zeros(v.shape[0], dtype=v.dtype)
    for s in range(v.shape[1]):
        tot = tot + v[:, s]
    return tot


def analytic(engine, what, c, pk, k, z=None, kscale=None, mutation=None):
    """cp_power_eval of the cosmologies ``c`` (``background_truth.cosmo``) with primordial parameters pk (n, 5) float64 at the shared wavenumbers k (nk,)
    float64, cosmology i at k * kscale[i]: (n, nk), or (n, nz, nk) for 'matter' at the redshifts z (nz,).  In the type of c."""
    dtype = c['dtype']
    n = c['n']
    kk = np.broadcast_to(np.asarray(k, dtype='f8').astype(dtype), (n, np.size(k)))
    if kscale is not None:
        kk = kk * np.asarray(kscale, dtype='f8').astype(dtype)[:, None]
    pk = np.asarray(pk, dtype='f8').reshape(n, len(PK_PARAMS)).astype(dtype)
    Opn, Oppn = omega_nu_m(c)
    nu_m = np.zeros(n, dtype=dtype) if mutation == 'no_nu_m' else sum_species(Opn) - sum_species(Oppn)
    with np.errstate(all='ignore'):
        prim = primordial_pk(kk, c['h'], *(pk[:, i] for i in range(5)), dtype=dtype, mutation=mutation)
        if what == 'primordial':
            return prim
        if engine == 'bbks':
            T = transfer_bbks(kk, c['h'], bbks_gamma(c['h'], c['Omega_cdm'], c['Omega_b'], nu_m, dtype), dtype)
        else:
            s = eh_scalars(c['h'], c['Omega_cdm'], c['Omega_b'], c['T_cmb'], dtype)
            T = transfer_eh(kk, c['h'], s, dtype, mutation) if engine == 'eisenstein_hu' else transfer_nowiggle(kk, c['h'], s, dtype)
        if what == 'transfer':
            return T
        P = pk_callable(kk, T, c['Omega_b'] + c['Omega_cdm'] + nu_m, c['h'], prim, dtype)
        if what == 'log_k_matter':
            return np.log(kk * P)
        if z is None:
            return P
        g = bt.elementwise(c, np.asarray(z, dtype='f8'), 'growth_cpt')      # growth_factor(z, znorm=0), eisenstein_hu.py:317
        return P[:, None, :] * (g**2)[:, :, None]


def analytic_x(c, k, kscale=None):
    """x = 2.34 q of the BBKS form at the wavenumbers of :func:`analytic`, (n, nk)."""
    dtype = c['dtype']
    kk = np.broadcast_to(np.asarray(k, dtype='f8').astype(dtype), (c['n'], np.size(k)))
    if kscale is not None:
        kk = kk * np.asarray(kscale, dtype='f8').astype(dtype)[:, None]
    Opn, Oppn = omega_nu_m(c)
    return bbks_x(kk, c['h'], bbks_gamma(c['h'], c['Omega_cdm'], c['Omega_b'], sum_species(Opn) - sum_species(Oppn), dtype), dtype)


def scalars_of(c, parts=False):
    """cp_eh_scalars: dict name of EH_SCALARS -> (n,)."""
    s = eh_scalars(c['h'], c['Omega_cdm'], c['Omega_b'], c['T_cmb'], c['dtype'], parts=parts)
    Opn, Oppn = omega_nu_m(c)
    s['gamma'] = bbks_gamma(c['h'], c['Omega_cdm'], c['Omega_b'], sum_species(Opn) - sum_species(Oppn), c['dtype'])
    return s


# ---- eisenstein_hu_nowiggle_variants ---------------------------------------------------------------------------------------------------------------------

def variants_scalars(h, Omega_cdm, Omega_b, T_cmb, Omega_ncdm, Omega_pncdm, dtype=LD):
    """oracle.power.variants_scalars (eisenstein_hu_nowiggle_variants.py:32-76): the parameters (n,), Omega_ncdm and Omega_pncdm (n, nsp)."""
    dtype = np.dtype(dtype).type
    h, Omega_cdm, Omega_b, T_cmb = (np.asarray(v).astype(dtype) for v in (h, Omega_cdm, Omega_b, T_cmb))
    Omega_ncdm, Omega_pncdm = (np.asarray(v).astype(dtype) for v in (Omega_ncdm, Omega_pncdm))
    h2 = h**2
    s = {}
    s['omega_b'] = Omega_b * h2
    N = Omega_ncdm.shape[-1]
    ncdm = (sum_species(Omega_ncdm) - sum_species(Omega_pncdm)) if N else 0.
    s['omega_m'] = Omega_cdm * h2 + Omega_b * h2 + ncdm * h2
    s['frac_b'] = s['omega_b'] / s['omega_m']
    s['frac_cdm'] = Omega_cdm * h2 / s['omega_m']
    s['frac_cb'] = s['frac_cdm'] + s['frac_b']
    s['frac_ncdm'] = 1. - s['frac_cb']
    s['N_ncdm'] = N
    s['theta_cmb'] = T_cmb / 2.7
    om, ob_ = s['omega_m'], s['omega_b']
    s['z_eq'] = 2.5e4 * om * s['theta_cmb'] ** (-4) - 1.
    s['k_eq'] = 0.0746 * om * s['theta_cmb'] ** (-2)
    b1 = 0.313 * om ** (-0.419) * (1 + 0.607 * om ** 0.674)
    b2 = 0.238 * om ** 0.223
    s['z_drag'] = 1291 * om ** 0.251 / (1. + 0.659 * om ** 0.828) * (1. + b1 * ob_ ** b2)
    s['rs_drag'] = 44.5 * np.log(9.83 / om) / np.sqrt(1. + 10. * ob_ ** 0.75)
    fbn = s['frac_b'] + s['frac_ncdm']
    s['p_c'] = (5. - np.sqrt(1 + 24 * s['frac_cdm'])) / 4.
    s['p_cb'] = (5. - np.sqrt(1 + 24. * s['frac_cb'])) / 4.
    y_drag = (1 + s['z_eq']) / (1 + s['z_drag'])
    Nf = dtype(N)
    with np.errstate(all='ignore'):      # (without species frac_ncdm is the rounding of 1 - frac_cb, of either sign: its root is multiplied by N = 0)
        root = np.sqrt(s['frac_ncdm'] * N) if N else np.zeros_like(h)
        alpha = s['frac_cdm'] / s['frac_cb'] * (5. - 2. * (s['p_c'] + s['p_cb'])) / (5. - 4. * s['p_cb']) * (1 + y_drag) ** (s['p_cb'] - s['p_c']) \
            * (1 + fbn * (-0.553 + 0.126 * fbn ** 2)) \
            / (1 - 0.193 * root + 0.169 * s['frac_ncdm'] * Nf ** 0.2) \
            * (1 + (s['p_c'] - s['p_cb']) / 2 * (1 + 1 / (3. - 4. * s['p_c']) / (7. - 4. * s['p_cb'])) / (1 + y_drag))
    s['gamma_ncdm'] = np.sqrt(alpha)
    s['beta_c'] = 1 / (1 - 0.949 * fbn)
    return s


def variants_transfer_kz(k, h, s, growth_k0, of='delta_m', dtype=LD, mutation=None):
    """oracle.power.variants_transfer_kz (eisenstein_hu_nowiggle_variants.py:87-154) for a batch: k (nk,), h and the scalars (n,), growth_k0 (n, nz) ->
    (n, nz, nk)."""
    dtype = np.dtype(dtype).type
    g = {n: np.asarray(v).astype(dtype)[:, None, None] for n, v in s.items() if n != 'N_ncdm'}
    k = np.asarray(k).astype(dtype)[None, None, :] * np.asarray(h).astype(dtype)[:, None, None]
    growth_k0 = np.asarray(growth_k0).astype(dtype)[:, :, None]
    q = k / g['omega_m'] * g['theta_cmb'] ** 2
    N, f = s['N_ncdm'], g['frac_ncdm']
    Nf = dtype(N)
    if N:
        yfs = 17.2 * f * (1 + 0.488 * f ** (-7. / 6.)) * (Nf * q / f) ** 2
        if mutation == 'no_yfs':
            yfs = 0. * yfs
        t1 = growth_k0 ** (1. - g['p_cb'])
        t2 = (growth_k0 / (1 + yfs)) ** 0.7
        if of == 'delta_cb':
            growth = (1. + t2) ** (g['p_cb'] / 0.7) * t1
        else:
            growth = (g['frac_cb'] ** (0.7 / g['p_cb']) + t2) ** (g['p_cb'] / 0.7) * t1
    else:
        growth = growth_k0 = np.ones_like(growth_k0)
    gamma_eff = g['omega_m'] * (g['gamma_ncdm'] + (1 - g['gamma_ncdm']) / (1 + (k * g['rs_drag'] * 0.43) ** 4))
    q_eff = q * g['omega_m'] / gamma_eff
    TL = np.log(np.e + 1.84 * g['beta_c'] * g['gamma_ncdm'] * q_eff)
    TC = 14.4 + 325. / (1 + 60.5 * q_eff ** 1.08)
    T = TL / (TL + TC * q_eff ** 2)
    if N:
        qn = 3.92 * q * np.sqrt(Nf / f)
        T = T * (1 + 1.24 * f ** 0.64 * Nf ** (0.3 + 0.6 * f) / (qn ** (-1.6) + qn ** 0.8))
    return T * growth / growth_k0


def variants_inputs(c):
    """The arguments of :func:`variants_scalars` from ``background_truth.cosmo``."""
    return (c['h'], c['Omega_cdm'], c['Omega_b'], c['T_cmb']) + omega_nu_m(c)


def variants(what, of, c, pk, k, z, mutation=None):
    """cp_power_eval_variants: (n, nz, nk) in the type of c -- transfer_kz, or the spectrum of Fourier.pk_interpolator's pk_callable
    (eisenstein_hu_nowiggle_variants.py:178-191): T^2 growth_factor(z, znorm=0)^2 x potential_to_density x curvature_to_potential x P_primordial."""
    dtype = c['dtype']
    n = c['n']
    with np.errstate(all='ignore'):
        s = variants_scalars(*variants_inputs(c), dtype=dtype)
        g = bt.elementwise(c, np.asarray(z, dtype='f8'), 'growth_cpt')
        growth_k0 = (1. + s['z_eq'])[:, None] * g      # growth_factor(z, znorm=z_eq), eisenstein_hu.py:134-139
        T = variants_transfer_kz(k, c['h'], s, growth_k0, of, dtype, mutation)
        if what == 'transfer':
            return T
        pk = np.asarray(pk, dtype='f8').reshape(n, len(PK_PARAMS)).astype(dtype)
        kk = np.broadcast_to(np.asarray(k, dtype='f8').astype(dtype), (n, np.size(k)))
        prim = primordial_pk(kk, c['h'], *(pk[:, i] for i in range(5)), dtype=dtype)
        Opn, Oppn = omega_nu_m(c)
        Omega0_m = c['Omega_b'] + c['Omega_cdm'] + sum_species(Opn) - sum_species(Oppn)
        potential_to_density = (3. * Omega0_m[:, None] * 100**2 / (2. * bt.C_KMS**2 * kk**2)) ** (-2)
        curvature_to_potential = 9. / 25. * 2. * np.pi**2 / kk**3 / c['h'][:, None] ** 3
        pdd = potential_to_density * curvature_to_potential * prim
        return T**2 * (g**2)[:, :, None] * pdd[:, None, :]


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------------------

def against(scale, dev, truth, f64):
    """(dev, truth, f64) moved so that ``assert_pointwise``'s relative rule is the rule against ``scale`` (> 0) in place of |truth|: the truth becomes
    the scale, the two others keep their distances from it (in longdouble)."""
    truth = np.asarray(truth).astype(LD)
    scale = np.broadcast_to(np.asarray(scale).astype(LD), truth.shape)
    return scale + (np.asarray(dev).astype(LD) - truth), scale, scale + (np.asarray(f64).astype(LD) - truth)


def decade_rows(a, k, n):
    """a (n, nk) or (n, nz, nk) as rows of one (cosmology, decade of k) block each, (n x decades, most), short rows padded with NaN."""
    a = np.asarray(a)
    a = a.reshape(n, -1, np.size(k))
    decade = np.floor(np.log10(np.asarray(k, dtype='f8')))
    blocks = [a[:, :, decade == d].reshape(n, -1) for d in np.unique(decade)]
    most = max(b.shape[1] for b in blocks)
    out = np.full((len(blocks), n, most), np.nan, dtype=a.dtype)
    for i, b in enumerate(blocks):
        out[i, :, :b.shape[1]] = b
    return out.reshape(-1, most)


def prepared(engine, what, k, dev, truth, f64, x=None):
    """The three results of a case as the rows of the rule, against the scale of (engine, what): the module's docstring.  ``x``: :func:`analytic_x` in
    longdouble (BBKS)."""
    truth = np.asarray(truth)
    n = truth.shape[0]
    scale = None
    if what == 'log_k_matter':
        scale = np.maximum(1., np.abs(truth))
    if engine == 'bbks' and what != 'primordial':
        w = 1. + (1. if what == 'transfer' else 2.) / np.asarray(x).astype(LD)
        w = w if truth.ndim == 2 else w[:, None, :]
        scale = w * (np.abs(truth) if scale is None else scale)
    if scale is not None:
        dev, truth, f64 = against(scale, dev, truth, f64)
    return tuple(decade_rows(a, k, n) for a in (dev, truth, f64))


def level_floors(engine, what, k, truth, f64, x=None, weighted=True):
    """The largest level of the case's rows, in FLOORs (``weighted`` False: BBKS without its weight)."""
    _, t, f = prepared(engine if weighted else 'unweighted', what, k, truth, truth, f64, x)
    return float(bt.pointwise_level(t, f).max() / FLOOR)


def assert_quantity(engine, what, k, dev, truth, f64, x=None, name='', extra=None, measure_only=False):
    """The device's result of a case within the rule; returns (largest fraction of the allowance, largest level in FLOORs).  ``extra``: another one than
    the rule's, with ``measure_only`` (a figure beside the assertion)."""
    d, t, f = prepared(engine, what, k, dev, truth, f64, x)
    assert extra is None or measure_only
    extra = extra_of(engine, what) if extra is None else extra
    worst = assert_pointwise(d, t, f, '%s %s, %s' % (engine, what, name), extra=extra, cap=cap_of(what), measure_only=measure_only)
    return worst, float(bt.pointwise_level(t, f).max() / FLOOR)


ABSOLUTE_SCALARS = {'frac_ncdm': 1., 'p_c': 1.25, 'p_cb': 1.25}      # differences: held against their minuend (the module's docstring)


def prepared_scalars(names, dev, truth, f64, weights):
    """dicts name -> (n,) as rows of one (cosmology, scalar) entry each, (n x names, 1); ``weights``: 'alpha_b_weight' of the longdouble truth."""
    out = []
    for name in names:
        d, t, f = (np.asarray(a[name]) for a in (dev, truth, f64))
        if name == 'alpha_b':
            d, t, f = against(weights['alpha_b_weight'] * np.abs(t), d, t, f)
        if name in ABSOLUTE_SCALARS:
            d, t, f = against(np.full_like(t, ABSOLUTE_SCALARS[name]), d, t, f)
        out.append([np.asarray(a).astype(LD) for a in (d, t, f)])
    return tuple(np.concatenate([o[i] for o in out])[:, None] for i in range(3))


# ---- the launch shapes (cp_power.hip: cp_power_eval, split_wavenumbers) ----------------------------------------------------------------------------------

def split_wavenumbers(ncosmo, nk, block):
    """(kspan, kchunks, kiter) of split_wavenumbers."""
    kiter = (nk + block - 1) // block
    while kiter > 1 and ncosmo * ((nk + block * kiter - 1) // (block * kiter)) < 2048:
        kiter = (kiter + 1) // 2
    kspan = block * kiter
    return kspan, (nk + kspan - 1) // kspan, kiter


def launch_shape(ncosmo, nk, nz=0, variants=False):
    """What a launch of cp_power_eval (``variants``: of cp_power_eval_variants, always 256 threads) reaches: dict with block, kspan, kchunks, kiter and the
    edges -- 'kiter' (a thread walks more than one wavenumber), 'partial_pass' (the last pass of a workgroup's walk leaves lanes idle), 'partial_chunk' (the
    last workgroup of a cosmology has fewer wavenumbers than kspan, and there is more than one), 'z_blocks' (more redshifts than threads),
    'one_wave' (block 64)."""
    block = 64 if (ncosmo >= 256 * 12 and not variants) else 256
    kspan, kchunks, kiter = split_wavenumbers(ncosmo, nk, block)
    last = nk - (kchunks - 1) * kspan
    return dict(block=block, kspan=kspan, kchunks=kchunks, kiter=kiter, one_wave=block == 64, edges=dict(
        kiter=kiter > 1, partial_pass=last % block != 0, partial_chunk=kchunks > 1 and last != kspan, z_blocks=nz > block, one_wave=block == 64))


# ---- the cases of the device tests (tests/test_power_truth_host.py holds every block of them below its cap) ---------------------------------------------

BG_SCALARS = bt.SCALAR_PARAMS      # T_cmb and N_ur go as scalars in the calls that mix the two forms
PK_SCALARS = (1, 4)                # ... and n_s and k_pivot
K_SMALL = np.geomspace(1e-4, 30., 61)
SMALLEST_NORMAL = 2.2250738585072014e-308


def primordial_parameters(n, seed):
    """(n, 5) float64: A_s, n_s, non-zero alpha_s and beta_s, a k_pivot that is not the default."""
    rng = np.random.default_rng(seed)
    sign = np.where(rng.uniform(size=(2, n)) < 0.5, -1., 1.)
    return np.stack([rng.uniform(1e-9, 3e-9, n), rng.uniform(0.9, 1., n), sign[0] * rng.uniform(0.002, 0.01, n), sign[1] * rng.uniform(0.002, 0.01, n),
                     rng.uniform(0.03, 0.07, n)], axis=1)


def spread(n, count, always=()):
    """``count`` members of a batch of n, in order: ``always``, the first, the last and the rest spread evenly."""
    if n <= count:
        return np.arange(n)
    picked = sorted(set(int(i) for i in always if i < n) | {0, n - 1})
    for i in np.linspace(0, n - 1, 4 * count).astype(int):
        if len(picked) >= count:
            break
        if int(i) not in picked:
            picked.append(int(i))
    return np.array(sorted(picked))


def make_case(name, ncosmo, k, nz=0, kscale=False, nsp=0, mixed=False, second_is_omega_m=0, rows=None, seed=0, engines=ENGINES, whats=WHATS, edges=(),
              masses=(0.06, 0.1, 0.3)):
    """A batch of the device tests: p (ncosmo, 8) and pk (ncosmo, 5) as the call computes them (``mixed``: the columns BG_SCALARS and PK_SCALARS go as
    scalars), the shared wavenumbers, ``nz`` redshifts from 0 to 10, not sorted, for 'matter', factors ``kscale`` in [0.9, 1.1], the tables of ``nsp``
    massive species (float64, an input), the members ``rows`` that are compared with the truth, the engines and quantities that are run and the edges
    of ``launch_shape`` the case is there for."""
    seed = 1000 + seed
    rng = np.random.default_rng(seed)
    p = bt.cosmologies(ncosmo, 'alternating', seed, nan_member=False)
    pk = primordial_parameters(ncosmo, seed + 1)
    if mixed:
        p = bt.with_scalars(p, BG_SCALARS)
        pk[:, list(PK_SCALARS)] = pk[0, list(PK_SCALARS)]
    z = None
    if nz:
        z = rng.uniform(0., 10., nz)
        z[0] = 10.
        if nz > 1:
            z[-1] = 0.
    rows = np.arange(ncosmo) if rows is None else np.asarray(rows)
    tab = bt.species_tables(p, nsp, masses) if nsp else None
    return dict(name=name, p=p, pk=pk, bg_scalars=BG_SCALARS if mixed else (), pk_scalars=PK_SCALARS if mixed else (), second_is_omega_m=second_is_omega_m,
                k=np.asarray(k, dtype='f8'), z=z, kscale=rng.uniform(0.9, 1.1, ncosmo) if kscale else None, nsp=nsp, tab=tab, rows=rows, engines=tuple(engines),
                whats=tuple(whats), edges=tuple(edges), ncosmo=ncosmo, nk=np.size(k), nz=nz)


def case_cosmo(case, dtype=LD, rows=None):
    rows = case['rows'] if rows is None else rows
    return bt.cosmo(case['p'][rows], case['second_is_omega_m'], None if case['tab'] is None else case['tab'][rows], dtype=dtype)


def case_truth(case, engine, what, dtype=LD, rows=None, mutation=None):
    """:func:`analytic` of the members ``rows`` of a case in ``dtype``."""
    rows = case['rows'] if rows is None else rows
    c = case_cosmo(case, dtype, rows)
    return analytic(engine, what, c, case['pk'][rows], case['k'], case['z'] if what == 'matter' else None,
                    None if case['kscale'] is None else case['kscale'][rows], mutation)


def case_x(case, rows=None):
    rows = case['rows'] if rows is None else rows
    return analytic_x(case_cosmo(case, LD, rows), case['k'], None if case['kscale'] is None else case['kscale'][rows])


@functools.lru_cache(maxsize=None)
def analytic_cases():
    """The batches of cp_power_eval, in the order of the device test's docstring."""
    out = []
    for n in (1, 63, 64, 65):      # the pre-kernel: one lane per cosmology, 64 per workgroup; scalars and arrays in one launch, Omega_m for Omega_cdm
        out.append(make_case('pre-kernel, %d cosmologies' % n, n, K_SMALL, mixed=True, second_is_omega_m=1, seed=300 + n))      # (seed n: over the cap, the docstring)
    for nk in (1, 255, 256, 257):      # 256 threads, one wavenumber each
        out.append(make_case('3 cosmologies x %d wavenumbers' % nk, 3, np.geomspace(1e-4, 30., nk) if nk > 1 else np.array([0.1]), kscale=nk == 257, seed=10 + nk))
    out.append(make_case('kiter > 1: 1024 cosmologies x 1100 wavenumbers', 1024, np.geomspace(1e-4, 50., 1100), rows=spread(1024, 24), seed=20,
                         edges=('kiter', 'partial_pass', 'partial_chunk')))
    for n in (3071, 3072):      # both sides of the switch to one wave per cosmology
        for nk in (64, 65, 341):
            out.append(make_case('%d cosmologies x %d wavenumbers' % (n, nk), n, np.geomspace(1e-3, 5., nk), kscale=nk == 341, rows=spread(n, 32, (0, 1, 63, 64)),
                                 seed=30 + nk + n, edges=('one_wave',) * (n == 3072) + ('kiter', 'partial_pass') * (nk != 64 and n == 3072)))
    for nz in (1, 256, 257):      # the blocks of redshifts of the 256-thread shape
        out.append(make_case('3 cosmologies x 70 wavenumbers x %d redshifts' % nz, 3, np.geomspace(1e-3, 5., 70), nz=nz, seed=40 + nz, whats=('matter',),
                             edges=('z_blocks',) * (nz == 257)))
    for nz in (64, 65):      # ... and of the one-wave shape
        out.append(make_case('3072 cosmologies x 65 wavenumbers x %d redshifts' % nz, 3072, np.geomspace(1e-3, 5., 65), nz=nz, rows=spread(3072, 32, (0, 1, 63, 64)),
                             seed=50 + nz, whats=('matter',), edges=('one_wave', 'kiter', 'partial_pass') + ('z_blocks',) * (nz == 65)))
    for nsp in (1, 3):      # massive species: Omega_m of the BBKS shape parameter, Omega0_m and the growth factor of EH98's spectrum
        for som in (0, 1):
            out.append(make_case('%d species, parameter 1 %s, bbks' % (nsp, 'Omega_m' if som else 'Omega_cdm'), 3, K_SMALL, nz=5, nsp=nsp, second_is_omega_m=som,
                                 seed=60 + 2 * nsp + som, engines=('bbks',), whats=('transfer', 'matter', 'log_k_matter')))
            out.append(make_case('%d species, parameter 1 %s, eisenstein_hu' % (nsp, 'Omega_m' if som else 'Omega_cdm'), 3, K_SMALL, nz=5, nsp=nsp,
                                 second_is_omega_m=som, seed=60 + 2 * nsp + som, engines=('eisenstein_hu',), whats=('matter',)))
    # the wavenumbers
    out.append(make_case('geomspace(1e-8, 1e2)', 3, np.geomspace(1e-8, 1e2, 401), seed=70))
    out.append(make_case('linspace(7e-5, 7, 4096) of wallish2018', 3, np.linspace(7e-5, 7., 4096), seed=71))
    out.append(make_case('3e3 to 3e5 h/Mpc: k rs_drag across 1e6', 3, np.geomspace(3e3, 3e5, 129), seed=72))
    # subnormal and smallest normal wavenumbers: the transfer functions only (T = 1 to rounding) -- k P underflows in float64, and the tilt's exponent takes
    # log k = -740 times O(0.1) factors, whose float64 rounding no power function sees
    tiny = np.array([5e-324, 1e-320, np.nextafter(SMALLEST_NORMAL, 0.), SMALLEST_NORMAL, np.nextafter(SMALLEST_NORMAL, 1.), 1e-300])
    out.append(make_case('subnormal and smallest normal wavenumbers', 3, tiny, seed=73, whats=('transfer',)))
    return out


VARIANTS_SHAPES = ((1, 1, 1), (3, 256, 257), (3, 257, 256), (1, 257, 1))      # (ncosmo, nk, nz)
VARIANTS_MASSES = (0.06, 0.1, 0.3)


@functools.lru_cache(maxsize=None)
def variants_cases(nsp):
    out = [make_case('variants, %d species, %d cosmologies x %d wavenumbers x %d redshifts' % ((nsp,) + shape), shape[0], np.geomspace(1e-4, 30., shape[1])
                     if shape[1] > 1 else np.array([0.1]), nz=shape[2], nsp=nsp, mixed=shape[0] == 3 and shape[1] == 256, seed=80 + 10 * nsp + i,
                     whats=('matter', 'transfer'), edges=('z_blocks',) * (shape[2] == 257), masses=VARIANTS_MASSES) for i, shape in enumerate(VARIANTS_SHAPES)]
    if nsp != 1:
        out.append(make_case('variants, %d species, kiter > 1: 1024 cosmologies x 1100 wavenumbers x 2 redshifts' % nsp, 1024, np.geomspace(1e-4, 50., 1100), nz=2,
                             nsp=nsp, rows=spread(1024, 24), seed=120 + nsp, whats=('matter', 'transfer'), edges=('kiter', 'partial_pass', 'partial_chunk'),
                             masses=VARIANTS_MASSES))
    return out


def variants_truth(case, what, of, dtype=LD, rows=None, mutation=None):
    rows = case['rows'] if rows is None else rows
    return variants(what, of, case_cosmo(case, dtype, rows), case['pk'][rows], case['k'], case['z'], mutation)


SCALAR_COUNTS = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def scalars_case(n, nsp):
    return make_case('scalars, %d cosmologies, %d species' % (n, nsp), n, K_SMALL, nsp=nsp, mixed=n % 2 == 0, second_is_omega_m=int(n in (255, 256)), seed=200 + n + nsp)


def scalars_truth(case, which, dtype=LD, parts=False):
    """dict name -> (n,) of cp_eh_scalars (``which`` 'eh') or cp_variants_scalars ('variants': that entry takes parameter 1 as Omega_cdm, whatever the
    case says for cp_eh_scalars) in ``dtype``."""
    if which == 'eh':
        return scalars_of(case_cosmo(case, dtype), parts=parts)
    return variants_scalars(*variants_inputs(case_cosmo(dict(case, second_is_omega_m=0), dtype)), dtype=dtype)
