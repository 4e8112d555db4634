"""Restatement of the background kernels (csrc/cp_background.hip, csrc/cp_cosmo_common.h) for tests/test_background_truth_host.py and
tests/test_background_edges_gpu.py: every operation in numpy, in any floating-point type.  ``np.longdouble`` is the truth, float64 the reference
implementation that is not the code under test.  numpy only (no scipy); the natural-spline solve is ``spline_truth.slopes`` (a Thomas solve for the
first derivatives over ALL knots: no truncated elimination, no reach).

Operation order: that of the reference as oracle/background.py cites it (file:line there) -- the expressions of ``oracle.background.derived``, ``efunc``,
``densities``, ``distance_table``, ``time_table``, ``romberg``, ``rs``, ``growth_ode_tables`` with a ``dtype`` and with the splined densities of massive
species where ``efunc_ncdm`` has them -- and that of the kernel where only the kernel states one (``ncdm_momenta_kernel``'s prefactors,
``spline_m_eval``, ``derived_parameters_kernel``, ``load_cosmo``'s species sums).  The knots (119 of the distances and of the species, 400 of time,
201 of the growth ODE) are taken from the library's host exports; they are exact inputs of the truth, as are the physical constants (float64 values).

What a cosmology is: ``cosmo(params, second_is_omega_m, tab)`` with params (n, 8) in the order of enum cp_bg_param and, with massive species, their
spline tables (n, nsp, 4, 119) as ``cp_ncdm`` takes them -- float64 INPUTS of the entry points (the device tests upload the float64 restatement of
``cp_ncdm_tables``), so truth and device interpolate in the same bits.

Tolerance rule (tests/jacobian_reference.py): ``level`` is the float64 restatement's distance from the longdouble truth, floored
at FLOOR = 1.1e-16; the device must lie within ALLOW = 16 levels of the truth.  Blocks:
  :func:`assert_pointwise`  distances and the elementwise quantities, ``rs``: a block is a cosmology's row (``rs``: one sample), its level the row's largest
                            RELATIVE error of the restatement, and every entry is held relative to itself, allowed_ij = (ALLOW level_i + extra) |truth_ij|
                            (a row holds z from 1e-3 to 9999: the row's largest entry as the scale would hide everything at low z);
  :func:`assert_blocks`     time (absolute against the row's age: the cancellation T_last - T(z) is the reference's own), the growth tables, the species'
                            tables (against the table's largest entry; their second derivatives: the last paragraph).
``extra`` is zero except for the four distance kinds, where it is DISTANCE_EXTRA = 1e-14: what the kernel's truncated backward elimination documents
(the comment under CP_BG_REACH_LEFT: 1e-13 of the cubic's correction inside one interval, "below 1e-14 of the distance").  No further term is added
for the device.  One term comes from the number format itself: a float64 below 2^-1022 has no relative precision (the distance at the first float64
above z = 0 is 1e-320), so an entry whose truth is subnormal does not count for the row's level; it has a level of its own, ABSOLUTE -- the device
is allowed ALLOW times the float64 restatement's distance from the truth at that entry (sin(sqrt(K) chi) / sqrt(K) with a subnormal product is off by
thousands of subnormal spacings in any float64 arithmetic) -- and every non-zero entry is allowed one subnormal spacing, 2^-1074, on top: the rounding
of the one product that forms it.  A truth of exactly zero (D(0)) must be met exactly.
A case is used on the device only while the level of its restatement stays below CAP = 32 floors (the condition of tests/spline_truth.py);
tests/test_background_truth_host.py holds every case of the device tests to it.

Over the cap and therefore not held to the rule: the SECOND DERIVATIVES of the species' tables, in every case (measured by
tests/test_background_truth_host.py as ``block_level`` of the float64 and the longdouble ``ncdm_truth``, per table against its largest entry: the largest
level of a shape's tables is 7e11 to 3e12 FLOOR over the species of non-zero mass, and 2e19 to 5e19 FLOOR for the species of mass 0, whose truth is
itself rounding noise).  They are second differences of values that carry
1e-16 of themselves, over knots 1 / 19 apart, of functions that are straight lines at both ends of the grid (exactly so for a mass of 0): the rounding
of the values is 1e-4 of the largest second derivative and no float64 restatement is closer to the truth than that.  The device tests hold them by
their consequence instead -- the splines through the device's values and second derivatives at the midpoint of every interval, pointwise relative
(levels below the cap) -- and hold the tabulated values pointwise as well as against the table's largest entry.
"""
import ctypes
import functools

import numpy as np

import spline_truth as st
from jacobian_reference import LD, FLOOR, ALLOW

CAP = 32.
DISTANCE_EXTRA = 1e-14
SMALLEST_NORMAL, SUBNORMAL_SPACING = 2.**-1022, 2.**-1074
NPARAMS = 8
PARAMS = ('h', 'Omega_cdm', 'Omega_b', 'Omega_k', 'T_cmb', 'N_ur', 'w0_fld', 'wa_fld')      # enum cp_bg_param
NK_DIST, NK_TIME, NK_NCDM, NK_GROWTH = 119, 400, 119, 201
DERIVED_NVALUES = 17

# cosmoprimo/constants.py:9-21 with scipy.constants' float64 values written out (tests/test_background_truth_host.py holds them to the oracle's)
C = 299792458.0
STEFAN_BOLTZMANN = 5.6703744191844314e-08
PARSEC = 3.085677581491367e16
GRAVITATIONAL = 6.6743e-11
PI = 3.141592653589793
ELECTRON_VOLT, BOLTZMANN = 1.602176634e-19, 1.380649e-23
MPC = 1e6 * PARSEC
MSUN = 1.98847 * 1e30
RHO_CRIT_KG = 3.0 * (100. * 1e3 / MPC)**2 / (8 * PI * GRAVITATIONAL)
RHO_CRIT = RHO_CRIT_KG / (1e10 * MSUN) * MPC**3
C_KMS = C / 1e3
GIGAYEAR_OVER_MEGAPARSEC = 3.06601394e2
T_UR_OVER_CMB = 0.7137658555036082      # (4 / 11)^(1 / 3)

KINDS = {'comoving_radial_distance': 0, 'comoving_transverse_distance': 1, 'angular_diameter_distance': 2, 'luminosity_distance': 3, 'efunc': 4,
         'hubble_function': 5, 'growth_cpt': 6, 'growth_rate': 7, 'rho_crit': 8, 'Omega_m': 9, 'Omega_de': 10, 'rho_g': 11, 'rho_b': 12, 'rho_ur': 13,
         'rho_cdm': 14, 'rho_k': 15, 'rho_Lambda': 16, 'rho_fld': 17, 'rho_de': 18, 'rho_tot': 19, 'rho_m': 20, 'rho_r': 21, 'T_cmb': 22, 'time': 23,
         'age': 24, 'rho_ncdm': 25, 'p_ncdm': 26, 'rs': 27, 'rs_cosmomc': 28}      # enum cp_bg_kind
AS_FRACTION = 32
DISTANCE_KINDS = ('comoving_radial_distance', 'comoving_transverse_distance', 'angular_diameter_distance', 'luminosity_distance')
DENSITY_KINDS = ('rho_g', 'rho_b', 'rho_ur', 'rho_cdm', 'rho_k', 'rho_Lambda', 'rho_fld', 'rho_de', 'rho_tot', 'rho_m', 'rho_r', 'rho_ncdm', 'p_ncdm')
PLAIN_KINDS = ('efunc', 'hubble_function', 'growth_cpt', 'growth_rate', 'rho_crit', 'Omega_m', 'Omega_de', 'T_cmb')
# what cp_background_eval refuses with CP_BG_AS_FRACTION: everything below rho_g, T_cmb, time, age, rs, rs_cosmomc
FRACTION_ILLEGAL = DISTANCE_KINDS + ('efunc', 'hubble_function', 'growth_cpt', 'growth_rate', 'rho_crit', 'Omega_m', 'Omega_de', 'T_cmb', 'time', 'age',
                                     'rs', 'rs_cosmomc')


# ---- knots ---------------------------------------------------------------------------------------------------------------------------------------------

def knots(which):
    """The knots every function of this module takes: the library's (host-only exports, no device) -- 'distance' (119), 'time' (400), 'ncdm' (119),
    'growth' (201, ascending z)."""
    return library_knots(which)


@functools.lru_cache(maxsize=None)
def library_knots(which):
    from cosmoprimo_amd import _lib
    name, n = {'distance': ('cp_background_knots', NK_DIST), 'time': ('cp_background_knots', NK_TIME), 'ncdm': ('cp_ncdm_knots', NK_NCDM),
               'growth': ('cp_growth_ode_knots', NK_GROWTH)}[which]
    out = np.empty(n)
    _lib.check(getattr(_lib.load(), name)(out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n))
    out.setflags(write=False)
    return out


def growth_eta():
    """eta = ln a of the growth ODE (cosmology.py:2060): the library's knots are exp(-eta) - 1 of these, reversed."""
    return np.linspace(-6., 0., NK_GROWTH)


def reach(zc, left=1e-13):
    """build_pivots' ``reach`` from its comment: the smallest 8 + 4 i after which the product of the backward elimination's multipliers u_j / pivot_j is
    below ``left`` (CP_BG_REACH_LEFT) wherever it starts."""
    return pivots(zc, left)['reach']


def pivots(zc, left=1e-13):
    """The grid-only constants of bg_kernel's eliminations (build_pivots), float64."""
    n = zc.size
    dx = np.append(np.diff(zc), 0.)
    low, b, u, ra, rb = (np.zeros(n) for _ in range(5))
    b[0], u[0], rb[0] = 2. * dx[0], dx[0], 3.
    low[1:-1], b[1:-1], u[1:-1] = dx[1:-1], 2. * (dx[:-2] + dx[1:-1]), dx[:-2]
    ra[1:-1], rb[1:-1] = 3. * dx[1:-1] / dx[:-2], 3. * dx[:-2] / dx[1:-1]
    low[-1], b[-1], ra[-1] = dx[-2], 2. * dx[-2], 3.
    idf, cp, idb, bq = (np.zeros(n) for _ in range(4))
    idf[0] = 1. / b[0]
    cp[0] = u[0] * idf[0]
    for i in range(1, n):
        idf[i] = 1. / (b[i] - low[i] * cp[i - 1])
        cp[i] = u[i] * idf[i]
    idb[-1] = 1. / b[-1]
    bq[-1] = low[-1] * idb[-1]
    for i in range(n - 2, -1, -1):
        idb[i] = 1. / (b[i] - u[i] * bq[i + 1])
        bq[i] = low[i] * idb[i]
    mult = np.abs(u * idb)
    r = 8
    while r < n:
        worst = max((np.prod(mult[j:j + r]) for j in range(1, n - r)), default=0.)
        if worst < left:
            break
        r += 4
    return dict(zc=zc, dx=dx, l=low, u=u, ra=ra, rb=rb, idf=idf, cp=cp, idb=idb, bq=bq, reach=r)


def kernel_spline(P, inc, z, reach=None, inc_up_last=0.):
    """bg_kernel's route to the spline's value at the samples z (m,) of ONE cosmology from its increments inc (NK - 1,), float64: the forward elimination
    up to the sample's interval k, the backward one started ``reach`` knots above it, the 2 x 2 system.  For the host test's neighbours (a shorter
    ``reach``; ``inc_up_last``: what closes the elimination at k == NK - 2 in place of 0)."""
    zc, NK = P['zc'], P['zc'].size
    reach = P['reach'] if reach is None else reach
    out = np.full(len(z), np.nan)
    for n, zz in enumerate(z):
        if not (zz >= zc[0] and zz <= zc[-1]):
            continue
        k = min(max(int(np.searchsorted(zc, zz, side='right')) - 1, 0), NK - 2)
        dp = inc_prev = tk = 0.
        for idx in range(k + 1):
            d = P['ra'][idx] * inc_prev + P['rb'][idx] * inc[idx]
            dp = (d - P['l'][idx] * dp) * P['idf'][idx]
            if idx < k:
                tk = tk + inc[idx]
            inc_prev = inc[idx]
        inc_k = inc[k]
        top = min(k + 1 + reach, NK - 1)
        dq = inc_prev = 0.
        for idx in range(top - 1, k, -1):
            d = P['ra'][idx + 1] * inc[idx] + P['rb'][idx + 1] * inc_prev
            dq = (d - P['u'][idx + 1] * dq) * P['idb'][idx + 1]
            inc_prev = inc[idx]
        inc_up = inc_up_last if k == NK - 2 else inc_prev
        d = P['ra'][k + 1] * inc_k + P['rb'][k + 1] * inc_up
        dq = (d - P['u'][k + 1] * dq) * P['idb'][k + 1]
        cpk, bqk = P['cp'][k], P['bq'][k + 1]
        sk = (dp - cpk * dq) / (1. - cpk * bqk)
        sk1 = dq - bqk * sk
        hk = P['dx'][k]
        slope = inc_k / hk
        tt = (sk + sk1 - 2. * slope) / hk
        c3, c2 = tt / hk, (slope - sk) / hk - tt
        dz = zz - zc[k]
        out[n] = tk + dz * (sk + dz * (c2 + dz * c3))
    return out


# ---- the cosmology -------------------------------------------------------------------------------------------------------------------------------------

def cosmo(params, second_is_omega_m=0, tab=None, dtype=LD):
    """The per-cosmology block (load_cosmo; cosmology.py:355-397, 1163-1165): dict of (n,) arrays in ``dtype``.  params (n, 8) float64; tab: the species'
    tables (n, nsp, 4, 119) float64, or None."""
    dtype = np.dtype(dtype).type
    p = np.asarray(params, dtype='f8').reshape(-1, NPARAMS).astype(dtype)
    h, second, Omega_b, Omega_k, T_cmb, N_ur, w0, wa = (p[:, i] for i in range(NPARAMS))
    Omega_cdm = second - Omega_b if second_is_omega_m else second
    with np.errstate(all='ignore'):
        rho_g = T_cmb**4 * 4. / dtype(C)**3 * STEFAN_BOLTZMANN
        Omega_g = rho_g / (h**2 * RHO_CRIT_KG)
        T_ur = T_cmb * T_UR_OVER_CMB
        rho_ur = N_ur * 7. / 8. * T_ur**4 * 4. / dtype(C)**3 * STEFAN_BOLTZMANN
        Omega_ur = rho_ur / (h**2 * RHO_CRIT_KG)
        Omega_ncdm_tot = np.zeros_like(h)
        if tab is not None:
            tab = np.asarray(tab, dtype='f8').astype(dtype)
            rho0, p0 = np.zeros_like(h), np.zeros_like(h)
            for s in range(tab.shape[1]):
                rho0 = rho0 + tab[:, s, 0, 0]
                p0 = p0 + tab[:, s, 2, 0]
            Omega_ncdm_tot = rho0 / RHO_CRIT
            if second_is_omega_m:
                Omega_cdm = Omega_cdm - (rho0 - 3 * p0) / RHO_CRIT
        Omega_de = 1. - (Omega_cdm + Omega_b + Omega_g + Omega_ur + Omega_ncdm_tot + Omega_k)
        K = -100.**2 / dtype(C_KMS)**2 * Omega_k
    return dict(h=h, Omega_cdm=Omega_cdm, Omega_b=Omega_b, Omega_k=Omega_k, Omega_g=Omega_g, Omega_ur=Omega_ur, Omega_de=Omega_de, w0_fld=w0, wa_fld=wa,
                K=K, T_cmb=T_cmb, N_ur=N_ur, tab=tab, dtype=dtype, n=h.size)


def take(c, index):
    """The cosmologies ``index`` of c."""
    out = {k: (v[index] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    out['n'] = out['h'].size
    return out


def _rows(c, z):
    """z as (n, m) in the type of c; z (m,) is shared by the cosmologies."""
    z = np.asarray(z)
    if z.ndim == 1:
        z = np.broadcast_to(z, (c['n'], z.size))
    return z.astype(c['dtype'])


def ncdm_eval(c, z, which, species=-1, leave_out=None):
    """ncdm_eval of cp_cosmo_common.h: the species' splined densities (which = 0) or pressures (1) at z (n, m), summed in the order of the species (or one
    species); zero without species, NaN outside the knots.  ``leave_out``: a species the sum forgets (the host test's neighbour)."""
    z = _rows(c, z)
    if c['tab'] is None:
        return np.zeros_like(z)
    x = knots('ncdm').astype(c['dtype'])
    with np.errstate(invalid='ignore'):
        inside = (z >= x[0]) & (z <= x[-1])
    lo = np.clip(np.searchsorted(x, np.where(inside, z, x[0]).ravel(), side='right').reshape(z.shape) - 1, 0, x.size - 2)
    hh = x[lo + 1] - x[lo]
    a, b = (x[lo + 1] - z) / hh, (z - x[lo]) / hh
    rows = np.arange(c['n'])[:, None]
    tot = np.zeros_like(z)
    for s in range(c['tab'].shape[1]):
        if (species >= 0 and s != species) or s == leave_out:
            continue
        y, m = c['tab'][:, s, 2 * which], c['tab'][:, s, 2 * which + 1]
        tot = tot + (a * y[rows, lo] + b * y[rows, lo + 1] + ((a * a * a - a) * m[rows, lo] + (b * b * b - b) * m[rows, lo + 1]) * (hh * hh) / 6.)
    tot[~inside] = np.nan
    return tot


def densities(c, z, leave_out=None, drop_pressure=False):
    """BaseBackground.rho_x(z) (cosmology.py:1680-1749) at z (n, m), with the splined species (DefaultBackground.rho_ncdm / p_ncdm): dict name -> (n, m).
    rho_Lambda and rho_fld are the two forms of the dark energy as the kernel has them (the caller knows which one is the cosmology's)."""
    z = _rows(c, z)
    col = {k: c[k][:, None] for k in ('Omega_cdm', 'Omega_b', 'Omega_k', 'Omega_g', 'Omega_ur', 'Omega_de', 'w0_fld', 'wa_fld')}
    rc = RHO_CRIT
    d = {}
    with np.errstate(all='ignore'):
        d['rho_ncdm'], d['p_ncdm'] = ncdm_eval(c, z, 0, leave_out=leave_out), ncdm_eval(c, z, 1, leave_out=leave_out)
        d['rho_g'] = col['Omega_g'] * (1 + z) * rc
        d['rho_b'] = col['Omega_b'] * np.ones_like(z) * rc
        d['rho_ur'] = col['Omega_ur'] * (1 + z) * rc
        d['rho_cdm'] = col['Omega_cdm'] * np.ones_like(z) * rc
        d['rho_k'] = col['Omega_k'] / (1 + z) * rc
        d['rho_de'] = col['Omega_de'] * (1 + z) ** (3. * (col['w0_fld'] + col['wa_fld'])) * np.exp(3. * col['wa_fld'] * (1. / (1 + z) - 1)) * rc
        d['rho_Lambda'] = col['Omega_de'] / (1 + z)**3 * rc
        d['rho_fld'] = col['Omega_de'] * (1 + z) ** (3. * (1 + col['w0_fld'] + col['wa_fld'])) * np.exp(3. * col['wa_fld'] * (1. / (1 + z) - 1)) * rc / (1 + z)**3
        d['rho_r'] = d['rho_g'] + d['rho_ur'] + 3. * d['p_ncdm']
        d['rho_m'] = d['rho_cdm'] + d['rho_b'] + d['rho_ncdm'] - (0. if drop_pressure else 3. * d['p_ncdm'])
        d['rho_tot'] = (d['rho_cdm'] + d['rho_b'] + d['rho_ncdm']) + (d['rho_g'] + d['rho_ur']) + d['rho_de']
        d['rho_crit'] = d['rho_tot'] + d['rho_k']
    return d


def efunc(c, z):
    """E(z) (cosmology.py:1751-1754, efunc_ncdm of the oracle) at z (n, m)."""
    z = _rows(c, z)
    with np.errstate(all='ignore'):
        return np.sqrt(densities(c, z)['rho_crit'] * (1 + z)**3 / RHO_CRIT)


def elementwise(c, z, kind, species=-1, **mutation):
    """The elementwise kinds of bg_kernel at z (n, m): ``kind`` a name of KINDS, ``fraction``: divided by rho_crit(z) (CP_BG_AS_FRACTION)."""
    kind, fraction = (kind[0], kind[1]) if isinstance(kind, tuple) else (kind, False)
    z = _rows(c, z)
    d = densities(c, z, **mutation)
    col = {k: c[k][:, None] for k in ('h', 'T_cmb', 'w0_fld', 'wa_fld')}
    with np.errstate(all='ignore'):
        if kind in ('efunc', 'hubble_function'):
            e = np.sqrt(d['rho_crit'] * (1 + z)**3 / RHO_CRIT)
            v = e if kind == 'efunc' else e * (col['h'] * 100.)
        elif kind == 'growth_cpt':      # eisenstein_hu.py:134-136
            Om, Ode = d['rho_m'] / d['rho_crit'], d['rho_de'] / d['rho_crit']
            v = 1. / (1 + z) * 5 * Om / 2. / (Om**(4. / 7.) - Ode + (1. + Om / 2.) * (1 + Ode / 70.))
        elif kind == 'growth_rate':      # eisenstein_hu.py:151-152
            Om = d['rho_m'] / d['rho_crit']
            v = Om**(0.55 + 0.05 * (1 + (col['w0_fld'] + (1. - 0.5) * col['wa_fld'])))
        elif kind == 'rho_crit':
            v = d['rho_crit']
        elif kind == 'Omega_m':
            v = d['rho_m'] / d['rho_crit']
        elif kind == 'Omega_de':
            v = d['rho_de'] / d['rho_crit']
        elif kind == 'T_cmb':
            v = col['T_cmb'] * (1 + z)
        elif kind in ('rho_ncdm', 'p_ncdm'):
            v = ncdm_eval(c, z, int(kind == 'p_ncdm'), species, leave_out=mutation.get('leave_out'))
        else:
            v = d[kind]
        if fraction:
            v = v / d['rho_crit']
    return v


# ---- the distance and time tables ----------------------------------------------------------------------------------------------------------------------

def scan_table(c, zc, time=False, mid_shift=0., simpson=False):
    """(inc (n, NK - 1), T (n, NK)): the reference's RK4 with a y-independent integrand over the knots (jax.py:700-710, cosmology.py:2005-2009,
    2036-2040), accumulated in knot order.  ``mid_shift`` (in knot spacings) and ``simpson`` (weights (1, 4, 1) / 6): the host test's neighbour."""
    zc = np.asarray(zc).astype(c['dtype'])

    def f(z):
        e = efunc(c, z)
        with np.errstate(all='ignore'):
            return C_KMS / (1. + z) / (100. * e) if time else C_KMS / (100. * e)

    t_last, t = zc[:-1], zc[1:]
    h = t - t_last
    mid = t_last + h / 2 + mid_shift * h
    with np.errstate(all='ignore'):
        k1, k2, k4 = f(t_last), f(mid), f(t)
        inc = h / 6. * (k1 + 4 * k2 + k4) if simpson else h / 6. * (k1 + 2 * k2 + 2 * k2 + k4)
        tab = np.concatenate([np.zeros((c['n'], 1), dtype=c['dtype']), np.cumsum(inc, axis=-1)], axis=-1)
    return inc, tab


def spline_rows(x, y, z, bc='natural'):
    """The spline through (x, y[i]) at z[i]: x (NK,) float64, y (n, NK), z (n, m) float64 -> (n, m) in the type of y; NaN outside the knots."""
    dtype = y.dtype
    z = np.asarray(z, dtype='f8')
    with np.errstate(all='ignore'):
        s = st.slopes(x, y, bc, dtype)
        xd = np.asarray(x).astype(dtype)
        inside = (z >= x[0]) & (z <= x[-1])
        j = np.clip(np.searchsorted(x, np.where(inside, z, x[0]).ravel(), side='right').reshape(z.shape) - 1, 0, x.size - 2)
        rows = np.arange(y.shape[0])[:, None]
        h = xd[j + 1] - xd[j]
        delta = (y[rows, j + 1] - y[rows, j]) / h
        s0, s1 = s[rows, j], s[rows, j + 1]
        c2 = (3 * delta - 2 * s0 - s1) / h
        c3 = (s0 + s1 - 2 * delta) / h**2
        t = z.astype(dtype) - xd[j]
        v = y[rows, j] + t * (s0 + t * (c2 + t * c3))
    v[~inside] = np.nan
    return v


def curvature_map(chi, K):
    """S_K(chi) (cosmology.py:1862-1868); K (n,) against chi (n, m), or a scalar."""
    K = np.broadcast_to(np.asarray(K).astype(chi.dtype)[..., None] if np.ndim(K) else chi.dtype.type(K), chi.shape)
    out = chi.copy()
    pos, neg = K > 0, K < 0
    with np.errstate(all='ignore'):
        out[pos] = np.sin(np.sqrt(K[pos]) * chi[pos]) / np.sqrt(K[pos])
        out[neg] = np.sinh(np.sqrt(-K[neg]) * chi[neg]) / np.sqrt(-K[neg])
    return out


def from_radial(chi, z, K, kind, dtype=LD):
    """cp_distance_from_radial (cosmology.py:1855-1912): chi, z (m,) float64, K a float."""
    dtype = np.dtype(dtype).type
    chi, zz = np.asarray(chi, dtype='f8').astype(dtype), np.asarray(z, dtype='f8').astype(dtype)
    with np.errstate(all='ignore'):
        da = curvature_map(chi, dtype(K)) / (1 + zz)
        return {'angular_diameter_distance': da, 'comoving_transverse_distance': da * (1. + zz), 'luminosity_distance': da * (1. + zz)**2}[kind]


def distances(c, z, kinds=DISTANCE_KINDS, bc='natural', **mutation):
    """dict kind -> (n, m): the natural spline of the WHOLE 119-knot table at z (n, m) float64 and the distances derived from it."""
    z = np.asarray(z, dtype='f8')
    if z.ndim == 1:
        z = np.broadcast_to(z, (c['n'], z.size))
    zc = knots('distance')
    dc = spline_rows(zc, scan_table(c, zc, **mutation)[1], z, bc)
    zz = z.astype(c['dtype'])
    with np.errstate(all='ignore'):
        da = curvature_map(dc, c['K']) / (1 + zz)
        out = {'comoving_radial_distance': dc, 'angular_diameter_distance': da, 'comoving_transverse_distance': da * (1. + zz),
               'luminosity_distance': da * (1. + zz)**2}
    return {kind: out[kind] for kind in kinds}


def time(c, z, order='kernel'):
    """(time (n, m), age (n,)) in Gyr (cosmology.py:2000-2025).  ``order`` 'kernel': (T_last - spline(T)(z)) / h / Gyr, what bg_kernel<NK_TIME> forms;
    'reference': the spline of (T_last - T) / h / Gyr, what DefaultBackground.time interpolates (the same function: a spline is linear in its values)."""
    z = np.asarray(z, dtype='f8')
    if z.ndim == 1:
        z = np.broadcast_to(z, (c['n'], z.size))
    zc = knots('time')
    tab = scan_table(c, zc, time=True)[1]
    h = c['h'][:, None]
    with np.errstate(all='ignore'):
        age = ((tab[:, -1:] - tab[:, :1]) / h / GIGAYEAR_OVER_MEGAPARSEC)[:, 0]
        if order == 'reference':
            return spline_rows(zc, (tab[:, -1:] - tab) / h / GIGAYEAR_OVER_MEGAPARSEC, z), age
        return (tab[:, -1:] - spline_rows(zc, tab, z)) / h / GIGAYEAR_OVER_MEGAPARSEC, age


# ---- the sound horizon ---------------------------------------------------------------------------------------------------------------------------------

def rs(c, z, cosmomc=False, divmax=15):
    """(rs, err, threshold, raw), each (n, m): the reference's fixed-depth Romberg rule (jax.py:519-660) of dsoundda (cosmology.py:1914-1933; ``cosmomc``:
    dsoundda_approx, :202-228) from a = 1e-8 to 1 / (1 + z).  rs is NaN where the rule misses its 1e-7 (``err`` is |last_row[divmax - 1] - row[divmax]|,
    ``threshold`` the smaller of 1e-7 and 1e-7 |row[divmax]|), as rs_kernel has it; ``raw`` is the rule's value whatever the verdict."""
    z = _rows(c, z)
    n, m = z.shape
    dtype = c['dtype']
    col = {k: c[k][:, None] for k in ('h', 'Omega_b', 'Omega_g')}
    omega_b = col['Omega_b'] * col['h']**2

    def f(a):      # (n, m, k)
        shape = a.shape
        a = a.reshape(n, -1)
        dtauda = 1. / (a**2 * (efunc(c, 1 / a - 1.) * (col['h'] * 100.)) / C_KMS)
        R = 3e4 * a * omega_b if cosmomc else 3 / 4. * a * col['Omega_b'] / col['Omega_g']
        return (dtauda * (3 * (1 + R))**(-0.5)).reshape(shape)

    with np.errstate(all='ignore'):
        a, b = np.full(z.shape, 1e-8, dtype=dtype), 1. / (1 + z)
        count, intrange = 1, b - a
        ordsum = 0.5 * (f(a[..., None]) + f(b[..., None]))[..., 0]
        last_row = [intrange * ordsum]
        err = np.zeros_like(z)
        for i in range(1, divmax + 1):
            count *= 2
            numtosum = count // 2
            h = (b - a) * 1. / numtosum
            ordsum = ordsum + np.sum(f((a + 0.5 * h)[..., None] + h[..., None] * np.arange(numtosum)), axis=-1)
            x = intrange * ordsum / count
            row = [x]
            for k, y in enumerate(last_row[:i]):
                x = (4.0**(k + 1) * x - y) / (4.0**(k + 1) - 1.0)
                row.append(x)
            err = np.abs(last_row[i - 1] - row[i])
            last_row = row
        res = last_row[divmax]
        threshold = np.minimum(1e-7, np.abs(res) * 1e-7)
        ok = (err < 1e-7) & (err < np.abs(res) * 1e-7)
        raw = res if cosmomc else res * col['h']
    return np.where(ok, raw, np.nan), err, threshold, raw


# ---- the growth ODE ------------------------------------------------------------------------------------------------------------------------------------

def growth_tables(c, mass=0, eta=None):
    """(D, D'/D), each (n, nknots) in ascending z: RK4 (jax.py:700-710) of D'' = f2 D + f1 D' in eta = ln a (cosmology.py:2044-2093), ``mass`` 0 ('m')
    or 1 ('cb').  ``eta``: another grid than linspace(-6, 0, 201) (the host test's neighbour)."""
    dtype = c['dtype']
    eta = (growth_eta() if eta is None else np.asarray(eta, dtype='f8')).astype(dtype)
    w0, wa = c['w0_fld'], c['wa_fld']

    def deriv(D, Dp, e):
        z = np.full((c['n'], 1), np.exp(-e) - 1., dtype=dtype)
        d = {k: v[:, 0] for k, v in densities(c, z).items()}
        z = z[:, 0]
        rc = d['rho_crit']
        Ok, Or, Ode = d['rho_k'] / rc, d['rho_r'] / rc, d['rho_de'] / rc
        Om = d['rho_m'] / rc if mass == 0 else d['rho_cdm'] / rc + d['rho_b'] / rc
        w_fld = w0 + z / (1. + z) * wa
        f1 = -1. - (-1. / 2. * (1. - Ok + Or + 3 * w_fld * Ode))
        f2 = 3. / 2. * Om
        return Dp, f2 * D + f1 * Dp

    with np.errstate(all='ignore'):
        D = np.full(c['n'], np.exp(eta[0]), dtype=dtype)
        Dp = D.copy()
        out, t_last = [], eta[0]
        for t in eta:
            h = t - t_last
            a1, b1 = deriv(D, Dp, t_last)
            a2, b2 = deriv(D + h * a1 / 2, Dp + h * b1 / 2, t_last + h / 2)
            a3, b3 = deriv(D + h * a2 / 2, Dp + h * b2 / 2, t_last + h / 2)
            a4, b4 = deriv(D + h * a3, Dp + h * b3, t)
            D = D + h / 6. * (a1 + 2 * a2 + 2 * a3 + a4)
            Dp = Dp + h / 6. * (b1 + 2 * b2 + 2 * b3 + b4)
            out.append((D, Dp / D))
            t_last = t
    return np.array([o[0] for o in out[::-1]]).T, np.array([o[1] for o in out[::-1]]).T


# ---- the species' tables -------------------------------------------------------------------------------------------------------------------------------

def second_derivatives(x, y):
    """The second derivatives of the natural splines through the rows y (..., n) at the knots x (n,), in the type of y:
    h_{i-1} m_{i-1} + 2 (h_{i-1} + h_i) m_i + h_i m_{i+1} = 6 (slope_i - slope_{i-1}), m_0 = m_{n-1} = 0, by elimination (ncdm_spline_kernel)."""
    x = np.asarray(x).astype(y.dtype)
    n = x.size
    cp, dp = np.zeros_like(y), np.zeros_like(y)
    with np.errstate(all='ignore'):
        for j in range(1, n - 1):
            h0, h1 = x[j] - x[j - 1], x[j + 1] - x[j]
            rhs = 6. * ((y[..., j + 1] - y[..., j]) / h1 - (y[..., j] - y[..., j - 1]) / h0)
            den = 2. * (h0 + h1) - h0 * cp[..., j - 1]
            cp[..., j] = h1 / den
            dp[..., j] = (rhs - h0 * dp[..., j - 1]) / den
        m = np.zeros_like(y)
        for j in range(n - 2, 0, -1):
            m[..., j] = dp[..., j] - cp[..., j] * m[..., j + 1]
    return m


def ncdm_tables(h, T_cmb, m_ncdm, T_over, nodes, weights, dtype=LD):
    """cp_ncdm_tables: (n, nsp, 4, 119) -- rho, rho'', p, p'' on the species' knots -- from h, T_cmb (n,), m_ncdm, T_over (n, nsp) and a Gauss-Laguerre
    rule of any size: _compute_ncdm_momenta (cosmology.py:74-137) / (1 + z)^3 / h^2 (:441-442), the prefactors as ncdm_momenta_kernel groups them."""
    dtype = np.dtype(dtype).type
    h, T_cmb = (np.asarray(v, dtype='f8').astype(dtype)[:, None, None] for v in (h, T_cmb))
    m, T_over = (np.asarray(v, dtype='f8').astype(dtype)[:, :, None] for v in (m_ncdm, T_over))
    t, w = (np.asarray(v, dtype='f8').astype(dtype) for v in (nodes, weights))
    x = knots('ncdm')
    z = x.astype(dtype)
    with np.errstate(all='ignore'):
        T_eff = T_cmb * T_over
        a = 1. / (1. + z)
        over_T = ELECTRON_VOLT / (BOLTZMANN * (T_eff / a))
        m2 = ((m * over_T)**2)[..., None]
        e, f = np.sqrt(t**2 + m2), 1. + np.exp(-t)
        rho = np.sum(t**2 * e / f * w, axis=-1)                      # cosmology.py:59-60
        pr = np.sum(1. / 3. * t**4 / e / f * w, axis=-1)             # :65-66
        Ta = T_eff / a
        pref = 7. / 8. * 4 / dtype(C)**3 * STEFAN_BOLTZMANN * Ta**4
        norm = (7. * dtype(PI)**4 / 120.) * (1e10 * MSUN)
        zp1 = 1. + z
        scale = dtype(MPC)**3 / zp1**3 / (h * h)
        y_rho, y_p = pref * rho / norm * scale, pref * pr / norm * scale
    return np.stack([y_rho, second_derivatives(x, y_rho), y_p, second_derivatives(x, y_p)], axis=2)


def midpoint_values(tab):
    """The splines of the tables (..., 4, 119) at the midpoints of the species' knots, (..., 2, 118) in longdouble: a = b = 1 / 2 in spline_m_eval."""
    tab = np.asarray(tab).astype(LD)
    x = knots('ncdm').astype(LD)
    hh = np.diff(x)
    y, m = tab[..., 0::2, :], tab[..., 1::2, :]
    return 0.5 * (y[..., :-1] + y[..., 1:]) - 0.375 * (m[..., :-1] + m[..., 1:]) * (hh * hh) / 6.


# ---- the derived parameters ----------------------------------------------------------------------------------------------------------------------------

def derived_parameters(params, dtype=LD):
    """cp_derived_parameters: (17, n), the rows in the order of enum cp_derived_value (cosmology.py:355-397 as derived_parameters_kernel restates them)."""
    dtype = np.dtype(dtype).type
    p = np.asarray(params, dtype='f8').reshape(-1, NPARAMS).astype(dtype)
    h, Omega_cdm, Omega_b, Omega_k, T_cmb, N_ur = (p[:, i] for i in range(6))
    with np.errstate(all='ignore'):
        h2 = h * h
        c3 = dtype(C)**3
        Omega_g = (T_cmb * T_cmb) * (T_cmb * T_cmb) * 4. / c3 * STEFAN_BOLTZMANN / (h2 * RHO_CRIT_KG)
        T_ur = T_cmb * T_UR_OVER_CMB
        Omega_ur = N_ur * 7. / 8. * ((T_ur * T_ur) * (T_ur * T_ur)) * 4. / c3 * STEFAN_BOLTZMANN / (h2 * RHO_CRIT_KG)
        Omega_r, Omega_m = Omega_g + Omega_ur, Omega_b + Omega_cdm
        Omega_de = 1. - (Omega_cdm + Omega_b + Omega_g + Omega_ur + Omega_k)
        K = -(100. * 100.) / (dtype(C_KMS) * dtype(C_KMS)) * Omega_k
        return np.array([h2, h * 100, Omega_g, T_ur, Omega_ur, Omega_r, Omega_m, Omega_de, K, Omega_b * h2, Omega_cdm * h2, Omega_m * h2, Omega_g * h2,
                         Omega_ur * h2, Omega_r * h2, Omega_k * h2, Omega_de * h2])


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------------------

def pointwise_level(truth, f64):
    """(rows,): the largest relative distance of the float64 restatement from the truth in each row, floored at FLOOR.  NaN and zero entries must agree and
    do not count."""
    truth, f64 = np.asarray(truth), np.asarray(f64).astype(LD)
    assert truth.shape == f64.shape and np.array_equal(np.isnan(truth), np.isnan(f64)), 'the restatements disagree about NaN'
    skip = np.isnan(truth) | (np.abs(truth) < SMALLEST_NORMAL)
    assert (f64[truth == 0] == 0).all(), 'the restatements disagree about zeros'
    with np.errstate(all='ignore'):
        rel = np.where(skip, 0, np.abs(f64 - truth) / np.abs(truth))
    return np.maximum(np.asarray(rel.reshape(rel.shape[0], -1).max(axis=-1), dtype='f8'), FLOOR)


def block_level(truth, f64, top=None):
    """(top, level), each (rows,): the largest |truth| of each row (or ``top``) and the restatement's largest distance from the truth over it, floored."""
    truth, f64 = np.asarray(truth), np.asarray(f64).astype(LD)
    assert truth.shape == f64.shape and np.array_equal(np.isnan(truth), np.isnan(f64)), 'the restatements disagree about NaN'
    nan = np.isnan(truth)
    flat = lambda a: a.reshape(a.shape[0], -1)      # noqa: E731
    if top is None:
        top = flat(np.where(nan, 0, np.abs(truth))).max(axis=-1)
    dist = flat(np.where(nan, 0, np.abs(f64 - truth))).max(axis=-1)
    with np.errstate(all='ignore'):
        level = np.where(top > 0, dist / top, 0)
    return np.asarray(top).astype(LD), np.maximum(np.asarray(level, dtype='f8'), FLOOR)


def below_cap(truth, f64, rule='pointwise', top=None):
    """The largest level of the case in FLOORs; a case is used on the device while this is below CAP."""
    level = pointwise_level(truth, f64) if rule == 'pointwise' else block_level(truth, f64, top)[1]
    return float(level.max() / FLOOR)


def _report(what, fraction, level):
    worst = float(fraction.max()) if fraction.size else 0.
    print('%s: largest fraction of the allowance %.3g (level at most %.3g FLOOR)' % (what, worst, float(level.max() / FLOOR)))
    return worst


def assert_pointwise(dev, truth, f64, what='', extra=0., measure_only=False, cap=CAP):
    """Every entry of the device's rows within (ALLOW x the row's level + extra) of the truth, relative to the entry; NaN exactly where the truth has it and
    zero where it is zero.  Prints and returns the largest fraction of the allowance used (``measure_only``: without holding it to 1).  ``cap``: the
    cap of the case's levels in FLOORs (tests/power_truth.py: 64 for spectra, P ~ T^2)."""
    dev, truth = np.asarray(dev), np.asarray(truth)
    assert dev.shape == truth.shape, (what, dev.shape, truth.shape)
    level = pointwise_level(truth, f64)
    assert level.max() < cap * FLOOR, '{}: the case is over the cap ({:.3g} FLOOR)'.format(what, level.max() / FLOOR)
    assert np.array_equal(np.isnan(dev), np.isnan(truth)), '{}: NaN in other places than the truth has them'.format(what)
    nan = np.isnan(truth)
    assert np.isfinite(dev[~nan]).all(), what
    allowed = (ALLOW * level + extra).reshape((-1,) + (1,) * (truth.ndim - 1)) * np.abs(truth) + np.where(truth == 0, 0, SUBNORMAL_SPACING)
    subnormal = ~nan & (truth != 0) & (np.abs(truth) < SMALLEST_NORMAL)
    allowed = allowed + np.where(subnormal, ALLOW * np.abs(np.asarray(f64).astype(LD) - truth), 0)
    dist = np.where(nan, 0, np.abs(dev.astype(LD) - truth))
    with np.errstate(all='ignore'):
        fraction = np.where(nan, 0, np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0)))
    worst = _report(what, fraction, level)
    assert worst <= 1. or measure_only, '{}: entry {} at {:.3g} of its allowance'.format(what, np.unravel_index(np.argmax(fraction), fraction.shape), worst)
    return worst


def assert_blocks(dev, truth, f64, what='', top=None):
    """Every row of the device's result within ALLOW x its level of the truth, against the row's largest |truth| (or ``top`` (rows,)); NaN exactly where
    the truth has it.  Prints and returns the largest fraction of the allowance used."""
    dev, truth = np.asarray(dev), np.asarray(truth)
    assert dev.shape == truth.shape, (what, dev.shape, truth.shape)
    top, level = block_level(truth, f64, top)
    assert level.max() < CAP * FLOOR, '{}: the case is over the cap ({:.3g} FLOOR)'.format(what, level.max() / FLOOR)
    assert np.array_equal(np.isnan(dev), np.isnan(truth)), '{}: NaN in other places than the truth has them'.format(what)
    nan = np.isnan(truth)
    assert np.isfinite(dev[~nan]).all(), what
    dist = np.where(nan, 0, np.abs(dev.astype(LD) - truth)).reshape(truth.shape[0], -1).max(axis=-1)
    allowed = ALLOW * level * top
    with np.errstate(all='ignore'):
        fraction = np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0))
    worst = _report(what, fraction, level)
    assert worst <= 1., '{}: row {} at {:.3g} of its allowance'.format(what, int(np.argmax(fraction)), worst)
    return worst


# ---- the cases of the device tests (tests/test_background_truth_host.py holds them below the cap) ----------------------------------------------------

MIXES = ('lambda', 'fluid', 'alternating', 'closed', 'open')
SAMPLE_COUNTS = {1: (1, 1), 255: (3, 85), 256: (4, 64), 257: (1, 257), 513: (3, 171)}      # samples -> (ncosmo, nz) of the shared-z layout
SPECIES_SEED = 5


def cosmologies(n, mix, seed, nan_member=True):
    """(n, 8) float64: ordinary cosmologies, every one a cosmological constant ('lambda'), a fluid ('fluid') or alternately one and the other (the other
    mixes); flat, but for one closed member (Omega_k = -0.05: the sweeps that select, the walk above ``top``) or one open member (Omega_k = 0.05).  In a
    batch of more than one, ``nan_member`` gives member n // 2 a NaN for its h."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0.6, 0.8, n), rng.uniform(0.2, 0.3, n), rng.uniform(0.04, 0.06, n), np.zeros(n), rng.uniform(2.6, 2.8, n),
                  rng.uniform(2., 3.5, n), rng.uniform(-1.2, -0.8, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    lam = np.ones(n, dtype='?') if mix == 'lambda' else (np.zeros(n, dtype='?') if mix == 'fluid' else np.arange(n) % 2 == 0)
    p[lam, 6], p[lam, 7] = -1., 0.
    if mix == 'closed':
        p[min(5, n - 1), 3] = -0.05
    if mix == 'open':
        p[min(5, n - 1), 3] = 0.05
    if nan_member and n > 1:
        p[n // 2, 0] = np.nan
    return p


SCALAR_PARAMS = (4, 5)      # T_cmb and N_ur go as scalars (cp_param.ptr == NULL) in the calls that mix the two forms


def with_scalars(p, scalars=SCALAR_PARAMS):
    """p with the columns ``scalars`` set to their first entry: what the call computes when those parameters are passed as scalars."""
    p = p.copy()
    p[:, list(scalars)] = p[0, list(scalars)]
    return p


def species_inputs(n, nsp, seed=SPECIES_SEED, zero_mass=False):
    """(m_ncdm (n, nsp) in eV, log-uniform in [1e-4, 10]; T_ncdm_over_cmb (n, nsp)); ``zero_mass``: the last species of cosmology 0 has mass exactly 0."""
    rng = np.random.default_rng(seed + 1000 * nsp + n)
    m = 10.**rng.uniform(-4., 1., (n, nsp))
    if zero_mass:
        m[0, -1] = 0.
    return m, rng.uniform(0.68, 0.74, (n, nsp))


@functools.lru_cache(maxsize=None)
def laguerre(nq):
    t, w = np.polynomial.laguerre.laggauss(nq)
    return np.ascontiguousarray(t, dtype='f8'), np.ascontiguousarray(w, dtype='f8')


def species_tables(p, nsp, masses=(0.06, 0.1, 0.3)):
    """(n, nsp, 4, 119) float64: the tables the background tests hand to the entry points as INPUT -- the float64 restatement of cp_ncdm_tables for
    species of fixed masses (moderate ones: a cosmology stays a cosmology) at the cosmologies p, 100 Gauss-Laguerre nodes."""
    n = len(p)
    h, T = np.where(np.isnan(p[:, 0]), 0.7, p[:, 0]), p[:, 4]
    m = np.broadcast_to(np.asarray(masses[:nsp]), (n, nsp))
    return np.asarray(ncdm_tables(h, T, m, np.full((n, nsp), 0.71611), *laguerre(100), dtype='f8'), dtype='f8')


def distance_z():
    """The redshifts of the distance tests (:func:`edge_z` of the 119 knots).  Every interval is there: so are the first for which k + 1 + reach meets
    NK - 1 and the one below it."""
    return edge_z(knots('distance'))


def edge_z(zc):
    """Every knot, every interval midpoint, the neighbours of the first, second, second-to-last and last knot on both sides, 0 and the last knot exactly, a
    NaN, -1e-300 and one redshift above the grid."""
    mid = zc[:-1] + np.diff(zc) / 2
    near = np.concatenate([[np.nextafter(zc[i], -np.inf), np.nextafter(zc[i], np.inf)] for i in (0, 1, -2, -1)])
    return np.concatenate([zc, mid, near, [0., zc[-1], np.nan, -1e-300, 2. * zc[-1]]])


def tables_for(p, nsp):
    return species_tables(p, nsp) if nsp else None


@functools.lru_cache(maxsize=None)
def distance_configs(mix, nsp):
    """The batches of the distance tests for one mix of cosmologies and 0 or 2 massive species: for every count of samples of SAMPLE_COUNTS one with a
    redshift per cosmology (n, 1), all parameters as arrays, parameter 1 Omega_cdm, and one with shared redshifts (n / nz, nz), T_cmb and N_ur as scalars,
    parameter 1 Omega_m; then 8 cosmologies at the whole set of redshifts.  Each a dict: p (n, 8) as the call computes them, scalars, second_is_omega_m,
    z, z_shared, tab."""
    zset = distance_z()
    out = []
    for samples, (ncosmo, nz) in SAMPLE_COUNTS.items():
        seed = 100 * samples + 10 * MIXES.index(mix) + nsp
        p = cosmologies(samples, mix, seed)
        out.append(dict(p=p, scalars=(), second_is_omega_m=0, z=zset[(7 * samples + np.arange(samples)) % zset.size][:, None], z_shared=0, tab=tables_for(p, nsp)))
        p = with_scalars(cosmologies(ncosmo, mix, seed + 1))
        out.append(dict(p=p, scalars=SCALAR_PARAMS, second_is_omega_m=1, z=zset[(11 * samples + 3 * np.arange(nz)) % zset.size], z_shared=1, tab=tables_for(p, nsp)))
    p = cosmologies(8, mix, 77 + nsp)
    out.append(dict(p=p, scalars=(), second_is_omega_m=0, z=zset, z_shared=1, tab=tables_for(p, nsp)))
    return out


def config_truth(config, what, dtype=LD, **kwargs):
    """``what(c, z, ...)`` of a config in ``dtype``."""
    c = cosmo(config['p'], config['second_is_omega_m'], config['tab'], dtype=dtype)
    return what(c, config['z'], **kwargs)


@functools.lru_cache(maxsize=None)
def time_configs(nsp):
    """ncosmo 1 and 65 at the whole set of redshifts of the 400 knots (shared; 65: scalars mixed in, parameter 1 Omega_m), 257 with four redshifts each."""
    zset = edge_z(knots('time'))
    out = []
    for n in (1, 65, 257):
        p = cosmologies(n, 'closed', 300 + n + nsp)
        if n == 65:
            p = with_scalars(p)
        z = zset[(4 * np.arange(n)[:, None] + np.arange(4)) % zset.size] if n == 257 else zset
        out.append(dict(p=p, scalars=SCALAR_PARAMS if n == 65 else (), second_is_omega_m=int(n == 65), z=z, z_shared=int(n != 257), tab=tables_for(p, nsp)))
    return out


# -0.5: outside the species' knots.  The cosmological constants of the mix (even members) go through all of these in turn, the fluids (odd members)
# through all but 9999: a fluid's (1 + z)^(3 (w0 + wa)) there carries the rounding of its exponent times log(1 + z), 66 FLOORs at worst, which no
# restatement in float64 keeps below the cap
ELEMENTWISE_Z = np.array([0., 1e-3, 9999., 0.5, np.nan, -0.5, 1100., 3., 100., 10., 1.])
ELEMENTWISE_Z_FLUID = ELEMENTWISE_Z[ELEMENTWISE_Z != 9999.]
ELEMENTWISE_SEED = 400
ELEMENTWISE_KINDS = [(k, False) for k in PLAIN_KINDS + DENSITY_KINDS] + [(k, True) for k in DENSITY_KINDS]


@functools.lru_cache(maxsize=None)
def elementwise_config(nsp):
    """257 cosmologies (the 'closed' mix with an open member as well), one redshift each."""
    n = 257
    p = cosmologies(n, 'closed', ELEMENTWISE_SEED + nsp)
    p[7, 3] = 0.05
    i = np.arange(n)
    z = np.where(i % 2 == 0, ELEMENTWISE_Z[(i // 2) % ELEMENTWISE_Z.size], ELEMENTWISE_Z_FLUID[(i // 2) % ELEMENTWISE_Z_FLUID.size])
    return dict(p=p, scalars=(), second_is_omega_m=0, z=z[:, None], z_shared=0,
                tab=species_tables(p, nsp) if nsp else None)


RS_Z = (1059.94, 10., 2000.)


@functools.lru_cache(maxsize=None)
def rs_configs(nsp):
    """(1, 1), a cosmological constant; (3, 2) with shared redshifts, fluids; (3, 2) with a redshift per sample, z = 0 among them (the rule misses its 1e-7
    there: NaN), cosmological constants around the member with the NaN."""
    out = []
    for n, z, shared in ((1, np.array([RS_Z[0]]), 1), (3, np.array([RS_Z[1], RS_Z[2]]), 1), (3, np.array([[RS_Z[0], 0.], [RS_Z[1], RS_Z[2]], [0., RS_Z[0]]]), 0)):
        p = cosmologies(n, 'fluid' if shared and n > 1 else 'alternating', 500 + n + nsp + shared)
        if shared and n > 1:
            p = with_scalars(p)
        out.append(dict(p=p, scalars=SCALAR_PARAMS if shared and n > 1 else (), second_is_omega_m=int(shared), z=z, z_shared=shared, tab=tables_for(p, nsp)))
    return out


GROWTH_COUNTS = (1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def growth_config(n, nsp):
    p = cosmologies(n, 'alternating', 600 + n + nsp)
    scalars = SCALAR_PARAMS if n % 2 == 0 else ()
    if scalars:
        p = with_scalars(p)
    return dict(p=p, scalars=scalars, second_is_omega_m=n % 2, tab=tables_for(p, nsp))


def growth_truth(config, mass, dtype=LD):
    """(n, 2, 201) as cp_growth_ode_tables lays it out."""
    D, f = growth_tables(cosmo(config['p'], config['second_is_omega_m'], config['tab'], dtype=dtype), mass)
    return np.stack([D, f], axis=1)


NCDM_SHAPES = ((1, 1, 100), (1, 8, 1), (2, 3, 128), (32, 1, 2), (33, 1, 100), (65, 2, 7))      # (ncosmo, nsp, nq)


@functools.lru_cache(maxsize=None)
def ncdm_config(ncosmo, nsp, nq):
    """h, T_cmb (ncosmo,), m, T_over (ncosmo, nsp) as the call computes them; which of them go as scalars; the rule.  In a batch of more than one,
    member ncosmo // 2 (``nan_member``) has a NaN: its h where h goes as an array (all its species' tables are NaN), else the mass of its species 0 (that
    species' tables are)."""
    index = NCDM_SHAPES.index((ncosmo, nsp, nq))
    rng = np.random.default_rng(700 + index)
    h, T_cmb = rng.uniform(0.6, 0.8, ncosmo), rng.uniform(2.6, 2.8, ncosmo)
    m, T_over = species_inputs(ncosmo, nsp, zero_mass=True)
    scalar = dict(h=index % 2 == 1, T_cmb=index % 3 == 1, T_over=index % 2 == 0, m=False)
    if scalar['h']:
        h[:] = h[0]
    if scalar['T_cmb']:
        T_cmb[:] = T_cmb[0]
    if scalar['T_over']:
        T_over[:] = T_over[0]
    nan_member = ncosmo // 2 if ncosmo > 1 else None
    if nan_member is not None:
        if scalar['h']:
            m[nan_member, 0] = np.nan
        else:
            h[nan_member] = np.nan
    nodes, weights = laguerre(nq)
    return dict(h=h, T_cmb=T_cmb, m=m, T_over=T_over, scalar=scalar, nodes=nodes, weights=weights, nan_member=nan_member)


def ncdm_without_nan(config):
    """The config with its NaN made an ordinary value."""
    clean = dict(config, h=np.where(np.isnan(config['h']), 0.7, config['h']), m=np.where(np.isnan(config['m']), 0.2, config['m']))
    return clean


def ncdm_truth(config, dtype=LD):
    return ncdm_tables(config['h'], config['T_cmb'], config['m'], config['T_over'], config['nodes'], config['weights'], dtype=dtype)


DERIVED_COUNTS = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def derived_config(n):
    p = cosmologies(n, 'closed', 800 + n)
    if n > 7:
        p[7, 3] = 0.05
    scalars = SCALAR_PARAMS if n % 2 == 0 else ()
    return dict(p=with_scalars(p) if scalars else p, scalars=scalars)


RADIAL_COUNTS = (1, 255, 257, 1048576, 1048577)
RADIAL_K = (5e-9, 0., -5e-9)
RADIAL_KINDS = ('angular_diameter_distance', 'comoving_transverse_distance', 'luminosity_distance')


@functools.lru_cache(maxsize=None)
def radial_config(n):
    """(chi, z): radial distances in (0, 1e4) Mpc/h and redshifts in (0, 10), a zero and a NaN among the distances and a NaN among the redshifts."""
    rng = np.random.default_rng(900 + n % 1000)
    chi, z = rng.uniform(0., 1e4, n), rng.uniform(0., 10., n)
    chi[n // 2] = 0.
    if n > 2:
        chi[n // 3], z[n - 1] = np.nan, np.nan
    return chi, z
