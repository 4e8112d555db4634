"""GPU: the kernels of csrc/cp_background.hip through the C ABI against tests/background_truth.py (numpy longdouble; the rule of that module's
docstring: ALLOW = 16 levels of the float64 restatement, plus the 1e-14 of the truncated backward elimination for the four distance kinds), at the
smallest shapes that cross each boundary of a launch:

  bg_kernel, distances  1, 255, 256, 257 and 513 samples, a redshift per cosmology and shared redshifts (85 and 171 of them: no divisor of the 256
                        samples of a workgroup); every knot, every interval midpoint (so every interval, and with it every value of k + 1 + reach on both
                        sides of NK - 1), the neighbours of the end knots, NaN, -1e-300, above the grid; waves of cosmological constants, of fluids, of
                        both, with a closed member (the sweeps that select, the walk above ``top``), with an open one; 0 and 2 massive species
  bg_kernel<NK_TIME>    time at the same kind of redshifts on the 400 knots, and age, for 1, 65 and 257 cosmologies, 0 and 1 species
  elementwise kinds     every kind and every legal CP_BG_AS_FRACTION combination at 257 samples, species -1, 0 and 2 of 3; the illegal ones refused
  rs_kernel             (1, 1), (3, 2) shared and per cosmology, both kinds, with z = 0 where the rule misses its 1e-7: NaN
  cp_growth_ode_tables  1, 63, 64, 65, 129 cosmologies, mass 0 and 1, 0 and 2 species
  cp_ncdm_tables        (ncosmo, nsp, nq) with 64 and 66 spline lanes and momenta blocks that end inside a row, at a species and at a cosmology border
  cp_derived_parameters 1, 255, 256, 257 cosmologies
  cp_distance_from_radial  1, 255, 257, 2^20 and 2^20 + 1 samples (the last takes the grid-stride loop), K > 0, = 0, < 0: the three kinds under every K
                        up to 257 samples, one kind per K at the two large sizes (angular with K > 0, transverse with K = 0, luminosity with K < 0).  The
                        library accepts the comoving transverse distance here (it is one of the three derived kinds); the radial distance and every
                        other kind are refused

Every output stands between sentinels, every input is compared with what was uploaded, every call is made twice (the same bits), parameters go as
arrays and as scalars, parameter 1 as Omega_cdm and as Omega_m, and every batch of more than one cosmology, those of cp_ncdm_tables included, holds a
cosmology with a NaN parameter: the others keep the bits of the batch without it.  (cp_distance_from_radial has one cosmology; NaN is among its samples.)
In the elementwise kinds the fluids see every redshift of the list but 9999 (tests/background_truth.py: ELEMENTWISE_Z); rs is compared for cosmological
constants and for fluids.

Largest fraction of the allowance used, as measured on an MI355X (printed by the tests; the largest level of a case was 28.5 FLOOR):
  distances 0.0625 with the documented 1e-14 and 0.402 WITHOUT it (measured beside the assertion, not asserted): the truncated backward elimination
  fits ALLOW x level alone, the 1e-14 is not needed; time and age 0.353; elementwise kinds 0.444; rs 0.172; growth tables 0.671; species tables 0.246
  (values against the largest entry and pointwise, splines at the midpoints); derived parameters 0.239; distances from the radial distance 0.0645.
"""
import ctypes
import functools

import numpy as np
import pytest

import background_truth as bt

pytestmark = pytest.mark.gpu
LD, F8 = np.longdouble, np.float64
GUARD = 32
SENTINEL = -7.25e77
FILL = 123.
CP_OK, CP_EINVAL, CP_EUNSUPPORTED = 0, 1, 2


class Guarded(object):
    """A float64 array on the device between two runs of sentinels."""

    def __init__(self, array):
        import torch
        self.before = np.ascontiguousarray(array, dtype='f8').copy()
        self.shape, self.size = self.before.shape, self.before.size
        self.buffer = torch.full((self.size + 2 * GUARD,), SENTINEL, dtype=torch.float64, device='cuda:0')
        self.buffer[GUARD:GUARD + self.size] = torch.as_tensor(self.before.reshape(-1), device='cuda:0')

    def ptr(self):
        return self.buffer.data_ptr() + GUARD * self.buffer.element_size()

    def host(self):
        whole = self.buffer.cpu().numpy()
        assert (whole[:GUARD] == SENTINEL).all() and (whole[GUARD + self.size:] == SENTINEL).all(), 'a sentinel was overwritten'
        return whole[GUARD:GUARD + self.size].reshape(self.shape).copy()

    def untouched(self):
        return same_bits(self.host(), self.before)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module', autouse=True)
def lib():
    import torch
    assert torch.cuda.is_available()
    from cosmoprimo_amd import _lib
    _lib.background_init(0)
    return _lib.load()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def synchronize():
    """Wait for the device; an error of the device ends the session (nothing more is started on a device that has faulted)."""
    import torch
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit('the device reported an error: {}'.format(exc), returncode=3)


def param_array(columns, scalars):
    """(array of cp_param, the Guarded inputs): column i of ``columns`` (n, ncol) as a device array, or as a scalar where i is in ``scalars``."""
    from cosmoprimo_amd import _lib
    columns = np.asarray(columns, dtype='f8')
    carr = (_lib.cp_param * columns.shape[1])()
    guards = []
    for i in range(columns.shape[1]):
        if i in scalars:
            assert same_bits(columns[:, i], np.full(len(columns), columns[0, i]))
            carr[i] = _lib.cp_param(None, float(columns[0, i]))
        else:
            guards.append(Guarded(columns[:, i]))
            carr[i] = _lib.cp_param(guards[-1].ptr(), 0.)
    return carr, guards


def species_struct(tab, species=-1):
    from cosmoprimo_amd import _lib
    if tab is None:
        return None, []
    g = Guarded(tab)
    return _lib.cp_ncdm(tab.shape[1], species, g.ptr()), [g]


def call_twice(once):
    first, second = once(), once()
    assert all(same_bits(a, b) for a, b in zip(first, second)), 'two calls differ'
    return first


def evaluate(lib, config, kind, species=-1, fraction=False, status=CP_OK):
    """cp_background_eval of a config of tests/background_truth.py: (ncosmo, nz) float64."""
    p, z = config['p'], np.asarray(config['z'], dtype='f8')
    ncosmo, nz = len(p), z.shape[-1]
    code = bt.KINDS[kind] | (bt.AS_FRACTION if fraction else 0)

    def once():
        carr, inputs = param_array(p, config['scalars'])
        cn, more = species_struct(config['tab'], species)
        zin, out = Guarded(z), Guarded(np.full((ncosmo, nz), FILL))
        got = lib.cp_background_eval(ncosmo, nz, ctypes.cast(carr, ctypes.c_void_p), config['second_is_omega_m'], ctypes.byref(cn) if cn is not None else None,
                                     zin.ptr(), config['z_shared'], out.ptr(), code, 0, stream())
        synchronize()
        assert got == status, (kind, fraction, got, lib.cp_last_error())
        assert all(g.untouched() for g in inputs + more + [zin]), 'an input was written'
        return (out.host(),)

    out = call_twice(once)[0]
    if status != CP_OK:
        assert (out == FILL).all(), 'a refused call wrote'
    return out


def without_nan(config):
    """(the config with its NaN member made ordinary, the member) -- None for a batch of one."""
    bad = np.flatnonzero(np.isnan(config['p'][:, 0]))
    if not bad.size:
        return None, None
    p = config['p'].copy()
    p[bad, 0] = 0.7
    return dict(config, p=p), bad


def others_keep_their_bits(lib, config, dev, run):
    """The members of the batch other than the one with the NaN have the bits of the batch without it."""
    clean, bad = without_nan(config)
    if clean is None:
        assert len(config['p']) == 1
        return
    keep = np.ones(len(config['p']), dtype='?')
    keep[bad] = False
    assert same_bits(run(clean)[keep], dev[keep]), 'a NaN reached its neighbours'


WORST = {}


def note(family, fraction):
    WORST[family] = max(WORST.get(family, 0.), fraction)
    print('%s: largest fraction so far %.3g' % (family, WORST[family]))


# ---- distances -------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def distance_truths(mix, nsp):
    return [(bt.config_truth(cfg, bt.distances), bt.config_truth(cfg, bt.distances, dtype=F8)) for cfg in bt.distance_configs(mix, nsp)]


@pytest.mark.parametrize('nsp', [0, 2])
@pytest.mark.parametrize('mix', bt.MIXES)
def test_distances(lib, mix, nsp):
    configs = bt.distance_configs(mix, nsp)
    for index, (cfg, (ld, f8)) in enumerate(zip(configs, distance_truths(mix, nsp))):
        for kind in (bt.DISTANCE_KINDS if index == len(configs) - 1 else bt.DISTANCE_KINDS[:1]):
            what = '%s, %s, %d species, %d cosmologies x %d redshifts (%s)' % (kind, mix, nsp, len(cfg['p']), np.shape(cfg['z'])[-1], 'shared' if cfg['z_shared'] else 'own')
            dev = evaluate(lib, cfg, kind)
            shape = dev.shape
            note('distances', bt.assert_pointwise(dev, ld[kind].reshape(shape), f8[kind].reshape(shape), what, extra=bt.DISTANCE_EXTRA))
            note('distances, extra = 0 (not asserted)', bt.assert_pointwise(dev, ld[kind].reshape(shape), f8[kind].reshape(shape), what + ', extra = 0', measure_only=True))
            if kind == bt.DISTANCE_KINDS[0]:
                others_keep_their_bits(lib, cfg, dev, lambda clean: evaluate(lib, clean, kind))


# ---- time and age ----------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def time_truths(nsp):
    return [(bt.config_truth(cfg, bt.time), bt.config_truth(cfg, bt.time, dtype=F8)) for cfg in bt.time_configs(nsp)]


@pytest.mark.parametrize('nsp', [0, 1])
def test_time_and_age(lib, nsp):
    for cfg, ((tl, al), (t8, a8)) in zip(bt.time_configs(nsp), time_truths(nsp)):
        what = '%d cosmologies, %d species' % (len(cfg['p']), nsp)
        dev = evaluate(lib, cfg, 'time')
        note('time', bt.assert_blocks(dev, tl, t8, 'time, ' + what, top=al))
        others_keep_their_bits(lib, cfg, dev, lambda clean: evaluate(lib, clean, 'time'))
        one = dict(cfg, z=np.zeros((len(cfg['p']), 1)), z_shared=0)      # age: z is not read for its value
        note('time', bt.assert_pointwise(evaluate(lib, one, 'age'), al[:, None], a8[:, None], 'age, ' + what))


# ---- the elementwise kinds -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nsp', [0, 3])
def test_elementwise(lib, nsp):
    cfg = bt.elementwise_config(nsp)
    for kind, fraction in bt.ELEMENTWISE_KINDS:
        for species in ((-1, 0, nsp - 1) if kind in ('rho_ncdm', 'p_ncdm') and nsp else (-1,)):
            ld, f8 = (bt.config_truth(cfg, bt.elementwise, dtype=dtype, kind=(kind, fraction), species=species) for dtype in (LD, F8))
            dev = evaluate(lib, cfg, kind, species, fraction)
            note('elementwise', bt.assert_pointwise(dev, ld, f8, '%s%s, species %d of %d' % (kind, ' / rho_crit' if fraction else '', species, nsp)))
            if kind in ('efunc', 'rho_m', 'rho_ncdm'):
                others_keep_their_bits(lib, cfg, dev, lambda clean: evaluate(lib, clean, kind, species, fraction))
    for kind in bt.FRACTION_ILLEGAL:
        evaluate(lib, cfg, kind, fraction=True, status=CP_EINVAL)


def test_eval_refuses_a_species_out_of_range(lib):
    cfg = bt.elementwise_config(3)
    for species in (-2, 3):
        evaluate(lib, cfg, 'rho_ncdm', species, status=CP_EINVAL)


# ---- the sound horizon -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nsp', [0, 1])
def test_rs(lib, nsp):
    for cfg in bt.rs_configs(nsp):
        for kind, cosmomc in (('rs', False), ('rs_cosmomc', True)):
            ld, f8 = (bt.config_truth(cfg, bt.rs, dtype=dtype, cosmomc=cosmomc)[0] for dtype in (LD, F8))
            dev = evaluate(lib, cfg, kind)
            what = '%s, %d cosmologies, %s redshifts, %d species' % (kind, len(cfg['p']), 'shared' if cfg['z_shared'] else 'own', nsp)
            note('rs', bt.assert_pointwise(dev.reshape(-1, 1), ld.reshape(-1, 1), f8.reshape(-1, 1), what))
            others_keep_their_bits(lib, cfg, dev, lambda clean: evaluate(lib, clean, kind))
            if not cfg['z_shared']:      # z = 0: the reference's rule misses its 1e-7
                assert np.isnan(dev[0, 1]) and np.isnan(dev[2, 0]) and np.isfinite(dev[0, 0]) and np.isfinite(dev[2, 1])


# ---- the growth ODE --------------------------------------------------------------------------------------------------------------------------------------

def growth_tables(lib, cfg, mass, status=CP_OK):
    n = len(cfg['p'])

    def once():
        carr, inputs = param_array(cfg['p'], cfg['scalars'])
        cn, more = species_struct(cfg['tab'])
        out = Guarded(np.full((n, 2, bt.NK_GROWTH), FILL))
        got = lib.cp_growth_ode_tables(n, ctypes.cast(carr, ctypes.c_void_p), cfg['second_is_omega_m'], ctypes.byref(cn) if cn is not None else None, mass,
                                       out.ptr(), 0, stream())
        synchronize()
        assert got == status, lib.cp_last_error()
        assert all(g.untouched() for g in inputs + more), 'an input was written'
        return (out.host(),)

    return call_twice(once)[0]


@pytest.mark.parametrize('nsp', [0, 2])
@pytest.mark.parametrize('n', bt.GROWTH_COUNTS)
def test_growth_ode_tables(lib, n, nsp):
    cfg = bt.growth_config(n, nsp)
    for mass in (0, 1):
        ld, f8 = (bt.growth_truth(cfg, mass, dtype).reshape(-1, bt.NK_GROWTH) for dtype in (LD, F8))
        dev = growth_tables(lib, cfg, mass)
        note('growth', bt.assert_blocks(dev.reshape(-1, bt.NK_GROWTH), ld, f8, 'growth, %d cosmologies, mass %d, %d species' % (n, mass, nsp)))
        others_keep_their_bits(lib, cfg, dev, lambda clean: growth_tables(lib, clean, mass))
    assert (growth_tables(lib, cfg, 2, status=CP_EINVAL) == FILL).all()


# ---- the species' tables ---------------------------------------------------------------------------------------------------------------------------------

def ncdm_tables(lib, cfg, nsp=None, nq=None, status=CP_OK):
    from cosmoprimo_amd import _lib
    ncosmo, real = cfg['m'].shape
    nsp = real if nsp is None else nsp
    nq = cfg['nodes'].size if nq is None else nq
    nodes, weights = (np.ascontiguousarray(np.resize(v, max(nq, 1))) for v in (cfg['nodes'], cfg['weights']))

    def once():
        scalar = cfg['scalar']
        (ch, cT), inputs = param_array(np.stack([cfg['h'], cfg['T_cmb']], axis=1), [i for i, k in enumerate(('h', 'T_cmb')) if scalar[k]])
        cm, more = param_array(np.resize(cfg['m'], (ncosmo, nsp)) if nsp != real else cfg['m'], ())
        ct, more2 = param_array(np.resize(cfg['T_over'], (ncosmo, nsp)) if nsp != real else cfg['T_over'], range(nsp) if scalar['T_over'] and nsp == real else ())
        out = Guarded(np.full((ncosmo, nsp, 4, bt.NK_NCDM), FILL))
        before = nodes.copy(), weights.copy()
        got = lib.cp_ncdm_tables(ncosmo, nsp, ch, cT, ctypes.cast(cm, ctypes.c_void_p), ctypes.cast(ct, ctypes.c_void_p), nq, _lib.as_double_p(nodes),
                                 _lib.as_double_p(weights), out.ptr(), 0, stream())
        synchronize()
        assert got == status, (got, lib.cp_last_error())
        assert all(g.untouched() for g in inputs + more + more2) and same_bits(nodes, before[0]) and same_bits(weights, before[1]), 'an input was written'
        return (out.host(),)

    return call_twice(once)[0]


@pytest.mark.parametrize('shape', bt.NCDM_SHAPES)
def test_ncdm_tables(lib, shape):
    cfg = bt.ncdm_config(*shape)
    masses = cfg['m'][~np.isnan(cfg['m'])]
    assert (masses == 0).sum() == 1 and masses.max() <= 10. and np.append(masses[masses > 0], 1.).min() >= 1e-4
    ld, f8 = bt.ncdm_truth(cfg), bt.ncdm_truth(cfg, F8)
    dev = ncdm_tables(lib, cfg)
    assert dev.shape == ld.shape and np.array_equal(np.isnan(dev), np.isnan(ld)) and np.isfinite(dev[~np.isnan(ld)]).all()
    if cfg['nan_member'] is None:
        assert shape[0] == 1 and np.isfinite(dev).all()
    else:
        # the member with the NaN: NaN in its own tables (all of them, or those of its species 0: natural ends stay 0) and nowhere else, and every other
        # table has the bits of the batch without it
        hit = np.zeros(dev.shape[:2], dtype='?')
        hit[cfg['nan_member'], slice(None) if np.isnan(cfg['h']).any() else 0] = True
        assert np.array_equal(np.isnan(dev).any(axis=(2, 3)), hit) and np.isnan(dev[hit][:, 0::2]).all() and np.isnan(dev[hit][:, 1::2, 1:-1]).all()
        clean = ncdm_tables(lib, bt.ncdm_without_nan(cfg))
        assert np.isfinite(clean).all() and same_bits(clean[~hit], dev[~hit]), 'a NaN reached its neighbours'
    what = 'species tables %s' % (shape,)
    rows = lambda t: t[..., 0::2, :].reshape(-1, bt.NK_NCDM)      # noqa: E731
    note('ncdm tables', bt.assert_blocks(rows(dev), rows(ld), rows(f8), what + ', values against the largest entry'))
    note('ncdm tables', bt.assert_pointwise(rows(dev), rows(ld), rows(f8), what + ', values pointwise'))
    # the second derivatives by their consequence (the module's docstring): the splines at the midpoints of the knots
    mid = lambda t: bt.midpoint_values(t).reshape(-1, bt.NK_NCDM - 1)      # noqa: E731
    note('ncdm tables', bt.assert_pointwise(np.asarray(mid(dev), dtype='f8'), mid(ld), mid(f8), what + ', splines at the midpoints'))
    assert (dev[..., 1::2, 0] == 0).all() and (dev[..., 1::2, -1] == 0).all()      # natural ends


def test_ncdm_tables_refusals(lib):
    cfg = bt.ncdm_config(2, 3, 128)
    for kwargs, status in ((dict(nsp=9), CP_EUNSUPPORTED), (dict(nq=0), CP_EINVAL), (dict(nq=129), CP_EINVAL)):
        assert (ncdm_tables(lib, cfg, status=status, **kwargs) == FILL).all()


# ---- the derived parameters ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n', bt.DERIVED_COUNTS)
def test_derived_parameters(lib, n):
    cfg = bt.derived_config(n)

    def run(config):
        def once():
            carr, inputs = param_array(config['p'], config['scalars'])
            out = Guarded(np.full((bt.DERIVED_NVALUES, n), FILL))
            assert lib.cp_derived_parameters(n, ctypes.cast(carr, ctypes.c_void_p), out.ptr(), 0, stream()) == CP_OK, lib.cp_last_error()
            synchronize()
            assert all(g.untouched() for g in inputs), 'an input was written'
            return (out.host(),)
        return call_twice(once)[0]

    dev = run(cfg)
    ld, f8 = bt.derived_parameters(cfg['p']), bt.derived_parameters(cfg['p'], F8)
    note('derived', bt.assert_pointwise(dev.T, ld.T, f8.T, 'derived parameters, %d cosmologies' % n))      # every row of (17, n) whole: no FILL left
    others_keep_their_bits(lib, cfg, dev.T, lambda clean: run(clean).T)


# ---- the derived distances of a catalogue ----------------------------------------------------------------------------------------------------------------

def from_radial(lib, chi, z, K, kind, status=CP_OK):
    def once():
        a, b, out = Guarded(chi), Guarded(z), Guarded(np.full(chi.shape, FILL))
        got = lib.cp_distance_from_radial(a.ptr(), b.ptr(), chi.size, K, bt.KINDS[kind], out.ptr(), 0, stream())
        synchronize()
        assert got == status, lib.cp_last_error()
        assert a.untouched() and b.untouched(), 'an input was written'
        return (out.host(),)
    return call_twice(once)[0]


@pytest.mark.parametrize('n', bt.RADIAL_COUNTS)
def test_distance_from_radial(lib, n):
    chi, z = bt.radial_config(n)
    for i, K in enumerate(bt.RADIAL_K):
        for kind in (bt.RADIAL_KINDS if n < 1000 else bt.RADIAL_KINDS[i:i + 1]):
            dev = from_radial(lib, chi, z, K, kind)
            ld, f8 = bt.from_radial(chi, z, K, kind), bt.from_radial(chi, z, K, kind, F8)
            note('from_radial', bt.assert_pointwise(dev[None], ld[None], f8[None], '%s from the radial distance, n = %d, K = %g' % (kind, n, K)))
            assert dev[n // 2] == 0. and (n < 3 or (np.isnan(dev[n // 3]) and np.isnan(dev[n - 1])))
    for kind in ('comoving_radial_distance', 'efunc'):
        assert (from_radial(lib, chi, z, 0., kind, status=CP_EINVAL) == FILL).all()
