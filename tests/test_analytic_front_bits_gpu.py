"""GPU: the results of the analytic-spectrum entry points, bit for bit, against tests/golden/analytic_front_bits.npz -- what the library gave through its
Python wrappers before these entry points were put behind one shared front (recorded on an MI355X by tools/gen_analytic_front_bits.py, every call made
twice there and refused if its two runs differed).  That change touched no kernel, and the kernels use no atomics and sum in a fixed order, so every
output must be EQUAL: a tolerance would not see a dispatch that runs the kernel of one engine on the coefficients of another, a grid one workgroup short,
or tables of the wavenumbers read from the wrong place in the workspace.

The file holds the inputs too (``in.*``: cosmologies drawn with a fixed seed from the ranges of tests/test_corners_gpu.py: normal_cosmologies, growth
factors, neutrino masses).  What the host code steers and the shapes that cross it: the three engines; parameters as per-cosmology arrays and as
broadcast values (h alone an array, so that the call is still a batch); with and without one massive species; ``second_is_omega_m`` where the wrapper
has it (``Omega_m=`` of power.analytic and power.eh_scalars); batches of 1, 2 and 5 (alone, one pair, an odd tail); sigma(r, z) through the functional
with 1 and 4 radii, the fused kernel prefiltered and plain, and two blocks on two streams; 1027 cosmologies for the transform that evaluates its spectra
and the whole wallish2018 filter, 2051 for the fused sigma(r, z) (on 256 CUs the first sizes at which every workgroup takes two rounds of pairs and the
stagger of the sigma kernel switches on; their first two and last three rows are kept).  Rows of 4096 coefficients are kept as every 128th entry,
spectra of 1024 likewise.  One flat float64 array per group and the names and shapes of its entries, as tests/test_emulator_front_bits_gpu.py."""
import os
import types

import numpy as np
import pytest

from test_emulator_front_bits_gpu import assert_equal_bits, flatten  # noqa: F401  (flatten: for the generator)

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'analytic_front_bits.npz')
ENGINES = ['eisenstein_hu', 'eisenstein_hu_nowiggle', 'bbks']
BG_NAMES = ['h', 'Omega_cdm', 'Omega_b', 'Omega_k', 'T_cmb', 'N_ur', 'w0_fld', 'wa_fld']
SIZES = (1, 2, 5)
# (size, parameters as arrays or broadcast, one massive species)
CASES = [(n, form, ncdm) for n in SIZES for form, ncdm in (('arrays', False), ('broadcast', True))] + [(5, 'arrays', True), (5, 'broadcast', False)]
LARGE_DST, LARGE_SIGMA, KEPT = 1027, 2051, [0, 1, -3, -2, -1]
K = np.geomspace(1e-4, 10., 8)
Z = np.array([0., 1.5])
RADII = {'one': np.array([8.]), 'four': np.array([2., 8., 12., 30.]), 'many': np.geomspace(1., 60., 8)}
T_NCDM_OVER_CMB = 0.71611


def draw_inputs():
    """What the generator stores as ``in.*``: 5 cosmologies for the small batches (a batch of n takes the first n), LARGE_SIGMA values of h, Omega_cdm,
    Omega_b for the large ones (ranges of tests/test_corners_gpu.py: normal_cosmologies, 'mixed' and safe)."""
    rng = np.random.default_rng(20261019)
    n = max(SIZES)
    small = np.stack([rng.uniform(0.6, 0.8, n), rng.uniform(0.2, 0.3, n), rng.uniform(0.04, 0.06, n), rng.uniform(0., 0.05, n), rng.uniform(2.6, 2.8, n),
                      rng.uniform(2., 3.5, n), rng.uniform(-1.2, -0.8, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    small[::2, 6], small[::2, 7] = -1., 0.
    return {'in.bg': small, 'in.A_s': rng.uniform(1.5e-9, 2.5e-9, n), 'in.n_s': rng.uniform(0.9, 1., n), 'in.m_ncdm': rng.uniform(0.05, 0.15, n),
            'in.growth_sq': rng.uniform(0.3, 1., (n, 2)), 'in.sigma8': rng.uniform(0.7, 0.9, n),
            'in.large': np.stack([rng.uniform(0.6, 0.8, LARGE_SIGMA), rng.uniform(0.2, 0.3, LARGE_SIGMA), rng.uniform(0.04, 0.06, LARGE_SIGMA)], axis=1),
            'in.large_growth_sq': rng.uniform(0.3, 1., (LARGE_SIGMA, 2))}


def _device():
    import torch
    return torch.device('cuda', 0)


def _host(x, rows=None):
    """float64 numpy of a device tensor (int32 boxes are exact in it); ``rows``: keep these rows."""
    a = np.asarray(x.cpu().numpy(), dtype='f8')
    return np.ascontiguousarray(a if rows is None else a[rows])


def parameters(inputs, n, form, ncdm):
    """(bg, pk, tables or None) of a batch of the first ``n`` stored cosmologies."""
    from cosmoprimo_amd import background as bgm
    table = inputs['in.bg'][:n]
    if form == 'arrays':
        bg = {name: table[:, i].copy() for i, name in enumerate(BG_NAMES)}
        pk = dict(A_s=inputs['in.A_s'][:n].copy(), n_s=inputs['in.n_s'][:n].copy())
        m = inputs['in.m_ncdm'][:n].copy()
    else:
        bg = {name: float(table[0, i]) for i, name in enumerate(BG_NAMES)}
        bg['h'] = table[:, 0].copy()
        pk = dict(A_s=float(inputs['in.A_s'][0]), n_s=float(inputs['in.n_s'][0]))
        m = float(inputs['in.m_ncdm'][0])
    tables = None
    if ncdm:
        T = np.full(n, T_NCDM_OVER_CMB) if form == 'arrays' else T_NCDM_OVER_CMB
        tables = bgm.NcdmTables([m], [T], h=bg['h'], T_cmb=bg['T_cmb'], ncosmo=n, device=_device())
    return bg, pk, tables


def wallish_filter():
    """A wallish2018 filter that has not run: its plans for the default wavenumbers, for ``_full`` (cp_wallish_full) on rows set by the caller."""
    from cosmoprimo_amd.bao_filter import Wallish2018PowerSpectrumBAOFilter
    f = Wallish2018PowerSpectrumBAOFilter.__new__(Wallish2018PowerSpectrumBAOFilter)
    f.pk_interpolator = types.SimpleNamespace(extrap_kmin=1e-7, extrap_kmax=1e2)
    f.device, f.k = _device(), np.geomspace(1e-7, 1e2, 1024)
    f._operators()
    return f


def _sigma_routes(engine, bg, pk, growth_sq, rows=None, few=True):
    """sigma_rz_analytic by its routes: {label: array}."""
    from cosmoprimo_amd import interpolator as itp
    dev, out = _device(), {}
    routes = [('prefiltered', 'many', True, 0), ('plain', 'many', False, 0)]
    if few:
        routes = [('functional1', 'one', True, 0), ('functional4', 'four', True, 0)] + routes + [('blocks2', 'many', True, 2)]
    saved = itp._SIGMA_RZ_PREFILTERED
    try:
        for label, radii, prefiltered, blocks in routes:
            itp._SIGMA_RZ_PREFILTERED = prefiltered
            sigma, spectra, _ = itp.sigma_rz_analytic(engine, bg, pk, RADII[radii], growth_sq, dev, blocks=blocks, keep_spectra=True)
            out['sigma_' + label], out['sigma_' + label + '_pk'] = _host(sigma, rows), _host(spectra[:, ::128], rows)
    finally:
        itp._SIGMA_RZ_PREFILTERED = saved
    return out


def _transform_routes(f, engine, bg, pk, rows=None, layouts=True):
    """DST.forward_analytic plain, split and with the boxes, and the whole filter: {label: array}."""
    from cosmoprimo_amd import power as pw
    dst, out = f._operators()['dst'], {}
    if layouts:
        out['dst_plain'] = _host(dst.forward_analytic(engine, bg, pk)[:, ::128], rows)
        out['dst_split'] = _host(dst.forward_analytic(engine, bg, pk, split=True)[:, ::128], rows)
    coefficients, boxes = dst.forward_analytic(engine, bg, pk, split=True, box=(f._margin_first, f._margin_second, f._offset[0], f._offset[1]))
    out['dst_box'], out['dst_box_boxes'] = _host(coefficients[:, ::128], rows), _host(boxes.view(-1, 4), rows)
    f._pk_rows = pw.analytic(engine, 'matter', f.k, bg=bg, pk=pk, device=_device())
    assert f._full(engine, bg, pk, dst)
    out['wallish_full'], out['wallish_full_boxes'] = _host(f._pknow_rows[:, ::128], rows), np.stack([_host(box, rows) for box in f._boxes], axis=-1)
    return out


def engine_entries(inputs, engine, f):
    """Every entry that takes an engine, over CASES."""
    import torch
    from cosmoprimo_amd import power as pw, interpolator as itp
    dev, out = _device(), {}
    for n, form, ncdm in CASES:
        bg, pk, tables = parameters(inputs, n, form, ncdm)
        if tables is not None:
            bg['ncdm'] = tables
        tag = '%d.%s.%s.' % (n, form, 'ncdm' if ncdm else 'massless')
        Omega_m = bg['Omega_cdm'] + bg['Omega_b']
        out[tag + 'matter'] = _host(pw.analytic(engine, 'matter', K, z=Z, bg=bg, pk=pk, device=dev))
        out[tag + 'matter_omega_m'] = _host(pw.analytic(engine, 'matter', K, z=Z, bg=bg, pk=pk, Omega_m=Omega_m, device=dev))
        out[tag + 'transfer_kscale'] = _host(pw.analytic(engine, 'transfer', K, bg=bg, pk=pk, device=dev, kscale=1. + 0.01 * np.arange(n)))
        out[tag + 'log_k_matter'] = _host(pw.analytic(engine, 'log_k_matter', K, bg=bg, pk=pk, device=dev))
        growth_sq = torch.as_tensor(inputs['in.growth_sq'][:n], device=dev)
        for name, value in _sigma_routes(engine, bg, pk, growth_sq).items():
            out[tag + name] = value
        target = torch.as_tensor(inputs['in.sigma8'][:n], device=dev) if form == 'arrays' else float(inputs['in.sigma8'][0])
        rs, amplitude, spectra, _ = itp.sigma8_normalise(engine, bg, pk, target, dev)
        out[tag + 'sigma8_rs'], out[tag + 'sigma8_amplitude'], out[tag + 'sigma8_pk'] = _host(rs), _host(amplitude), _host(spectra[:, ::128])
        for name, value in _transform_routes(f, engine, bg, pk).items():
            out[tag + name] = value
    return out


def common_entries(inputs):
    """The entries without an engine argument: cp_eh_scalars, cp_variants_scalars, cp_power_eval_variants."""
    from cosmoprimo_amd import _lib, power as pw
    dev, out = _device(), {}
    for n, form, ncdm in CASES + [(1, 'scalars', False)]:
        bg, pk, tables = parameters(inputs, n, 'arrays' if form == 'scalars' else form, ncdm)
        if form == 'scalars':      # one cosmology that is no batch
            bg, pk = {name: float(v[0]) for name, v in bg.items()}, {name: float(v[0]) for name, v in pk.items()}
        tag = '%d.%s.%s.' % (n, form, 'ncdm' if ncdm else 'massless')
        with_tables = dict(bg, ncdm=tables) if tables is not None else bg
        for label, Omega_m in (('eh_scalars', None), ('eh_scalars_omega_m', bg['Omega_cdm'] + bg['Omega_b'])):
            scalars = pw.eh_scalars(bg=with_tables, Omega_m=Omega_m, device=dev)
            out[tag + label] = np.stack([_host(scalars[name]) for name in _lib.EH_SCALARS], axis=-1)
        scalars = pw.variants_scalars(bg=bg, ncdm=tables, device=dev)
        out[tag + 'variants_scalars'] = np.stack([_host(scalars[name]) for name in _lib.VARIANTS_SCALARS], axis=-1)
        for what, of in (('matter', 'delta_m'), ('transfer', 'delta_cb')):
            out[tag + 'variants_%s_%s' % (what, of)] = _host(pw.variants(what, K, Z, of=of, bg=bg, pk=pk, ncdm=tables, device=dev))
    return out


def large_entries(inputs, f):
    """1027 cosmologies through the transform that evaluates its spectra and through the whole filter, 2051 through the fused sigma(r, z), plain and
    prefiltered: two rounds of pairs per workgroup on 256 CUs.  Rows KEPT."""
    import torch
    out = {}
    for n, label in ((LARGE_DST, 'dst'), (LARGE_SIGMA, 'sigma')):
        table = inputs['in.large'][:n]
        bg, pk = dict(h=table[:, 0].copy(), Omega_cdm=table[:, 1].copy(), Omega_b=table[:, 2].copy()), dict(n_s=0.96)
        if label == 'dst':
            found = _transform_routes(f, 'eisenstein_hu', bg, pk, rows=KEPT, layouts=False)
        else:
            found = _sigma_routes('eisenstein_hu', bg, pk, torch.as_tensor(inputs['in.large_growth_sq'][:n], device=_device()), rows=KEPT, few=False)
        for name, value in found.items():
            out['%d.%s' % (n, name)] = value
    return out


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


@pytest.fixture(scope='module')
def wallish():
    return wallish_filter()


@pytest.mark.parametrize('engine', ENGINES)
def test_engine_entries(recorded, wallish, engine):
    assert_equal_bits(engine_entries(recorded, engine, wallish), recorded, engine)


def test_entries_without_engine(recorded):
    assert_equal_bits(common_entries(recorded), recorded, 'common')


def test_large_batches(recorded, wallish):
    assert_equal_bits(large_entries(recorded, wallish), recorded, 'large')
