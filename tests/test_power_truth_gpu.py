"""GPU: the kernels of csrc/cp_power.hip and csrc/cp_power_eval.h through ``cosmoprimo_amd.power`` (``analytic``, ``eh_scalars``, ``variants_scalars``,
``variants``) against tests/power_truth.py (numpy longdouble; the rule of that module's docstring: ALLOW = 16 levels of the float64 restatement, plus
the figures that cp_power_eval.h states for its short forms -- 1e-14 for EH98, 1e-15 for the no-wiggle form, twice that for spectra, nothing for BBKS, the
primordial spectrum, the scalars and the variants --, a row one (cosmology, decade of k) block), at the smallest shapes that cross each boundary of a
launch.  The three engines x transfer, primordial, matter, log_k_matter, unless stated:

  coefficients_kernel   1, 63, 64, 65 cosmologies (one lane each, 64 per workgroup); T_cmb, N_ur, n_s, k_pivot as scalars and the rest as arrays in one
                        launch; parameter 1 as Omega_m; non-zero alpha_s, beta_s, a k_pivot that is not the default (every case has those)
  power_kernel, 256     3 cosmologies x 1, 255, 256, 257 wavenumbers; 1024 x 1100: 768 wavenumbers per workgroup in three passes, two workgroups per
                        cosmology, a partial last pass and a partial last workgroup -- truth on 24 members, the first and the last among them, and every
                        member finite and bit-equal to itself in a batch of 24 (256 wavenumbers per workgroup there)
  power_kernel, 64      3071 (the last batch of 256 threads) and 3072 cosmologies x 64, 65, 341 wavenumbers, truth on 32 members (0, 1, 63, 64, the last)
  redshifts             matter at 1, 256, 257 redshifts (3 x 70) and at 64, 65 (3072 x 65): the second block of both shapes; from 0 to 10, not sorted
  kscale                factors in [0.9, 1.1] at 3 x 257 and at 3071 / 3072 x 341
  massive species       1 and 3, float64 tables of tests/background_truth.py as input, parameter 1 as Omega_cdm and as Omega_m: BBKS transfer, matter
                        with redshifts, log_k_matter; EH98 matter with redshifts
  wavenumbers           geomspace(1e-8, 1e2); linspace(7e-5, 7, 4096); 3e3 to 3e5 h/Mpc (k rs_drag across 1e6: sin_bounded hands over to the library's
                        sine); subnormal and smallest-normal k (log_tab_any's out-of-line branch), the transfer functions only
  variants_kernel       matter, transfer x delta_m, delta_cb x 0, 1, 3 species at (ncosmo, nk, nz) = (1, 1, 1), (3, 256, 257), (3, 257, 256), (1, 257, 1)
                        and, for 0 and 3 species, (1024, 1100, 2) with truth on 24 members
  eh_scalars_kernel, variants_scalars_kernel   1, 255, 256, 257 cosmologies, 0 and 3 species, every scalar of the two enums

Measured on an MI355X (printed by the tests as MEASURED lines): per engine and quantity the largest level of the float64 restatement over the cases, in
floors of 1.1e-16, the largest fraction of the allowance the device used, and -- measured beside the assertion, not asserted -- the same fraction with
the header's figure left out (extra = 0):

  engine                  quantity       level   fraction   with extra = 0
  eisenstein_hu           transfer        26.6     0.121        0.415
  eisenstein_hu           primordial      14.3     0.243
  eisenstein_hu           matter          53.7     0.120        0.293
  eisenstein_hu           log_k_matter    28.0     0.197        0.963
  eisenstein_hu_nowiggle  transfer        12.7     0.172        0.208
  eisenstein_hu_nowiggle  primordial      14.3     0.243
  eisenstein_hu_nowiggle  matter          37.2     0.153        0.217
  eisenstein_hu_nowiggle  log_k_matter    22.4     0.630        0.889
  bbks                    transfer         8.4     0.227
  bbks                    primordial      14.3     0.243
  bbks                    matter          25.5     0.238
  bbks                    log_k_matter    19.2     0.946
  variants                transfer        20.9     0.147
  variants                matter          52.5     0.129
  cp_eh_scalars           every scalar    11.1     0.474
  cp_variants_scalars     every scalar     5.8     0.302

The short forms fit ALLOW x level alone: no figure of cp_power_eval.h is contradicted, and none had to be corrected.  log_k_matter comes closest to its
allowance (the pre-kernel batches of 64 and 65 cosmologies) where log(k P) crosses zero: the kernel adds four terms of size 15 to 40, each with an ulp of
1.8e-15 to 7e-15, and is held there to 16 levels of max(1, |truth|) = 1: 1.8e-15 for a row at the floor.  No wrong result was found in the kernels.
"""
import numpy as np
import pytest

import background_truth as bt
import power_truth as pt

pytestmark = pytest.mark.gpu
F8 = np.float64


@pytest.fixture(scope='module', autouse=True)
def device():
    import torch
    assert torch.cuda.is_available()
    from cosmoprimo_amd import _lib
    _lib.background_init(0)
    return torch.device('cuda', 0)


def on_device(step):
    """step(), then the device is waited for; an error of the device ends the session (nothing more is started on a device that has faulted)."""
    import torch
    try:
        out = step()
        torch.cuda.synchronize()
        return out
    except RuntimeError as exc:
        pytest.exit('the device reported an error: {}'.format(exc), returncode=3)


def host(tensor):
    return on_device(lambda: tensor.cpu().numpy())


def all_finite(tensor):
    import torch
    return on_device(lambda: bool(torch.isfinite(tensor).all()))


def species(tab):
    """The float64 tables (n, nsp, 4, 119) of tests/background_truth.py as the ``bg['ncdm']`` of a call: an input, uploaded as it is."""
    import torch
    from cosmoprimo_amd.background import NcdmTables
    if tab is None:
        return None
    tables = NcdmTables([], [], ncosmo=tab.shape[0], device='cuda:0')
    tables.nspecies = tab.shape[1]
    tables.tab = torch.as_tensor(np.ascontiguousarray(tab, dtype='f8'), device='cuda:0')
    return tables


def arguments(case, members=None, second_is_omega_m=None):
    """(bg, pk, Omega_m, ncdm, kscale) of the members of a case: the columns the case names go as scalars, the others as arrays."""
    sel = slice(None) if members is None else members
    p, pk = case['p'][sel], case['pk'][sel]
    bg = {name: (float(p[0, i]) if i in case['bg_scalars'] else np.ascontiguousarray(p[:, i])) for i, name in enumerate(bt.PARAMS)}
    pk = {name: (float(pk[0, i]) if i in case['pk_scalars'] else np.ascontiguousarray(pk[:, i])) for i, name in enumerate(pt.PK_PARAMS)}
    som = case['second_is_omega_m'] if second_is_omega_m is None else second_is_omega_m
    Omega_m = bg.pop('Omega_cdm') if som else None
    return bg, pk, Omega_m, species(None if case['tab'] is None else case['tab'][sel]), None if case['kscale'] is None else case['kscale'][sel]


def analytic(case, engine, what, members=None):
    """``power.analytic`` of the whole batch of a case (or of its ``members`` as a batch of their own): the device tensor (n, nk) or (n, nz, nk)."""
    from cosmoprimo_amd import power as pw
    bg, pk, Omega_m, ncdm, kscale = arguments(case, members)
    if ncdm is not None:
        bg['ncdm'] = ncdm
    return pw.analytic(engine, what, case['k'], z=case['z'] if what == 'matter' else None, bg=bg, pk=pk, Omega_m=Omega_m, kscale=kscale)


def rows_of(case, out):
    """The members of the batch that are compared with the truth, on the host; the whole batch must be finite."""
    import torch
    n = case['ncosmo']
    assert out.shape[0] == n
    if len(case['rows']) == n:
        dev = host(out)
    else:
        dev = host(out[torch.as_tensor(case['rows'], device=out.device)])
        assert all_finite(out), case['name']
    return dev


WORST = {}


def note(key, fraction, level):
    f, lv = WORST.get(key, (0., 0.))
    WORST[key] = (max(f, fraction), max(lv, level))
    print('MEASURED %-70s level at most %5.1f FLOOR, largest fraction of the allowance %.3f' % ((' '.join(key),) + WORST[key][::-1]))


@pytest.mark.parametrize('index', range(len(pt.analytic_cases())))
def test_analytic(index):
    case = pt.analytic_cases()[index]
    for engine in case['engines']:
        x = pt.case_x(case) if engine == 'bbks' else None
        for what in case['whats']:
            dev = rows_of(case, analytic(case, engine, what))
            truth, f64 = pt.case_truth(case, engine, what), pt.case_truth(case, engine, what, F8)
            assert dev.shape == truth.shape
            note((engine, what), *pt.assert_quantity(engine, what, case['k'], dev, truth, f64, x, name=case['name']))
            if pt.extra_of(engine, what):      # what the short forms use of ALLOW x level alone: a figure, not asserted
                note((engine, what, 'with extra = 0 (not asserted)'), *pt.assert_quantity(engine, what, case['k'], dev, truth, f64, x, name=case['name'] + ', extra = 0',
                                                                                         extra=0., measure_only=True))


@pytest.mark.parametrize('engine', pt.ENGINES)
def test_every_member_of_the_large_batch_has_the_bits_of_a_batch_of_24(engine):
    """1024 cosmologies x 1100 wavenumbers (768 per workgroup, two workgroups per cosmology) against the same cosmologies 24 at a time (256 per workgroup,
    five workgroups): the same arithmetic per (cosmology, k), whichever lane of whichever pass evaluates it."""
    import torch
    case = [c for c in pt.analytic_cases() if c['name'].startswith('kiter > 1')][0]
    n = case['ncosmo']
    assert pt.launch_shape(24, case['nk'])['kspan'] == 256 and pt.launch_shape(n, case['nk'])['kspan'] == 768
    for what in pt.WHATS:
        whole = on_device(lambda: analytic(case, engine, what))
        assert all_finite(whole)
        parts = on_device(lambda: torch.cat([analytic(case, engine, what, np.arange(start, min(start + 24, n))) for start in range(0, n, 24)]))
        assert on_device(lambda: torch.equal(whole, parts)), (engine, what)


@pytest.mark.parametrize('nsp,index', [(nsp, index) for nsp in (0, 1, 3) for index in range(len(pt.VARIANTS_SHAPES) + (nsp != 1))])
def test_variants(nsp, index):
    from cosmoprimo_amd import power as pw
    case = pt.variants_cases(nsp)[index]      # (the large batch, the last case, is run without species and with three)
    bg, pk, _, ncdm, _ = arguments(case)
    for what in case['whats']:
        for of in ('delta_m', 'delta_cb'):
            dev = rows_of(case, pw.variants(what, case['k'], case['z'], of=of, bg=bg, pk=pk, ncdm=ncdm))
            truth, f64 = pt.variants_truth(case, what, of), pt.variants_truth(case, what, of, F8)
            assert dev.shape == truth.shape
            note(('variants', what), *pt.assert_quantity('variants', what, case['k'], dev, truth, f64, name='%s, %s' % (case['name'], of)))


@pytest.mark.parametrize('nsp', [0, 3])
@pytest.mark.parametrize('n', pt.SCALAR_COUNTS)
def test_scalars(n, nsp):
    from cosmoprimo_amd import power as pw
    from cosmoprimo_amd import _lib
    assert _lib.EH_SCALARS == pt.EH_SCALARS and _lib.VARIANTS_SCALARS == pt.VARIANTS_SCALARS
    case = pt.scalars_case(n, nsp)
    weights = pt.scalars_truth(case, 'eh', parts=True)
    for which, names in (('eh', pt.EH_SCALARS), ('variants', pt.VARIANTS_SCALARS)):
        bg, _, Omega_m, ncdm, _ = arguments(case, second_is_omega_m=None if which == 'eh' else 0)
        if which == 'eh':
            got = pw.eh_scalars(bg=dict(bg, ncdm=ncdm), Omega_m=Omega_m)
        else:
            got = pw.variants_scalars(bg=bg, ncdm=ncdm)
        assert tuple(got) == names
        dev = {name: host(v) for name, v in got.items()}
        assert all(v.shape == (n,) for v in dev.values())
        truth, f64 = pt.scalars_truth(case, which), pt.scalars_truth(case, which, F8)
        d, t, f = pt.prepared_scalars(names, dev, truth, f64, weights)
        what = 'cp_%s_scalars, %d cosmologies, %d species' % (which, n, nsp)
        note((which, 'scalars'), bt.assert_pointwise(d, t, f, what), float(bt.pointwise_level(t, f).max() / bt.FLOOR))
