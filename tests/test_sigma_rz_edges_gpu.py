"""GPU: the kernels of csrc/cp_sigma.hip that form their spectra themselves -- sigma_rz_kernel<E, false> (cp_sigma_rz_analytic's one-kernel route, the band
operator), sigma_rz_kernel<E, true> (cp_sigma_rz_analytic_prefiltered), sigma_functional_kernel (cp_sigma_rz_functional) and sigma8_normalise_kernel
(cp_sigma8_normalise) -- against the longdouble truth of tests/sigma_truth.py through the C ABI: spectra of tests/power_truth.py without growth on
geomspace(1e-7, 1e2, 1024), the tap transform of tests/fftlog_taps_truth.py, band weights / radii of the test's making, growth_sq and d_functional random
inputs.  tests/test_sigma_truth_host.py holds the levels of these cases below the cap.  sigma(r, z): ALLOW = 16 levels of the float64 restatement (float64
spectra, the pair packed into one transform as the kernel packs it, the float64 tail) per (cosmology, radius) block over the redshifts, + half the spectrum's
extra + 1e-16 for the root; pk_out: power_truth's per-decade rule with 1e-15 more for the geometric stepping of k inside the fused kernel.

  fused, both forms   (nq, nz) over the three store paths and their seams: nz 1, 2, 3, 64, 66, 128, 256, 258, 7 x nq 1, 127, 128, 129, 257; 1, 2, 3 cosmologies
                      and a second trip of the grid with an odd count (the staggered start); pk_out given and null; a NaN cosmology in slot a, in slot b
                      and last of an odd batch; guards behind out and pk_out; the largest 2 nq + 2 nz of the LDS bound, one more refused
                      both forms once with the tables of the package's own TophatVariance plan, the truth through longdouble FFTs (fractions 0.084, 0.079)
  functional          nq 1 ... 4, nz 1, 2, 63, 64, 65, nk 1, 63, 64, 65, 1024, 1030, 1, 3, 4, 5, 257 cosmologies, a NaN cosmology in each wave of a block; nq = 5 refused
  sigma8_normalise    1, 4, 5, 257 cosmologies, scalar and per-cosmology targets, amplitude and pk_out given and null, nk != 1024 refused, a NaN cosmology

Found here: with the level of the spectra at the tabulated wavenumbers and the 1e-15 that the comment over evaluate_spectrum stated for the geometric stepping of k,
most cases of the band form failed at up to 8 allowances and pk_out of BBKS at 1.7.  The float64 restatement of the stepping (sigma_truth.stepped_k) puts P 2.0e-14
from its truth for k > 7.6 h/Mpc; the level of the fused kernel takes that restatement too, and the comment now states it.
Largest fraction of the allowance measured on the MI355X: sigma_rz_kernel 0.116 (band), 0.111 (prefiltered), its pk_out 0.067; sigma_functional_kernel 0.198,
pk_out 0.129; sigma8_normalise_kernel 0.076 (rsigma8), 0.174 (amplitude), 0.178 (pk_out).
"""
import ctypes

import numpy as np
import pytest

import background_truth as bt
import power_truth as pt
import sigma_truth as sg
from sigma_device import CANARY, LDS_FFT, FftPlan, GeoPlan, synchronized

pytestmark = pytest.mark.gpu

GUARD = 1024
WORST = {}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


@pytest.fixture(scope='module')
def basis(env):
    torch, _lib, lib, dev, stream = env
    out = np.zeros(16)
    _lib.check(lib.cp_geospline_basis(ctypes.c_double(sg.RHO), _lib.as_double_p(out)))
    return out.reshape(4, 4)


def note(kernel, fraction):
    WORST[kernel] = max(WORST.get(kernel, 0.), fraction)
    print('MEASURED %-34s largest fraction of the allowance so far %.3f' % (kernel, WORST[kernel]))
    return fraction


class Launch(object):
    """The arguments every entry point shares: the packed cosmologies, the wavenumbers, growth_sq, the workspace, guarded outputs."""

    def __init__(self, env, case, k, nq, nz, pk_out=True):
        torch, _lib, lib, dev, stream = env
        from cosmoprimo_amd import _device as dv
        _lib.background_init(dev.index)
        self.env, self.case = env, case
        p, pk = case['p'], case['pk']
        self.n = len(p)
        bg = {name: np.ascontiguousarray(p[:, i]) for i, name in enumerate(bt.PARAMS)}
        pkd = {name: np.ascontiguousarray(pk[:, i]) for i, name in enumerate(pt.PK_PARAMS)}
        args, n, self.keep = dv.pack_cosmologies(bg, pkd, dev, ncosmo=self.n)
        assert n == self.n
        self.args = args()
        self.engine = _lib.ENGINES[case['engine']]
        self.nk, self.nq, self.nz = len(k), nq, nz
        self.k = torch.as_tensor(np.ascontiguousarray(k, dtype='f8'), device=dev)
        self.growth = torch.as_tensor(np.ascontiguousarray(case['growth']), device=dev) if 'growth' in case else None
        self.out = torch.full((self.n * nq * nz + GUARD,), CANARY, dtype=torch.float64, device=dev)
        self.pk_out = torch.full((self.n * self.nk + GUARD,), CANARY, dtype=torch.float64, device=dev) if pk_out else None
        self.work = torch.empty(max(int(lib.cp_sigma_rz_workspace_bytes(self.n, self.nk)), 8), dtype=torch.uint8, device=dev)

    def pk_ptr(self):
        return None if self.pk_out is None else self.pk_out.data_ptr()

    def read(self, tensor, shape):
        host = synchronized(self.env[0], tensor)
        count = int(np.prod(shape))
        assert (host[count:] == CANARY).all(), 'the guard behind the output was written'
        got = host[:count].reshape(shape)
        assert not (got == CANARY).any(), '{:d} output elements were not written'.format(int((got == CANARY).sum()))
        return got

    def sigma(self):
        return self.read(self.out, (self.n, self.nq, self.nz))

    def spectra(self):
        return self.read(self.pk_out, (self.n, self.nk))


def run_fused(env, case, pk_out, basis=None):
    """The fused kernel of the case's form; returns (sigma, spectra or None)."""
    torch, _lib, lib, dev, stream = env
    from cosmoprimo_amd.spline import LinearOperator
    nq, nz = case['true'].shape[1:]
    L = Launch(env, case, sg.K, nq, nz, pk_out)
    if case['form'] == 'band':
        op = LinearOperator.dense(case['w'], device=dev)
        with FftPlan(env, case['syn']) as fft:
            assert lib.cp_sigma_rz_fused_available(fft.handle, op._handle) == 1
            _lib.check(lib.cp_sigma_rz_analytic(L.engine, *L.args, L.nk, L.k.data_ptr(), fft.handle, op._handle, L.growth.data_ptr(), nz, L.out.data_ptr(), L.pk_ptr(),
                                                L.work.data_ptr(), 0, dev.index, stream))
            return L.sigma(), (L.spectra() if pk_out else None)
    with GeoPlan(env, case['r'], case['syn']) as plan:
        _lib.check(lib.cp_sigma_rz_analytic_prefiltered(L.engine, *L.args, L.nk, L.k.data_ptr(), plan.handle, L.growth.data_ptr(), nz, L.out.data_ptr(), L.pk_ptr(),
                                                        L.work.data_ptr(), dev.index, stream))
        return L.sigma(), (L.spectra() if pk_out else None)


def hold_fused(env, case, pk_out, basis, what):
    engine, form = case['engine'], case['form']
    got, spectra = run_fused(env, case, pk_out, basis)
    kernel = 'sigma_rz_kernel<%s>' % ('true' if form == 'prefiltered' else 'false')
    assert note(kernel, sg.rz_fraction(got, case, sg.sigma_extra(engine, True), what)) <= 1.
    if pk_out:
        assert note(kernel + ' pk_out', sg.pk_fraction(spectra, case, sg.pk_extra(engine, True), what + ', pk_out', cap=np.inf)) <= 1.


@pytest.mark.parametrize('index', range(len(sg.rz_cases())))
def test_fused(env, basis, index):
    engine, form, nq, nz, ncosmo, nan, pk_out = sg.rz_cases()[index]
    case = sg.rz_case(engine, form, nq, nz, ncosmo, basis, nan)
    hold_fused(env, case, pk_out, basis, '%s, %s, %d radii x %d redshifts, %d cosmologies, NaN %s' % (engine, form, nq, nz, ncosmo, nan))


@pytest.mark.parametrize('form', ['band', 'prefiltered'])
def test_fused_second_trip(env, basis, form):
    """More pairs than one trip of the grid (the workgroups of a CU start two sleeps apart), an odd count, a NaN cosmology first and last."""
    torch, dev = env[0], env[3]
    ncosmo = torch.cuda.get_device_properties(dev).multi_processor_count * 4 * 2 + 3
    case = sg.rz_case('eisenstein_hu', form, 129, 3, ncosmo, basis, (0, ncosmo - 1))
    hold_fused(env, case, True, basis, '%s, second trip, %d cosmologies' % (form, ncosmo))


@pytest.mark.parametrize('form', ['band', 'prefiltered'])
def test_fused_lds_bound(env, basis, form):
    """34960 + 16 (nq + nz) bytes against the 160 KiB of a workgroup: nq + nz = 8055 runs and is held, 8056 is refused with nothing written."""
    torch, _lib, lib, dev, stream = env
    from cosmoprimo_amd.spline import LinearOperator
    most = (160 * 1024 - LDS_FFT) // 16
    nq = 8000 if form == 'band' else 512
    nz = most - nq
    case = sg.rz_case('eisenstein_hu_nowiggle', form, nq, nz, 2, basis)
    assert float(case['level_plain'].max()) < sg.CAP * sg.FLOOR
    hold_fused(env, case, False, basis, '%s, %d radii x %d redshifts (the LDS bound)' % (form, nq, nz))
    over = dict(case, growth=sg.rz_growth(2, nz + 1))
    L = Launch(env, over, sg.K, nq, nz + 1, False)
    if form == 'band':
        op = LinearOperator.dense(case['w'], device=dev)
        with FftPlan(env, case['syn']) as fft:
            status = lib.cp_sigma_rz_analytic(L.engine, *L.args, L.nk, L.k.data_ptr(), fft.handle, op._handle, L.growth.data_ptr(), nz + 1, L.out.data_ptr(), None,
                                              L.work.data_ptr(), 0, dev.index, stream)
    else:
        with GeoPlan(env, case['r'], case['syn']) as plan:
            status = lib.cp_sigma_rz_analytic_prefiltered(L.engine, *L.args, L.nk, L.k.data_ptr(), plan.handle, L.growth.data_ptr(), nz + 1, L.out.data_ptr(), None,
                                                          L.work.data_ptr(), dev.index, stream)
    assert status == _lib.CP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((L.out == CANARY).all())


# ---- the functional kernels ----------------------------------------------------------------------------------------------------------------------
def run_functional(env, case, pk_out, nq=None):
    torch, _lib, lib, dev, stream = env
    nq = case['true'].shape[1] if nq is None else nq
    nz = case['true'].shape[2]
    L = Launch(env, case, case['k'], nq, nz, pk_out)
    functional = torch.as_tensor(np.ascontiguousarray(case['functional']), device=dev)
    status = lib.cp_sigma_rz_functional(L.engine, *L.args, L.nk, L.k.data_ptr(), functional.data_ptr(), nq, L.growth.data_ptr(), nz, L.out.data_ptr(), L.pk_ptr(),
                                        L.work.data_ptr(), dev.index, stream)
    return L, status


@pytest.mark.parametrize('index', range(len(sg.functional_cases())))
def test_functional(env, index):
    torch, _lib, lib, dev, stream = env
    engine, nq, nz, nk, ncosmo, nan, pk_out = sg.functional_cases()[index]
    case = sg.functional_case(engine, nq, nz, nk, ncosmo, nan)
    L, status = run_functional(env, case, pk_out)
    _lib.check(status)
    what = '%s, %d radii x %d redshifts, %d wavenumbers, %d cosmologies, NaN %s' % (engine, nq, nz, nk, ncosmo, nan)
    assert note('sigma_functional_kernel', sg.rz_fraction(L.sigma(), case, sg.sigma_extra(engine, False), what)) <= 1.
    if pk_out:
        assert note('sigma_functional_kernel pk_out', sg.pk_fraction(L.spectra(), case, sg.pk_extra(engine, False), what + ', pk_out')) <= 1.


def test_functional_refuses_five_radii(env):
    torch, _lib, lib, dev, stream = env
    case = sg.functional_case('bbks', 4, 2, 64, 3)
    case = dict(case, functional=np.concatenate([case['functional'], case['functional'][:1]]))
    L, status = run_functional(env, case, False, nq=5)
    assert status == _lib.CP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((L.out == CANARY).all())


def pointwise(name, dev, true, f64, extra, what):
    """Entry by entry, relative to the entry: ALLOW levels of the float64 restatement + extra (background_truth.assert_pointwise)."""
    keep = ~np.isnan(np.asarray(true).reshape(len(true), -1)[:, 0])
    assert np.isnan(np.asarray(dev)[~keep]).all(), what
    shape = (int(keep.sum()), -1)
    return bt.assert_pointwise(np.asarray(dev)[keep].reshape(shape), np.asarray(true)[keep].reshape(shape), np.asarray(f64)[keep].reshape(shape),
                               '%s, %s' % (name, what), extra=extra)


@pytest.mark.parametrize('ncosmo,per_cosmology,amplitude,pk_out,nan', [(1, False, True, True, ()), (4, True, False, True, ()), (5, False, True, False, (3,)),
                                                                       (257, True, True, True, (256,)), (5, True, False, False, ())])
@pytest.mark.parametrize('engine', pt.ENGINES)
def test_sigma8_normalise(env, engine, ncosmo, per_cosmology, amplitude, pk_out, nan):
    torch, _lib, lib, dev, stream = env
    case = sg.normalise_case(engine, ncosmo, per_cosmology, nan)
    L = Launch(env, case, sg.K, 1, 1, pk_out)
    functional = torch.as_tensor(np.ascontiguousarray(case['functional']), device=dev)
    target = _lib.cp_param()
    held = torch.as_tensor(case['target'], device=dev)
    if per_cosmology:
        target.ptr, target.value = held.data_ptr(), 0.
    else:
        target.ptr, target.value = None, float(case['target'][0])
    rs = torch.full((ncosmo + GUARD,), CANARY, dtype=torch.float64, device=dev)
    amp = torch.full((ncosmo + GUARD,), CANARY, dtype=torch.float64, device=dev) if amplitude else None
    _lib.check(lib.cp_sigma8_normalise(L.engine, *L.args, L.nk, L.k.data_ptr(), functional.data_ptr(), target, rs.data_ptr(), amp.data_ptr() if amplitude else None,
                                       L.pk_ptr(), L.work.data_ptr(), dev.index, stream))
    what = '%s, %d cosmologies, %s target' % (engine, ncosmo, 'per-cosmology' if per_cosmology else 'scalar')
    true, f64 = case['norm_true'], case['norm_f64']
    extra = sg.pk_extra(engine, False)      # rs ~ 1 / sqrt(sum F P): half the spectrum's extra; A_s rs^2: all of it; P rs^2: twice
    assert note('sigma8_normalise_kernel rsigma8', pointwise('rsigma8', L.read(rs, (ncosmo,)), true['rsigma8'], f64['rsigma8'], extra / 2., what)) <= 1.
    if amplitude:
        assert note('sigma8_normalise_kernel amplitude', pointwise('amplitude', L.read(amp, (ncosmo,)), true['amplitude'], f64['amplitude'], extra, what)) <= 1.
    if pk_out:
        keep = np.array([i not in nan for i in range(ncosmo)])
        got = L.spectra()
        assert np.isnan(got[~keep]).all()
        x = None if case['x'] is None else case['x'][keep]
        d, t, f = pt.prepared(engine, 'matter', sg.K, got[keep], true['pk_out'][keep], f64['pk_out'][keep], x)
        assert note('sigma8_normalise_kernel pk_out', bt.assert_pointwise(d, t, f, 'pk_out, ' + what, extra=2. * extra, cap=pt.cap_of('matter'))) <= 1.


def test_sigma8_normalise_refuses_other_grids(env):
    torch, _lib, lib, dev, stream = env
    case = sg.functional_case('eisenstein_hu', 1, 1, 1030, 3)
    L = Launch(env, case, case['k'], 1, 1, False)
    functional = torch.as_tensor(np.ascontiguousarray(case['functional']), device=dev)
    target = _lib.cp_param()
    target.ptr, target.value = None, 0.8
    rs = torch.full((3,), CANARY, dtype=torch.float64, device=dev)
    assert lib.cp_sigma8_normalise(L.engine, *L.args, 1030, L.k.data_ptr(), functional.data_ptr(), target, rs.data_ptr(), None, None, L.work.data_ptr(), dev.index,
                                   stream) == _lib.CP_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((rs == CANARY).all())


@pytest.mark.parametrize('form', ['band', 'prefiltered'])
@pytest.mark.parametrize('engine', pt.ENGINES)
def test_fused_real_tophat_tables(env, basis, engine, form):
    """Both forms with the tables of the package's own TophatVariance plan: the u table is taken as given, in float64, and the truth transforms with longdouble
    FFTs (sigma_truth.fft_truth); radii between 4 and 30 Mpc/h, the band form behind LinearOperator.spline(natural)."""
    torch, _lib, lib, dev, stream = env
    import cosmoprimo_amd as cp
    from cosmoprimo_amd import interpolator as itp
    from cosmoprimo_amd.spline import LinearOperator
    fft = cp.TophatVariance(sg.K, device=dev)
    assert fft.size == sg.N and fft.padded_size == sg.NPAD and fft.nparallel == 1
    tables = [np.ascontiguousarray(t).ravel() for t in (fft.padded_prefactor, fft.padded_postfactor, fft.padded_u)]
    assert not np.iscomplexobj(tables[0]) and not np.iscomplexobj(tables[1]) and tables[2].dtype == np.complex128
    s = np.ascontiguousarray(fft.y[0], dtype='f8')
    case = sg.rz_case(engine, form, 129, 3, 5, basis, seed=2, real=(sg.real_tables(*tables), s))
    assert float(case['level_plain'].max()) < sg.CAP * sg.FLOOR
    L = Launch(env, case, sg.K, 129, 3, True)
    native = fft._get_plan(dev)
    if form == 'band':
        op = LinearOperator.spline(s, case['r'], bc='natural', device=dev)
        assert lib.cp_sigma_rz_fused_available(native.handle, op._handle) == 1
        _lib.check(lib.cp_sigma_rz_analytic(L.engine, *L.args, L.nk, L.k.data_ptr(), native.handle, op._handle, L.growth.data_ptr(), 3, L.out.data_ptr(), L.pk_ptr(),
                                            L.work.data_ptr(), 0, dev.index, stream))
    else:
        geo = itp._GeoSpline(s, case['r'], dev, fft=fft, keep=native)
        assert geo.handle is not None and geo.prefiltered
        _lib.check(lib.cp_sigma_rz_analytic_prefiltered(L.engine, *L.args, L.nk, L.k.data_ptr(), geo.handle, L.growth.data_ptr(), 3, L.out.data_ptr(), L.pk_ptr(),
                                                        L.work.data_ptr(), dev.index, stream))
    what = '%s, %s, the real TophatVariance tables' % (engine, form)
    kernel = 'sigma_rz_kernel<%s>, real tables' % ('true' if form == 'prefiltered' else 'false')
    assert note(kernel, sg.rz_fraction(L.sigma(), case, sg.sigma_extra(engine, True), what)) <= 1.
    assert note(kernel + ' pk_out', sg.pk_fraction(L.spectra(), case, sg.pk_extra(engine, True), what + ', pk_out', cap=np.inf)) <= 1.
