"""GPU: ``EmulatedEngine`` (cosmoprimo_amd/emulators/emulated.py), a :class:`Cosmology` served from a saved emulator, section by section.

Fixture (module scope, fitted once): Taylor emulators of order 2 of the calculator of ``Cosmology(engine='eisenstein_hu')`` on Omega_m in (0.28, 0.34) and h
in (0.64, 0.72) -- one at the default amplitude (sigma8 = 0.8: every training spectrum normalised), one trained with A_s fixed -- and an MLP
(``nhidden=(8,)``, two epochs: its accuracy is irrelevant, it drives the second engine) on the samples of the first.

Tolerances.  The consistency tests are exact (``torch.equal`` / ``array_equal``): the sections make the calls of the composition by hand on the same numbers.
At the expansion centre the Taylor emulator returns its centre sample -- every monomial but the constant is zero --, within ``dot_bound`` of
tests/test_taylor_gpu.py: 2 (n + degree + 2) eps |y| with n = 1 non-zero monomial and degree 2, i.e. 10 eps |y|.  Between knots the splines are held to
scipy at the tolerance tests/test_interpolator_contracts_gpu.py holds ``Interpolator1D(k=3)`` to (rtol 1e-11, atol 1e-13), plus those 10 eps of the knot values.
``Interpolator1D(k=3)`` is the natural cubic spline (as the reference's); scipy's not-a-knot cubic through the same knots differs from it by its end
conditions only, a perturbation that decays by 2 - sqrt(3) = 0.27 per knot from either end ((2 - sqrt(3))^24 = 2e-14): the 50 redshifts held to the
not-a-knot cubic lie at least 24 knots from both ends of the 256-knot grid, and the natural cubic is held over the whole grid."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = 2.**-53
LIMITS = {'Omega_m': (0.28, 0.34), 'h': (0.64, 0.72)}
A_S = 2.1e-9
BATCH = {'Omega_m': np.array([0.29, 0.30, 0.31, 0.32, 0.33]), 'h': np.array([0.65, 0.66, 0.68, 0.70, 0.71])}
ONE = {'Omega_m': 0.305, 'h': 0.67}


@pytest.fixture(scope='module')
def emulators(tmp_path_factory):
    from cosmoprimo_amd import Cosmology
    from cosmoprimo_amd.emulators import Emulator, get_calculator
    base = tmp_path_factory.mktemp('emulated')
    toret = {}
    taylor = Emulator(get_calculator(Cosmology(engine='eisenstein_hu')), params=LIMITS, engine='taylor', order=2, device='cuda:0')
    taylor.set_samples()
    taylor.fit()
    mlp = Emulator(None, params=LIMITS, engine='mlp', nhidden=(8,), device='cuda:0')
    mlp.set_samples(samples=taylor.samples)
    mlp.fit(epochs=2)
    fixed = Emulator(get_calculator(Cosmology(engine='eisenstein_hu', A_s=A_S)), params=LIMITS, engine='taylor', order=2, device='cuda:0')
    fixed.set_samples()
    fixed.fit()
    for name, emulator in (('taylor', taylor), ('mlp', mlp), ('fixed_A_s', fixed)):
        fn = str(base / (name + '.npy'))
        emulator.save(fn)
        toret[name] = (fn, Emulator.load(fn, device='cuda:0'))
    toret['centre'] = {name: float(value) for name, value in zip(LIMITS, taylor.engine.center)}
    return toret


def emulated(emulators, name, **params):
    from cosmoprimo_amd import Cosmology
    from cosmoprimo_amd.emulators import EmulatedEngine
    return Cosmology(engine=EmulatedEngine.read(emulators[name][0]), **params)


def host(value):
    import torch
    return value.cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)


@pytest.mark.parametrize('name', ['taylor', 'mlp'])
@pytest.mark.parametrize('params', [ONE, BATCH], ids=['one', 'batch'])
def test_sections_are_the_composition_by_hand(emulators, name, params):
    """Every section quantity equals ``Emulator.predict(params, device=True)[key]`` put through ``Interpolator1D(k=3)`` / ``PowerSpectrumInterpolator2D``, bit
    for bit; a batch gives (B, nz) and (B, nk, nz) as the eisenstein_hu engine does."""
    import torch
    from cosmoprimo_amd import Cosmology
    from cosmoprimo_amd.emulators import get_default_z_callable
    from cosmoprimo_amd.interpolator import Interpolator1D, PowerSpectrumInterpolator2D
    cosmo = emulated(emulators, name, **params)
    true = Cosmology(engine='eisenstein_hu', **params)
    batch = np.ndim(params['h']) > 0
    assert cosmo.engine.batch_size == (5 if batch else None)
    pred = emulators[name][1].predict(dict(params), device=True)
    zk = get_default_z_callable('background')
    z = np.linspace(0.01, 3., 7)
    ba = cosmo.get_background()
    for key in ('comoving_radial_distance', 'time', 'rho_fld'):
        table = pred['background.' + key]
        assert isinstance(table, torch.Tensor) and tuple(table.shape) == ((5, 256) if batch else (256,))
        want = Interpolator1D(zk, table.movedim(-1, 0), k=3, interp_x='lin', interp_fun='lin', extrap=False, assume_sorted=True)(z)
        got = getattr(ba, key)(z)
        assert np.array_equal(got, want.T if batch else want, equal_nan=True), key
        assert got.shape == getattr(true.get_background(), key)(z).shape == ((5, 7) if batch else (7,))
    assert ba.rho_ncdm(z).shape == true.get_background().rho_ncdm(z).shape
    assert np.array_equal(ba.efunc(z), true.get_background().efunc(z))      # from the parameters, as ever
    th = cosmo.get_thermodynamics()
    for key in ('rs_drag', 'z_drag'):
        assert torch.equal(getattr(th, key), pred['thermodynamics.' + key])
        assert tuple(getattr(th, key).shape) == ((5,) if batch else ())
    fo = cosmo.get_fourier()
    rs = cosmo.engine._rsigma8      # sigma8 = 0.8 by default: the spectra are rescaled to it (a NaN for an MLP whose spectra are not positive)
    assert cosmo.engine._needs_rescale == 'sigma8' and np.shape(rs) == ((5,) if batch else ())
    factor = torch.as_tensor(np.asarray(rs, dtype='f8')**2, device='cuda:0').reshape((-1, 1, 1) if batch else ())
    k, zpk = np.geomspace(1e-3, 5., 9), np.array([0., 0.5, 2.])
    for of in ('delta_m', ('delta_m', 'theta_m'), 'theta_m'):
        names = (of, of) if isinstance(of, str) else of
        table = pred['fourier.pk.{}.{}'.format(*names)]
        assert tuple(table.shape) == ((5, 422, 30) if batch else (422, 30))
        scaled = table * factor
        want = PowerSpectrumInterpolator2D(pred['fourier.k'], pred['fourier.z'], scaled, device=table.device)(k, zpk)
        got = fo.pk_interpolator(of=of)(k, zpk)
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(fo.pk_kz(k, zpk, of=of), want, equal_nan=True), of
        assert got.shape == ((5, 9, 3) if batch else (9, 3)) == true.get_fourier().pk_interpolator(of=of)(k, zpk).shape
    assert np.shape(fo.sigma8_m) == np.shape(fo.sigma8_z(0.)) == ((5,) if batch else ())
    assert np.shape(fo.sigma_rz(np.array([4., 8.]), zpk)) == ((5, 2, 3) if batch else (2, 3))
    pm = cosmo.get_primordial()
    assert np.array_equal(host(pm.A_s), host(pred['primordial.A_s']) * np.asarray(rs)**2, equal_nan=True)
    assert np.allclose(host(pm.ln_1e10_A_s), np.log(1e10 * host(pm.A_s)), rtol=1e-15, atol=0, equal_nan=True)
    want = pm.pk_k(k)
    assert want.shape == ((5, 9) if batch else (9,)) == true.get_primordial().pk_k(k).shape
    h, A_s = (np.asarray(v, dtype='f8').reshape((-1, 1) if batch else ()) for v in (params['h'], host(pm.A_s)))
    assert np.allclose(want, h**3 * A_s * (k / (0.05 / h))**(0.96 - 1.), rtol=1e-14, atol=0, equal_nan=True)
    assert np.array_equal(pm.pk_interpolator()(k), want.T if batch else want, equal_nan=True)      # (nk, B): the columns of a 1D interpolator, as eisenstein_hu's


def test_background_alone_is_predicted_and_held(emulators, monkeypatch):
    """``get_background()`` of B = 2000 cosmologies asks the emulator for the 'background' keys only, and allocates less than the B x M doubles of the full
    table; ``get_fourier()`` is what asks for the spectra."""
    import torch
    from cosmoprimo_amd.emulators import Emulator
    calls = []
    predict = Emulator.predict

    def spy(self, params, device=False, keys=None):
        calls.append(keys)
        return predict(self, params, device=device, keys=keys)

    monkeypatch.setattr(Emulator, 'predict', spy)
    B = 2000
    rng = np.random.default_rng(3)
    device = torch.device('cuda', 0)
    cosmo = emulated(emulators, 'taylor', Omega_m=torch.as_tensor(rng.uniform(0.29, 0.33, B), device=device), h=torch.as_tensor(rng.uniform(0.65, 0.71, B), device=device))
    emulator = emulators['taylor'][1]
    M = int(emulator.engine.derivatives.shape[1])
    assert M > 3 * 422 * 30
    cosmo.engine      # (made with the cosmology)
    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    before = torch.cuda.memory_allocated(device)
    ba = cosmo.get_background()
    torch.cuda.synchronize(device)
    peak = torch.cuda.max_memory_allocated(device) - before
    print('get_background() of %d cosmologies: peak %d bytes allocated, the full table is %d' % (B, peak, 8 * B * M))
    assert calls == ['background']
    assert peak < 8 * B * M
    assert 'fourier' not in cosmo.engine._sections
    assert tuple(ba.comoving_radial_distance(np.array([0.5, 1.])).shape) == (B, 2)
    assert calls == ['background']
    cosmo.get_fourier()
    assert 'fourier' in calls and 'background' not in calls[1:]


@pytest.fixture(scope='module')
def centre(emulators):
    """The true engine at the expansion centre, evaluated as a batch of one cosmology: the route the training samples took."""
    from cosmoprimo_amd import Cosmology
    from cosmoprimo_amd.emulators import get_calculator
    params = {name: np.array([value]) for name, value in emulators['centre'].items()}
    true = Cosmology(engine='eisenstein_hu', **params)
    fixed = get_calculator(Cosmology(engine='eisenstein_hu', A_s=A_S))(**params)
    return params, true, fixed


@pytest.mark.parametrize('key', ['comoving_radial_distance', 'time'])
def test_background_at_the_centre_against_the_true_engine(emulators, centre, key):
    from scipy.interpolate import CubicSpline
    from cosmoprimo_amd.emulators import get_default_z_callable
    params, true, _ = centre
    zk = get_default_z_callable('background')
    truth = getattr(true.get_background(), key)(zk)[0]
    ba = emulated(emulators, 'taylor', **params).get_background()
    got = getattr(ba, key)(zk)[0]
    knots = np.abs(got - truth) / (10 * EPS * np.abs(truth) + 1e-300)
    print('%s at the 256 knots: %.3g of the bound' % (key, np.nanmax(knots)))
    assert got.shape == truth.shape == (256,) and np.isfinite(got).all() and (knots <= 1.).all()
    rng = np.random.default_rng(5)
    for name, spline, lo, hi in (('natural', CubicSpline(zk, truth, bc_type='natural'), 0, 255), ('not-a-knot', CubicSpline(zk, truth, bc_type='not-a-knot'), 24, 231)):
        i = rng.integers(lo, hi, 50)
        z = zk[i] + rng.uniform(0.05, 0.95, 50) * (zk[i + 1] - zk[i])
        got, want = getattr(ba, key)(z)[0], spline(z)
        excess = np.abs(got - want) / (1e-13 + (1e-11 + 10 * EPS) * np.abs(want))
        print('%s between knots against scipy %s: %.3g of the tolerance' % (key, name, excess.max()))
        assert got.shape == (50,) and (excess <= 1.).all(), name


def test_pk_at_the_centre_against_the_true_table(emulators, centre):
    """The emulator trained with A_s fixed, the cosmology given that A_s: no rescaling (``_rsigma8`` is exactly 1), the table is the centre sample."""
    from cosmoprimo_amd.interpolator import PowerSpectrumInterpolator2D
    params, _, fixed = centre
    cosmo = emulated(emulators, 'fixed_A_s', A_s=A_S, **params)
    fo = cosmo.get_fourier()
    assert cosmo.engine._needs_rescale == 'A_s' and np.all(np.asarray(cosmo.engine._rsigma8) == 1.)
    truth = fixed['fourier.pk.delta_m.delta_m']
    table = host(fo.table()[2])
    assert table.shape == truth.shape == (1, 422, 30) and (np.abs(table - truth) <= 10 * EPS * np.abs(truth)).all()
    rng = np.random.default_rng(6)
    k, z = np.exp(rng.uniform(np.log(1e-5), np.log(50.), 50)), rng.uniform(0., 9.5, 20)
    want = PowerSpectrumInterpolator2D(fixed['fourier.k'], fixed['fourier.z'], truth, device='cuda:0')(k, z)[0]
    got = fo.pk_interpolator()(k, z)[0]
    excess = np.abs(got - want) / (1e-13 * np.abs(truth).min() + (1e-11 + 10 * EPS) * np.abs(want))
    print('pk between knots: %.3g of the tolerance' % excess.max())
    assert got.shape == want.shape == (50, 20) and (excess <= 1.).all()


@pytest.mark.parametrize('params', [ONE, BATCH], ids=['one', 'batch'])
def test_sigma8_given_to_an_emulator_trained_with_A_s_fixed(emulators, params):
    cosmo = emulated(emulators, 'fixed_A_s', sigma8=0.8, **params)
    fo = cosmo.get_fourier()
    assert cosmo.engine._needs_rescale == 'sigma8'
    assert np.allclose(fo.sigma8_m, 0.8, rtol=1e-12, atol=0)
    plain = emulators['fixed_A_s'][1].predict(dict(params), device=True)
    from cosmoprimo_amd.interpolator import PowerSpectrumInterpolator2D
    sigma8_emulated = PowerSpectrumInterpolator2D(plain['fourier.k'], plain['fourier.z'], plain['fourier.pk.delta_m.delta_m']).sigma8_z(0.)
    factor = (0.8 / np.asarray(sigma8_emulated))**2
    assert np.array_equal(np.asarray(cosmo.engine._rsigma8)**2, factor)
    table = host(plain['fourier.pk.delta_m.delta_m'])
    assert np.array_equal(host(fo.table()[2]), table * factor.reshape(factor.shape + (1, 1) if factor.ndim else ()))
    assert np.allclose(host(cosmo.get_primordial().A_s), A_S * factor, rtol=1e-15, atol=0)      # A_s and sigma8_m reported consistently
    assert np.all(np.abs(factor - 1.) < 0.5) and np.all(factor != 1.)


@pytest.mark.parametrize('name', ['taylor', 'mlp'])
def test_calculator_of_an_emulated_cosmology_returns_the_emulator(emulators, name):
    """Keys, shapes and (without rescaling) values of ``Emulator.predict``: an emulator of an emulator, or a re-fit, sees what the emulator holds."""
    from cosmoprimo_amd.emulators import get_calculator
    cosmo = emulated(emulators, 'fixed_A_s' if name == 'taylor' else name, **({'A_s': A_S} if name == 'taylor' else {}))
    for params in (ONE, BATCH):
        got = get_calculator(cosmo)(**params)
        want = emulators['fixed_A_s' if name == 'taylor' else name][1].predict(dict(params))
        assert sorted(got) == sorted(want)
        for key in want:
            assert np.shape(got[key]) == np.shape(want[key]), key
            if name == 'taylor' or not key.startswith(('fourier.pk', 'primordial')):
                assert np.array_equal(got[key], want[key], equal_nan=True), key


def test_load_warns_and_missing_parameters_raise(emulators, tmp_path):
    from cosmoprimo_amd import Cosmology, CosmologyError
    from cosmoprimo_amd.emulators import EmulatedEngine
    with pytest.warns(DeprecationWarning):
        Engine = EmulatedEngine.load(emulators['taylor'][0])
    assert Cosmology(engine=Engine, **ONE).get_thermodynamics().rs_drag.ndim == 0
    state = emulators['taylor'][1].__getstate__()
    state['params'] = {'Omega_m': LIMITS['Omega_m'], 'no_such_parameter': (0., 1.)}
    fn = str(tmp_path / 'unknown_parameter.npy')
    np.save(fn, state, allow_pickle=True)
    with pytest.raises(CosmologyError, match='no_such_parameter'):
        Cosmology(engine=EmulatedEngine.read(fn), **ONE)
    cosmo = emulated(emulators, 'taylor', **ONE)
    with pytest.raises(CosmologyError):      # a key the emulator lacks
        cosmo.get_thermodynamics().rs_star
    with pytest.raises(CosmologyError):
        cosmo.get_fourier().pk_interpolator(of='delta_cb')


def test_clone_and_fiducial(emulators):
    from cosmoprimo_amd import Cosmology, fiducial
    from cosmoprimo_amd.emulators import EmulatedEngine
    cosmo = emulated(emulators, 'taylor', **ONE)
    z = np.array([0.3, 1.1])
    first = cosmo.comoving_radial_distance(z)
    clone = cosmo.clone(Omega_m=0.32)
    assert type(clone.engine) is type(cosmo.engine) and clone.engine is not cosmo.engine
    second = clone.comoving_radial_distance(z)
    assert second.shape == (2,) and np.isfinite(second).all() and (second < first).all()      # more matter, shorter distances
    again = Cosmology(engine='eisenstein_hu', **ONE).clone(engine=EmulatedEngine.read(emulators['taylor'][0]))
    assert np.array_equal(again.comoving_radial_distance(z), first)
    desi = fiducial.DESI(engine=EmulatedEngine.read(emulators['taylor'][0]))
    got = desi.comoving_radial_distance(z)
    assert got.shape == (2,) and np.isfinite(got).all()
    batch = fiducial.DESI(engine=EmulatedEngine.read(emulators['taylor'][0]), Omega_m=BATCH['Omega_m'])
    assert batch.get_background().time(z).shape == (5, 2)
