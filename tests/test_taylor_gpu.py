"""GPU: the Taylor emulator on the device (cp_taylor_fit / cp_taylor_predict, csrc/cp_taylor.hip; cosmoprimo_amd/emulators/tools) against
tests/golden/taylor.npz -- the reference's own coefficients and predictions for a toy function (tools/gen_taylor_golden.py) -- against an exact
polynomial, and on the package's own batch driver.

Tolerance (derived, not measured; the one of test_taylor_host.py).  Both sides compute the same dot products in different orders: for row t and column
m of A @ B the allowed difference is ``K eps sum_i |A_ti| |B_im|`` with eps = 2^-53 and K = 2 (n + ndim + 2): n the non-zero entries of the row of A,
ndim + 2 for the products that form a weight or a monomial, the factor 2 because the reference and this code each carry that error.  A, B are S, Y for
the fit and the monomials, ``derivatives`` for the prediction.  numpy's own products on the build machine used 0.054 (fit) and 0.12 (prediction) of it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NCONFIGS = 5
EPS = 2.**-53


def dot_bound(A, B, ndim):
    n = (A != 0).sum(axis=1)
    return (2 * (n + ndim + 2))[:, None] * EPS * (np.abs(A) @ np.abs(B))


def monomials(X, center, powers):
    d = np.asarray(X) - center
    mono = np.ones((len(d), len(powers)))
    for t, power in enumerate(powers):
        for j, p in enumerate(power):
            if p > 0:
                mono[:, t] *= d[:, j]**int(p)
    return mono


def engine_of(g, i, derivatives=None):
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    return TaylorEmulatorEngine.from_state({'center': g['c%d_center' % i], 'powers': g['c%d_powers' % i],
                                            'derivatives': g['c%d_derivatives' % i] if derivatives is None else derivatives}, device='cuda:0')


@pytest.mark.parametrize('i', range(NCONFIGS))
def test_fit(golden, i):
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    from cosmoprimo_amd.emulators.tools import taylor_operator
    g = golden('taylor')
    X, Y = g['c%d_X' % i], g['c%d_Y' % i]
    attrs = {'cidx': g['c%d_cidx' % i], 'order': g['c%d_order' % i], 'accuracy': g['c%d_accuracy' % i]}
    engine = TaylorEmulatorEngine(device='cuda:0').fit(X, Y, attrs)
    assert np.array_equal(engine.powers, g['c%d_powers' % i]) and np.array_equal(engine.center, g['c%d_center' % i])
    S = taylor_operator(X, attrs['cidx'], attrs['order'], attrs['accuracy'])[2]
    ratio = np.abs(engine.derivatives - g['c%d_derivatives' % i]) / dot_bound(S, Y, 3)
    print('config %d: fit, largest fraction of the bound %.3g' % (i, ratio.max()))
    assert engine.derivatives.shape == g['c%d_derivatives' % i].shape and ratio.max() <= 1.
    assert np.array_equal(engine._dev['derivatives'].cpu().numpy(), engine.derivatives)


@pytest.mark.parametrize('i', range(NCONFIGS))
def test_predict(golden, i):
    g = golden('taylor')
    engine = engine_of(g, i)
    Xq, Yq = g['c%d_Xq' % i], g['c%d_Yq' % i]
    bound = dot_bound(monomials(Xq, g['c%d_center' % i], g['c%d_powers' % i]), g['c%d_derivatives' % i], 3)
    got = engine.predict(Xq).cpu().numpy()      # one batch of 33
    ratio = np.abs(got - Yq) / bound
    print('config %d: predict, largest fraction of the bound %.3g' % (i, ratio.max()))
    assert got.shape == Yq.shape and ratio.max() <= 1.
    ones = np.concatenate([engine.predict(Xq[j:j + 1]).cpu().numpy() for j in range(len(Xq))])      # 33 batches of 1
    assert np.array_equal(ones, got)
    assert np.array_equal(engine.predict(Xq[5:22]).cpu().numpy(), got[5:22])      # a batch of 17


@pytest.mark.parametrize('i', range(NCONFIGS))
@pytest.mark.parametrize('M', [50, 1000])
def test_predict_tiled(golden, i, M):
    """More than one tile in each direction, with ragged ends: the columns of ``derivatives`` tiled to M, the queries to B = 300."""
    g = golden('taylor')
    reps = -(-M // 8)
    derivatives = np.tile(g['c%d_derivatives' % i], (1, reps))[:, :M]
    Xq = np.tile(g['c%d_Xq' % i], (10, 1))[:300]
    Yq = np.tile(np.tile(g['c%d_Yq' % i], (1, reps))[:, :M], (10, 1))[:300]
    got = engine_of(g, i, derivatives).predict(Xq).cpu().numpy()
    ratio = np.abs(got - Yq) / dot_bound(monomials(Xq, g['c%d_center' % i], g['c%d_powers' % i]), derivatives, 3)
    assert got.shape == (300, M) and ratio.max() <= 1.


def test_nan_containment(golden):
    """Configuration {a: 2, b: 0, c: 1}: no power of b is positive, so a NaN (or infinite) b changes nothing."""
    g = golden('taylor')
    assert (g['c4_powers'][:, 1] == 0).all()
    engine = engine_of(g, 4)
    Xq = g['c4_Xq'].copy()
    ref = Xq.copy()
    ref[:, 1] = g['c4_center'][1]
    Xq[::2, 1], Xq[1::2, 1] = np.nan, np.inf
    got = engine.predict(Xq).cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, engine.predict(ref).cpu().numpy())


@pytest.mark.parametrize('accuracy,cubes', [(2, False), (4, True)])
def test_polynomial_exactness(accuracy, cubes):
    """Independent of the reference: a polynomial of total degree <= 3 in 4 parameters (M = 40) is its own Taylor expansion of order 3, so an emulator of
    order 3 reproduces it wherever its finite differences are exact.  At accuracy 2 the first derivative is the three-point central difference, which is
    exact up to degree 2 in its parameter: (f(c + h) - f(c - h)) / 2h of x^3 is 3 c^2 + h^2, for the reference as for this code (on the build machine
    a pure cube costs 0.05 absolute in the prediction at these limits, 5e11 times the bound -- truncation, not rounding).  So the accuracy-2 case takes every
    monomial of total degree <= 3 except the four pure cubes (all mixed cubic terms x^2 y, x y z are in), and the general polynomial, cubes included, is
    asked at accuracy 4, whose five-point first and second and seven-point third differences are exact on it.
    The bound is the dot-product bound applied to S . Y (the coefficients), carried through the monomials, plus the dot-product bound of the prediction
    itself; the exact values are the polynomial evaluated in longdouble."""
    import itertools
    from cosmoprimo_amd.emulators import Emulator
    from cosmoprimo_amd.emulators.tools import taylor_operator
    rng = np.random.default_rng(7)
    names = ['p0', 'p1', 'p2', 'p3']
    limits = {'p0': (-0.5, 0.5), 'p1': (0.9, 1.1), 'p2': (1.5, 2.5), 'p3': (-1.2, -0.8)}
    exps = [e for e in itertools.product(range(4), repeat=4) if sum(e) <= 3 and (cubes or max(e) <= 2)]
    coeffs = rng.uniform(-1., 1., (len(exps), 40))
    calls = []

    def poly(X, dtype='f8'):
        X = np.asarray(X, dtype=dtype)
        return sum(np.prod([X[:, j:j + 1]**e[j] for j in range(4)], axis=0) * coeffs[k].astype(dtype) for k, e in enumerate(exps))

    def calculator(**params):
        calls.append({name: np.shape(value) for name, value in params.items()})
        X = np.column_stack([np.atleast_1d(params[name]) for name in names])
        value = poly(X)
        return {'y': value if np.ndim(params['p0']) else value[0], 'grid': np.arange(3.)}

    emulator = Emulator(calculator, params=limits, engine='taylor', order=3, accuracy=accuracy, device='cuda:0')
    samples = emulator.set_samples()
    npoints = len(samples['p0'])
    assert calls == [{name: () for name in names}, {name: (npoints,) for name in names}]      # the centre, and ONE call for the whole grid
    emulator.fit()
    assert len(calls) == 2
    engine = emulator.engine
    Xq = np.column_stack([rng.uniform(*limits[name], 64) for name in names])
    got = emulator.predict({name: Xq[:, j] for j, name in enumerate(names)})
    assert set(got) == {'y', 'grid'} and got['y'].shape == (64, 40) and np.array_equal(got['grid'], np.arange(3.))
    S = taylor_operator(samples.matrix(), samples.attrs['cidx'], [3] * 4, [accuracy] * 4)[2]
    Y = samples.varied['y']
    mono = monomials(Xq, engine.center, engine.powers)
    fit_bound = dot_bound(S, Y, 4)
    bound = np.abs(mono) @ fit_bound + dot_bound(mono, np.abs(engine.derivatives) + fit_bound, 4)
    exact = np.asarray(poly(Xq, dtype=np.longdouble), dtype='f8')
    ratio = np.abs(got['y'] - exact) / bound
    print('polynomial, accuracy %d: largest fraction of the bound %.3g' % (accuracy, ratio.max()))
    assert ratio.max() <= 1.


@pytest.fixture(scope='module')
def driver():
    import warnings
    import cosmoprimo_amd as cp
    from cosmoprimo_amd.emulators import Emulator, get_calculator
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        calculator = get_calculator(cp.Cosmology(engine='eisenstein_hu'), section=['background', 'thermodynamics'])
        params = {'Omega_m': (0.28, 0.34), 'h': (0.64, 0.72)}
        emulators = {}
        for order in (1, 2):
            emulators[order] = Emulator(calculator, params=params, engine='taylor', order=order, device='cuda:0')
            emulators[order].set_samples()
            emulators[order].fit()
        point = dict(Omega_m=0.325, h=0.70)
        batch = dict(Omega_m=np.linspace(0.29, 0.33, 5), h=np.linspace(0.65, 0.71, 5))
        return dict(calculator=calculator, emulators=emulators, point=point, batch=batch, at_point=calculator(**point), at_batch=calculator(**batch))


def test_driver_keys_and_shapes(driver):
    emulator = driver['emulators'][2]
    for params, ref in [(driver['point'], driver['at_point']), (driver['batch'], driver['at_batch'])]:
        got = emulator.predict(params)
        assert list(sorted(got)) == list(sorted(ref))
        for key, value in ref.items():
            assert np.shape(got[key]) == np.shape(value), key
        assert np.array_equal(got['background.z'], ref['background.z'])
        again = emulator.to_calculator()(**params)
        assert all(np.array_equal(again[key], got[key]) for key in got)
    assert 'background.z' in emulator.fixed and 'background.comoving_radial_distance' in emulator.varied_keys


def test_driver_centre_is_exact(driver):
    emulator = driver['emulators'][2]
    samples = emulator.samples
    cidx = samples.attrs['cidx'][0]
    got = emulator.predict({name: float(samples[name][cidx]) for name in emulator.params})
    for key in emulator.varied_keys:      # every monomial but term 0 is exactly 0
        assert np.array_equal(got[key], samples.varied[key][cidx]), key


def test_driver_order_2_beats_order_1(driver):
    ref = driver['at_point']['background.comoving_radial_distance']
    err = {order: np.abs(emulator.predict(driver['point'])['background.comoving_radial_distance'] - ref).max() for order, emulator in driver['emulators'].items()}
    print('off-centre error of the radial distance: order 1 %.3g, order 2 %.3g' % (err[1], err[2]))
    assert err[2] < err[1]


def test_driver_save_load(driver, tmp_path):
    from cosmoprimo_amd.emulators import Emulator
    emulator = driver['emulators'][2]
    fn = str(tmp_path / 'emulator.npy')
    emulator.save(fn)
    loaded = Emulator.load(fn, device='cuda:0')
    assert np.array_equal(loaded.engine.derivatives, emulator.engine.derivatives) and np.array_equal(loaded.engine.powers, emulator.engine.powers)
    assert loaded.engine.sampler_options == emulator.engine.sampler_options
    a, b = emulator.predict(driver['batch']), loaded.predict(driver['batch'])
    assert list(a) == list(b) and all(np.array_equal(a[key], b[key]) for key in a)


def test_no_host_sync_in_predict(golden):
    """``predict(device=True)`` can be recorded into a HIP graph (torch refuses synchronisations, pageable copies and allocations outside its pool while it
    captures), and a replay on new parameter values in the same buffers gives exactly what the eager call gives (tests/test_no_host_sync_gpu.py)."""
    import torch
    from cosmoprimo_amd.emulators import Emulator
    g = golden('taylor')
    dev = torch.device('cuda', 0)
    emulator = Emulator(None, params={str(name): tuple(limits) for name, limits in zip(g['names'], g['limits'])}, device=dev)
    emulator.engine = engine_of(g, 1)
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['curve', 'product'], [(7,), ()], {'x': np.linspace(0.1, 1., 7)}
    Xq = g['c1_Xq']
    static = {name: torch.as_tensor(Xq[:17, j].copy(), device=dev) for j, name in enumerate(emulator.params)}
    fresh = {name: torch.as_tensor(Xq[16:, j].copy(), device=dev) for j, name in enumerate(emulator.params)}

    def fn():
        out = emulator.predict({name: v[:] for name, v in static.items()}, device=True)
        assert out['curve'].shape == (17, 7) and out['product'].shape == (17,) and out['curve'].data_ptr() + 7 * 8 == out['product'].data_ptr()      # views of one buffer
        return out['curve']

    for _ in range(2):
        fn()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    for name, value in fresh.items():
        static[name].copy_(value)
    graph.replay()
    torch.cuda.synchronize(dev)
    replayed = out.clone()
    eager = fn()
    assert bool(torch.isfinite(eager).all()) and torch.equal(replayed, eager)
    ratio = np.abs(eager.cpu().numpy() - g['c1_Yq'][16:, :7]) / dot_bound(monomials(Xq[16:], g['c1_center'], g['c1_powers']), g['c1_derivatives'][:, :7], 3)
    assert ratio.max() <= 1.


def test_caps(golden):
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    g = golden('taylor')
    powers = g['c0_powers'].copy()
    powers[-1, 0] = 16
    engine = TaylorEmulatorEngine.from_state({'center': g['c0_center'], 'powers': powers, 'derivatives': g['c0_derivatives']}, device='cuda:0')
    with pytest.raises(NotImplementedError):
        engine.predict(g['c0_Xq'])
    powers[-1, 0] = 15      # the largest power that is built: x^15 by repeated multiplication
    engine = TaylorEmulatorEngine.from_state({'center': g['c0_center'], 'powers': powers, 'derivatives': g['c0_derivatives']}, device='cuda:0')
    ratio = np.abs(engine.predict(g['c0_Xq']).cpu().numpy() - monomials(g['c0_Xq'], g['c0_center'], powers) @ g['c0_derivatives'])
    assert (ratio <= dot_bound(monomials(g['c0_Xq'], g['c0_center'], powers), g['c0_derivatives'], 3 + 15)).all()
    engine = TaylorEmulatorEngine.from_state({'center': np.zeros(33), 'powers': np.ones((2, 33), dtype='i4'), 'derivatives': np.ones((2, 4))}, device='cuda:0')
    with pytest.raises(NotImplementedError):
        engine.predict(np.zeros((3, 33)))
