"""GPU: the MLP emulator on the device (cp_mlp_predict / cp_mlp_loss_grad / cp_mlp_adam, csrc/cp_mlp.hip; cosmoprimo_amd/emulators/tools/mlp.py) against
tests/golden/mlp.npz (the reference's predictions, tools/gen_mlp_golden.py), against a manual backward pass in ``np.longdouble``, against torch's autograd
and Adam on the CPU, and on the package's own batch driver.

Tolerances (tests/mlp_reference.py).  Predict: the derived running bound of the forward pass.  Gradient: per parameter block, 16 times the rounding
level of the float64 numpy backward pass (measured against the longdouble one on the same inputs, relative to the block's largest gradient, floored
at eps): the device sums in another order (MFMA steps of 4, tiles, slices) and has its own exp.  Adam: sqrt and division are correctly rounded and the
kernel rounds every operation once, as numpy does, so the two differ by the rounding of ``1 - b`` products at most; allowed: 4 eps of
``|p| + lr |m_hat| / (sqrt(v_hat) + eps)`` for p and 4 eps of the two terms' magnitudes for m and v."""
import ctypes

import numpy as np
import pytest

import mlp_reference as mr

pytestmark = pytest.mark.gpu
NCONFIGS = 6


def engine_of(cfg):
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    return MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')


@pytest.mark.parametrize('i', range(NCONFIGS))
def test_predict(golden, i):
    cfg = mr.golden_config(golden('mlp'), i)
    truth, bound = mr.predict_bound(*[cfg[name] for name in ('packed', 'dims', 'activations', 'Xq', 'xoffset', 'xscale', 'yoffset', 'yscale', 'yfunction')])
    got = engine_of(cfg).predict(cfg['Xq']).cpu().numpy()
    fraction, reference = float((np.abs(got - truth) / bound).max()), float((np.abs(cfg['Yq'] - truth) / bound).max())
    print('config %d: the device uses %.3g of the bound, the reference %.3g' % (i, fraction, reference))
    assert got.shape == cfg['Yq'].shape and fraction <= 1. and reference <= 1.


def device_loss_grad(packed, dims, activations, X, Y, with_grad=True):
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    L = len(dims) - 2
    widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in activations])
    Xd, Yd, pd = (torch.as_tensor(np.ascontiguousarray(a, dtype='f8'), device=device) for a in (X, Y, packed))
    work = torch.full((int(lib.cp_mlp_workspace_doubles(len(X), dims[0], L, widths, dims[-1])),), np.nan, dtype=torch.float64, device=device)
    loss = torch.full((1,), np.nan, dtype=torch.float64, device=device)
    grad = torch.full((pd.numel() + 1,), -7.25, dtype=torch.float64, device=device)
    _lib.check(lib.cp_mlp_loss_grad(Xd.data_ptr(), Yd.data_ptr(), len(X), dims[0], L, widths, acts, dims[-1], pd.data_ptr(), work.data_ptr(), work.numel(),
                                    loss.data_ptr(), grad.data_ptr() if with_grad else None, 0, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    grad = grad.cpu().numpy()
    assert grad[-1] == -7.25      # nothing past the packed layout
    return float(loss.item()), grad[:-1]


GRADIENT_CASES = [(b, M, widths, acts) for b in (1, 64, 100) for M, widths, acts in ((8, (32, 32, 32), ['silu', 'relu', 'tanh']), (300, (5, 17), ['identity-silu', 'silu']),
                                                                                    (300, (64,), ['identity-silu']), (8, (5, 17), ['tanh', 'identity-silu']))]


@pytest.mark.parametrize('b,M,widths,activations', GRADIENT_CASES, ids=['b%d-M%d-%s' % (c[0], c[1], 'x'.join(map(str, c[2]))) for c in GRADIENT_CASES])
def test_loss_grad(b, M, widths, activations):
    rng = np.random.default_rng(1000 * b + M + len(widths))
    dims = (3,) + tuple(widths) + (M,)
    packed = np.zeros(mr.nparams(dims))
    for name, sl in mr.blocks(dims).items():
        packed[sl] = rng.uniform(0.3, 1.2, 2) if name.startswith('alphabeta') else rng.normal(0., 1. / np.sqrt(dims[int(name[-1])]) if name.startswith('kernel') else 0.3, sl.stop - sl.start)
    X, Y = rng.uniform(0., 1., (b, 3)), rng.uniform(0., 1., (b, M))
    levels, (loss_ld, grad_ld), _ = mr.gradient_levels(packed, dims, activations, X, Y)
    loss, grad = device_loss_grad(packed, dims, activations, X, Y)
    again = device_loss_grad(packed, dims, activations, X, Y)
    only = device_loss_grad(packed, dims, activations, X, Y, with_grad=False)
    assert again[0] == loss and np.array_equal(again[1], grad)      # two calls, bit for bit
    assert only[0] == loss and (only[1] == -7.25).all()             # loss only: the same bits, the gradient untouched
    assert abs(loss - float(loss_ld)) <= 16 * 2 * np.sqrt(b * M) * mr.EPS * float(loss_ld)
    for name, sl in mr.blocks(dims).items():
        top, level = levels[name]
        if top == 0.:
            assert not grad[sl].any(), name
            continue
        fraction = float(np.abs(grad[sl] - np.asarray(grad_ld[sl], dtype='f8')).max()) / (16 * level * top)
        print('b = %d, M = %d, %s %s: level %.3g, the device uses %.3g of 16 x' % (b, M, widths, name, level, fraction))
        assert fraction <= 1., name


def test_adam():
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    rng = np.random.default_rng(9)
    n, lr, step = 1000, 1e-2, 3
    p, m, g = rng.normal(0., 1., n), rng.normal(0., 1e-2, n), rng.normal(0., 1e-2, n)
    v = rng.uniform(0., 1e-4, n)
    g[:100], v[50:150], m[50:60] = 0., 0., 0.      # g = 0, v = 0, both with m = 0: the update is 0 / (0 + eps)
    device = torch.device('cuda', 0)
    pd, md, vd, gd = (torch.as_tensor(a.copy(), device=device) for a in (p, m, v, g))
    c1, c2 = 1. - 0.9**step, 1. - 0.999**step
    _lib.check(_lib.load().cp_mlp_adam(pd.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), n, lr, 0.9, 0.999, 1e-8, c1, c2, 0, dv.stream_of(device)))
    p1, m1, v1 = mr.adam(p, m, v, g, lr, step)
    got_p, got_m, got_v = (t.cpu().numpy() for t in (pd, md, vd))
    assert np.array_equal(gd.cpu().numpy(), g)
    assert (np.abs(got_m - m1) <= 4 * mr.EPS * (0.9 * np.abs(m) + 0.1 * np.abs(g))).all()
    assert (np.abs(got_v - v1) <= 4 * mr.EPS * (0.999 * v + 0.001 * g * g)).all()
    update = lr * np.abs(m1 / c1) / (np.sqrt(v1 / c2) + 1e-8)
    excess = np.abs(got_p - p1) / (4 * mr.EPS * (np.abs(p) + update))
    print('adam: p uses %.3g of 4 eps' % excess.max())
    assert (excess <= 1.).all() and np.isfinite(got_p).all() and np.array_equal(got_p[50:60], p[50:60])


@pytest.fixture(scope='module')
def toy():
    from cosmoprimo_amd.emulators import QMCSampler
    X = QMCSampler(None, mr.TOY_LIMITS, engine='rqrs').points(256).matrix()
    return X, mr.toy(*X.T)


def test_first_three_steps(toy):
    """(a) One epoch of three batches against forward / backward / Adam restated in float64 numpy from the same initial weights.  Allowed per entry: the
    sum over the steps of ``lr min(2, 3 dg / (sqrt(v_hat) + eps))``, the first-order effect on ``m_hat / (sqrt(v_hat) + eps)`` of a gradient off by dg
    (both moments move; the ratio never moves by more than 2), with dg twice the gradient tolerance of test_loss_grad (16 x the block's float64 level x its
    largest gradient): once for the device's rounding, once for the parameters already differing by the earlier steps."""
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    from cosmoprimo_amd.emulators.tools import mlp
    X, Y = toy
    lr = 1e-2
    engine = MLPEmulatorEngine(nhidden=(16, 16), device='cuda:0').fit(X, Y, {}, batch_frac=(0.33,), epochs=1, learning_rate=lr, patience=5, seed=42)
    assert engine.history[0]['epochs'] == 1 and engine.history[0]['batch_size'] == 76
    dims, activations = (3, 16, 16, 8), ['silu', 'silu']
    Xs, Ys = mlp.apply_operations(engine.xoperations, X), mlp.apply_operations(engine.yoperations, Y)
    index1, index2 = mlp.split_indices(np.random.RandomState(seed=42), len(X), 0.1)
    slices = mlp.batch_slices(len(index2), 0.33)
    assert len(slices) == 3
    p = engine.initial_parameters(3, 8, seed=42)
    m, v, tol = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    for step, sl in enumerate(slices, 1):
        Xb, Yb = Xs[index2][sl], Ys[index2][sl]
        levels, _, (_, g) = mr.gradient_levels(p, dims, activations, Xb, Yb)
        dg = np.zeros_like(p)
        for name, block in mr.blocks(dims).items():
            dg[block] = 2 * 16 * levels[name][0] * levels[name][1]
        p, m, v = mr.adam(p, m, v, g, lr, step)
        tol += lr * np.minimum(2., 3 * dg / (np.sqrt(v / (1. - 0.999**step)) + 1e-8))
    silent = mr.blocks(dims)      # alpha, beta of silu layers: gradient 0, never moved
    for name, block in silent.items():
        if name.startswith('alphabeta'):
            assert not engine.parameters[block].any()
    excess = np.abs(engine.parameters - p) / np.where(tol > 0., tol, 1.)
    print('three steps: largest |difference| %.3g, largest fraction of the propagated tolerance %.3g (tolerance at most %.3g)' % (
        np.abs(engine.parameters - p).max(), excess.max(), tol.max()))
    assert (np.abs(engine.parameters - p) <= tol).all()
    loss = mr.loss_grad(p, dims, activations, Xs[index1], Ys[index1])[0]
    assert abs(engine.history[0]['best_loss'] - loss) <= 1e-9 * loss


def torch_training(Xs, Ys, index1, index2, slices, p0, dims, epochs, lr):
    """The same training with torch on the CPU in float64: autograd and torch.optim.Adam; (initial, best) validation loss."""
    import torch
    layers = []
    for kernel, bias, alpha, beta in mr.unpack(p0, dims):
        layers.append([torch.tensor(kernel.copy(), requires_grad=True), torch.tensor(bias.copy(), requires_grad=True)])
    params = [t for layer in layers for t in layer]
    Xt, Yt, Xv, Yv = (torch.tensor(a) for a in (Xs[index2], Ys[index2], Xs[index1], Ys[index1]))

    def model(x):
        for kernel, bias in layers[:-1]:
            x = x @ kernel + bias
            x = x / (1 + torch.exp(-x))
        return x @ layers[-1][0] + layers[-1][1]

    optimizer = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), eps=1e-8)
    with torch.no_grad():
        initial = float(torch.mean((Yv - model(Xv))**2))
    best = np.inf
    for epoch in range(epochs):
        for sl in slices:
            optimizer.zero_grad()
            torch.mean((Yt[sl] - model(Xt[sl]))**2).backward()
            optimizer.step()
        with torch.no_grad():
            best = min(best, float(torch.mean((Yv - model(Xv))**2)))
    return initial, best


def test_training_reaches_what_torch_reaches(toy):
    """(b) Same split, batches, initial weights and hyper-parameters; trajectories diverge under rounding, so the best validation losses are compared: the
    device's at most 4 times the CPU's, and the CPU's below 1 % of its initial one (a run that learns nothing cannot pass)."""
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    from cosmoprimo_amd.emulators.tools import mlp
    X, Y = toy
    epochs, lr, batch_frac = 80, 1e-2, 0.3
    engine = MLPEmulatorEngine(nhidden=(16, 16), device='cuda:0').fit(X, Y, {}, batch_frac=(batch_frac,), epochs=epochs, learning_rate=lr, patience=epochs, seed=42)
    Xs, Ys = mlp.apply_operations(engine.xoperations, X), mlp.apply_operations(engine.yoperations, Y)
    index1, index2 = mlp.split_indices(np.random.RandomState(seed=42), len(X), 0.1)
    initial, best = torch_training(Xs, Ys, index1, index2, mlp.batch_slices(len(index2), batch_frac), engine.initial_parameters(3, 8, seed=42), (3, 16, 16, 8), epochs, lr)
    print('validation loss: initial %.4g, torch on the CPU %.4g, the device %.4g' % (initial, best, engine.history[0]['best_loss']))
    assert best < 0.01 * initial
    assert engine.history[0]['epochs'] == epochs and engine.history[0]['best_loss'] <= 4. * best


def test_patience(toy):
    """(c) learning_rate = 0: nothing moves, every epoch after the first is one without improvement, so the stage stops after exactly patience = 3 of them
    and returns the initial parameters.  Epochs run: 1 + 3.  The first epoch improves on infinity and sets the counter to 0; the stage ends once the counter
    reaches the patience -- the reference's loop (mlp.py:316-343) does the same and runs 4 epochs here, so "after exactly 3 epochs" is read as three epochs
    without improvement, not three epochs in all."""
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    X, Y = toy
    engine = MLPEmulatorEngine(nhidden=(16, 16), device='cuda:0').fit(X, Y, {}, batch_frac=(0.3,), epochs=1000, learning_rate=0., patience=3, seed=42)
    history = engine.history[0]
    assert history['epochs'] == 1 + 3 and len(set(history['losses'])) == 1 and history['best_loss'] == history['losses'][0]
    assert np.array_equal(engine.parameters, engine.initial_parameters(3, 8, seed=42))


@pytest.fixture(scope='module')
def driver():
    import warnings
    import cosmoprimo_amd as cp
    from cosmoprimo_amd.emulators import Emulator, get_calculator
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        calculator = get_calculator(cp.Cosmology(engine='eisenstein_hu'), section=['background', 'thermodynamics'])
        params = {'Omega_m': (0.28, 0.34), 'h': (0.64, 0.72)}
        emulator = Emulator(calculator, params=params, engine='mlp', nhidden=(16,), yoperation='arcsinh', device='cuda:0')      # (not log10: the radial distance is 0 at z = 0)
        emulator.set_samples(niterations=64)
        emulator.fit(epochs=5, batch_frac=(0.5,), learning_rate=1e-2)
        point = dict(Omega_m=0.325, h=0.70)
        batch = dict(Omega_m=np.linspace(0.29, 0.33, 5), h=np.linspace(0.65, 0.71, 5))
        return dict(calculator=calculator, emulator=emulator, point=point, batch=batch, at_point=calculator(**point), at_batch=calculator(**batch))


def test_driver_keys_and_shapes(driver):
    emulator = driver['emulator']
    assert emulator.samples.attrs['ndropped'] == 0 and len(emulator.samples.matrix()) == 64
    for params, ref in [(driver['point'], driver['at_point']), (driver['batch'], driver['at_batch'])]:
        got = emulator.predict(params)
        assert list(sorted(got)) == list(sorted(ref))
        for key, value in ref.items():
            assert np.shape(got[key]) == np.shape(value), key
        assert np.array_equal(got['background.z'], ref['background.z'])
        assert all(np.isfinite(got[key]).all() for key in emulator.varied_keys)
        again = emulator.to_calculator()(**params)
        assert all(np.array_equal(again[key], got[key]) for key in got)
    assert 'background.z' in emulator.fixed and 'background.comoving_radial_distance' in emulator.varied_keys


def test_driver_save_load(driver, tmp_path):
    from cosmoprimo_amd.emulators import Emulator
    fn = str(tmp_path / 'emulator.npy')
    driver['emulator'].save(fn)
    loaded = Emulator.load(fn, device='cuda:0')
    got, want = loaded.predict(driver['batch']), driver['emulator'].predict(driver['batch'])
    assert sorted(got) == sorted(want) and all(np.array_equal(got[key], want[key]) for key in want)


def test_no_host_sync_in_predict(driver):
    """``predict(device=True)`` can be recorded into a HIP graph and a replay on new parameter values in the same buffers gives exactly what the eager
    call gives (tests/test_taylor_gpu.py::test_no_host_sync_in_predict)."""
    import torch
    emulator = driver['emulator']
    dev = torch.device('cuda', 0)
    values = {'Omega_m': np.linspace(0.285, 0.335, 33), 'h': np.linspace(0.645, 0.715, 33)}
    static = {name: torch.as_tensor(v[:17].copy(), device=dev) for name, v in values.items()}
    fresh = {name: torch.as_tensor(v[16:].copy(), device=dev) for name, v in values.items()}
    key = emulator.varied_keys[0]

    def fn():
        out = emulator.predict({name: v[:] for name, v in static.items()}, device=True)
        assert out[key].shape[0] == 17 and out[key].is_cuda
        return out[key]

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
