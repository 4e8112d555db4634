"""GPU: the MLP emulator on the device (cp_mlp_predict / cp_mlp_loss_grad / cp_mlp_adam, csrc/cp_mlp.hip; cosmoprimo_amd/emulators/tools/mlp.py) against
tests/golden/mlp.npz (the reference's predictions, tools/gen_mlp_golden.py), against a manual backward pass in ``np.longdouble``, against torch's autograd
and Adam on the CPU, and on the package's own batch driver.

Tolerances (tests/mlp_reference.py).  Predict: the derived running bound of the forward pass.  Gradient: per parameter block, 16 times the rounding
level of the float64 numpy backward pass (measured against the longdouble one on the same inputs, relative to the block's largest gradient, floored
at eps): the device sums in another order (MFMA steps of 4, tiles, slices) and has its own exp.  Adam: sqrt and division are correctly rounded and the
kernel rounds every operation once, as numpy does, so the two differ by the rounding of ``1 - b`` products at most; allowed: 4 eps of
``|p| + lr |m_hat| / (sqrt(v_hat) + eps)`` for p and 4 eps of the two terms' magnitudes for m and v."""
import numpy as np
import pytest

import mlp_reference as mr
from mlp_device import device_loss_grad

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


STAGE = dict(batch_frac=0.3, epochs=8, learning_rate=0.1, patience=8)      # one stage whose validation loss rises in its last epoch (test_fit_returns_the_best_state)
DIMS, SILU = (3, 16, 16, 8), ['silu', 'silu']


def fit_stages(X, Y, **second):
    """The stage STAGE, then (if given) a second one."""
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    kwargs = {name: (value, second[name]) if second else (value,) for name, value in STAGE.items()}
    return MLPEmulatorEngine(nhidden=(16, 16), device='cuda:0').fit(X, Y, {}, seed=42, **kwargs)


@pytest.fixture(scope='module')
def one_stage(toy):
    return fit_stages(*toy)


def scaled_splits(engine, X, Y, nstages):
    """The scaled samples and the (validation, training) indices of the first ``nstages`` stages, drawn from one generator as ``fit`` draws them."""
    from cosmoprimo_amd.emulators.tools import mlp
    rng = np.random.RandomState(seed=42)
    return mlp.apply_operations(engine.xoperations, X), mlp.apply_operations(engine.yoperations, Y), [mlp.split_indices(rng, len(X), 0.1) for _ in range(nstages)]


def test_fit_returns_the_best_state(toy, one_stage):
    """(d) At learning rate 0.1 the validation loss of the toy problem falls for seven epochs and rises in the eighth (0.0101 -> 0.0122 in float64 numpy from the
    same weights, split and batches; the margins are percents, rounding moves the fourth digit at most), so the best epoch is neither the first nor the last
    and the state ``fit`` keeps differs from the one it ends in.  The float64 loss of the returned parameters on the stage's validation split must be
    ``best_loss`` (1e-9 relative, as test_first_three_steps compares the same two quantities); the last epoch's loss is percents away from it."""
    X, Y = toy
    history = one_stage.history[0]
    losses = history['losses']
    print('one stage: validation losses %s' % ' '.join('%.5g' % value for value in losses))
    best = int(np.argmin(losses))
    assert history['epochs'] == len(losses) == STAGE['epochs']
    assert 0 < best < len(losses) - 1 and history['best_loss'] == losses[best] and losses[-1] > 1.01 * losses[best]
    Xs, Ys, [(index1, _)] = scaled_splits(one_stage, X, Y, 1)
    loss = mr.loss_grad(one_stage.parameters, DIMS, SILU, Xs[index1], Ys[index1])[0]
    assert abs(history['best_loss'] - loss) <= 1e-9 * loss


def test_next_stage_starts_from_the_best_state_with_a_fresh_split(toy, one_stage):
    """(e) A second stage at learning rate 0 with patience 1 moves nothing and ends after its second epoch (the first improves on infinity), so the two-stage fit
    must return, bit for bit, what the one-stage fit returns: the best state of stage one, not its last.  Its first validation loss is the float64 loss of
    those parameters on the SECOND split drawn from the same generator, and its batch size follows ``batch_slices`` on that split's training part."""
    from cosmoprimo_amd.emulators.tools import mlp
    X, Y = toy
    engine = fit_stages(X, Y, batch_frac=0.5, epochs=1000, learning_rate=0., patience=1)
    first, second = engine.history
    assert first['losses'] == one_stage.history[0]['losses'] and first['batch_size'] == one_stage.history[0]['batch_size']
    assert np.array_equal(engine.parameters, one_stage.parameters)
    assert second['epochs'] == 2 and second['losses'][0] == second['losses'][1] == second['best_loss'] and second['learning_rate'] == 0.
    Xs, Ys, [(first1, _), (index1, index2)] = scaled_splits(engine, X, Y, 2)
    assert not np.array_equal(np.sort(first1), np.sort(index1))      # (the two splits differ, so the loss below tells them apart)
    loss = mr.loss_grad(engine.parameters, DIMS, SILU, Xs[index1], Ys[index1])[0]
    other = mr.loss_grad(engine.parameters, DIMS, SILU, Xs[first1], Ys[first1])[0]
    print('stage two: first validation loss %.6g, float64 on the second split %.6g, on the first split %.6g' % (second['losses'][0], loss, other))
    assert abs(second['losses'][0] - loss) <= 1e-9 * loss and abs(other - loss) > 1e-6 * loss
    slices = mlp.batch_slices(len(index2), 0.5)
    assert second['batch_size'] == slices[0].stop - slices[0].start == 115


def test_next_stage_has_fresh_moments(toy, one_stage):
    """(f) A second stage of one epoch of one batch (batch_frac = 1: the 230 training samples of the second split) is ONE Adam step from the best state of stage
    one, and ``fit`` returns its result (the only epoch improves on infinity).  Restated in float64 numpy with m = v = 0 and step = 1; allowed: the
    propagated tolerance of test_first_three_steps for one step.  Moments carried over from stage one (24 steps at learning rate 0.1) would change
    m_hat / (sqrt(v_hat) + eps) by order 1 and the parameters by order lr = 1e-3."""
    from cosmoprimo_amd.emulators.tools import mlp
    X, Y = toy
    lr = 1e-3
    engine = fit_stages(X, Y, batch_frac=1., epochs=1, learning_rate=lr, patience=1)
    assert engine.history[1]['epochs'] == 1 and engine.history[1]['batch_size'] == 230
    Xs, Ys, [_, (index1, index2)] = scaled_splits(engine, X, Y, 2)
    [sl] = mlp.batch_slices(len(index2), 1.)
    p0 = one_stage.parameters
    levels, _, (_, g) = mr.gradient_levels(p0, DIMS, SILU, Xs[index2][sl], Ys[index2][sl])
    dg = np.zeros_like(p0)
    for name, block in mr.blocks(DIMS).items():
        dg[block] = 2 * 16 * levels[name][0] * levels[name][1]
    p, m, v = mr.adam(p0, np.zeros_like(p0), np.zeros_like(p0), g, lr, 1)
    tol = lr * np.minimum(2., 3 * dg / (np.sqrt(v / (1. - 0.999)) + 1e-8))
    difference, moved = np.abs(engine.parameters - p), np.abs(engine.parameters - p0)
    print('one step of stage two: largest |difference| %.3g (tolerance at most %.3g), the step itself up to %.3g' % (difference.max(), tol.max(), moved.max()))
    assert (difference <= tol).all() and tol.max() < 1e-3 * lr and moved.max() > 0.5 * lr
    loss = mr.loss_grad(p, DIMS, SILU, Xs[index1], Ys[index1])[0]
    assert abs(engine.history[1]['best_loss'] - loss) <= 1e-9 * loss


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
