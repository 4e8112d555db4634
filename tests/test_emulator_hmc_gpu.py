"""GPU: Emulator.hmc.  On the emulators of tests/test_emulator_gauss_newton_gpu.py (a Taylor emulator of order 3 and the golden MLP on the toy calculator) with
the noisy data of tests/test_emulator_least_squares_gpu.py: ``hmc`` is the alternation of ``gauss_newton(device=True)`` and ``hmc_step`` bit for bit; the same
seed gives the same bits and another seed other samples; a diagonal ``precision`` agrees with the ``weights`` route over one trajectory by the level rule of
tests/hmc_reference.py; scalar parameters drop the batch axis; the argument errors are those of ``least_squares``; and ``device=True`` records into a HIP
graph (no host synchronisation).  On Taylor emulators of order 1 of calculators linear in 2 and in 3 parameters with Gaussian data
(``hmc_reference.LinearModel``: the posterior is a known Gaussian): 4096 chains from the least-squares mode, whitened with the exact posterior after 20
trajectories, have a mean within 5 / sqrt(B) = 0.078 of zero and a covariance within 5 sqrt(2 / B) = 0.11 of the identity, with a mean acceptance above 0.9;
and with a bound through the posterior's bulk every sample lies inside the box, trajectories leave it (``nout``) and the acceptance is lower."""
import functools

import numpy as np
import pytest

import hmc_reference as hr
import mlp_reference as mr
from test_emulator_gauss_newton_gpu import KEYS, NAMES, emulators  # noqa: F401
from test_emulator_least_squares_gpu import problem

pytestmark = pytest.mark.gpu
LD = np.longdouble
LO, HI = (np.array([mr.TOY_LIMITS[name][side] for name in NAMES]) for side in (0, 1))
B_EXACT = 4096
RUN = dict(nsamples=3, nwarmup=2, thin=2, nleapfrog=3, seed=11)


def stacked(d, names=NAMES):
    import torch
    return torch.stack([d[name] for name in names], dim=-1) if torch.is_tensor(d[names[0]]) else np.stack([d[name] for name in names], axis=-1)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_composition(emulators, which):      # noqa: F811
    import torch
    from cosmoprimo_amd.emulators.tools import hmc_factor, hmc_state, hmc_step
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    B = len(start['a'])
    samples, chi2, info = emulator.hmc(start, weights, data, device=True, **RUN)
    assert all(torch.is_tensor(value) and value.is_cuda for value in list(samples.values()) + [chi2] + list(info.values()))
    assert list(samples) == NAMES and all(tuple(value.shape) == (3, B) for value in samples.values()) and tuple(chi2.shape) == (3, B)
    assert sorted(info) == ['acceptance', 'metric', 'naccepted', 'nout', 'status', 'step_size'] and tuple(info['metric'].shape) == (B, 3, 3)
    lo, hi = torch.as_tensor(LO, device='cuda:0'), torch.as_tensor(HI, device='cuda:0')

    def evaluate(x):
        fisher, gradient, c = emulator.gauss_newton({name: x[:, i] for i, name in enumerate(NAMES)}, weights, data=data, device=True)
        return fisher, stacked(gradient), c

    x = torch.clamp(torch.as_tensor(stacked(start), device='cuda:0'), min=lo, max=hi)
    fisher0, gradient, c = evaluate(x)
    state = hmc_state(x, gradient, c)
    factor = hmc_factor(fisher0, state['status'])
    ntrajectories = RUN['nwarmup'] + RUN['nsamples'] * RUN['thin']
    kept, kept_chi2 = torch.zeros((RUN['nsamples'], B, 3), dtype=torch.float64, device='cuda:0'), torch.zeros((RUN['nsamples'], B), dtype=torch.float64, device='cuda:0')
    controls = dict(jitter=0.1, seed=RUN['seed'])
    x = hmc_step(state, {'x': state['x'], 'gradient': state['gradient'], 'chi2': state['chi2']}, factor, lo, hi, 0.25, t_open=0, **controls)
    for t in range(ntrajectories):
        for leap in range(RUN['nleapfrog']):
            fisher, gradient, c = evaluate(x)
            trial = {'x': x, 'gradient': gradient, 'chi2': c}
            if leap < RUN['nleapfrog'] - 1:
                x = hmc_step(state, trial, factor, lo, hi, 0.25, **controls)
            else:
                s = {3: 0, 5: 1, 7: 2}.get(t)      # every second trajectory after the two of the warm-up
                x = hmc_step(state, trial, factor, lo, hi, 0.25, t_close=t, t_open=t + 1 if t + 1 < ntrajectories else None,
                             sample=kept[s] if s is not None else None, sample_chi2=kept_chi2[s] if s is not None else None, **controls)
    assert torch.equal(kept, stacked(samples)) and torch.equal(kept_chi2, chi2)
    assert all(torch.equal(state[name], info[name]) for name in ('naccepted', 'nout', 'status'))
    assert torch.equal(info['acceptance'], state['naccepted'].to(torch.float64) / ntrajectories) and torch.equal(info['metric'], fisher0)
    assert torch.equal(kept[-1], state['x']) and torch.equal(kept_chi2[-1], state['chi2'])
    assert int(state['naccepted'].sum()) > B * ntrajectories // 2 and not bool(state['status'].any())
    assert bool(((kept >= lo) & (kept <= hi)).all())
    # host arrays by default: the same numbers
    host = emulator.hmc(start, weights, data, **RUN)
    assert isinstance(host[1], np.ndarray) and np.array_equal(host[1], chi2.cpu().numpy()) and np.array_equal(stacked(host[0]), kept.cpu().numpy())
    assert np.array_equal(host[2]['naccepted'], state['naccepted'].cpu().numpy()) and host[2]['status'].dtype == np.int32
    with pytest.raises(ValueError):      # the state is written in place: taken as it is or not at all
        hmc_step(dict(state, out=state['out'].to(torch.int64)), trial, factor, lo, hi, 0.25)
    with pytest.raises(ValueError):
        hmc_step(state, trial, factor, lo, hi, 0.25, t_close=0, sample=kept[0])


class Linear(object):
    """A Taylor emulator of order 1 of ``hmc_reference.LinearModel(ndim)`` in a box of 10 posterior standard deviations around the mode."""

    def __init__(self, ndim):
        from cosmoprimo_amd.emulators import Emulator
        self.model = model = hr.LinearModel(ndim)
        self.names = ['p%d' % i for i in range(ndim)]
        lo, hi = model.limits(10.)
        self.limits = {name: (float(lo[i]), float(hi[i])) for i, name in enumerate(self.names)}

        def calculator(**params):
            theta = np.stack(np.broadcast_arrays(*[np.asarray(params[name], dtype='f8') for name in self.names]), axis=-1)
            return {'y': model.predict(theta)}

        self.emulator = Emulator(calculator, params=self.limits, engine='taylor', order=1, device='cuda:0')
        self.emulator.set_samples()
        self.emulator.fit()
        self.weights, self.data = {'y': model.weights}, {'y': model.data}
        centre = {name: 0.5 * (self.limits[name][0] + self.limits[name][1]) + 0.1 for name in self.names}
        best, chi2, info = self.emulator.least_squares(centre, self.weights, self.data)
        self.mode = np.array([best[name] for name in self.names])
        # the emulator's mode is the model's, as far as finite differences give the derivatives: 1e-3 standard deviations are nothing beside 5 / sqrt(B)
        assert info['status'] == 1 and np.abs(model.whiten(self.mode[None])).max() < 1e-3

    def hmc(self, B=B_EXACT, **kwargs):
        start = {name: np.full(B, self.mode[i]) for i, name in enumerate(self.names)}
        samples, chi2, info = self.emulator.hmc(start, self.weights, self.data, **dict(dict(nsamples=1, nwarmup=20, seed=42), **kwargs))
        return stacked(samples, self.names), chi2, info


@functools.lru_cache(maxsize=None)
def linear(ndim):
    return Linear(ndim)


@functools.lru_cache(maxsize=None)
def exact_run(ndim):
    return linear(ndim).hmc()


@pytest.mark.parametrize('ndim', [2, 3])
def test_exactness(ndim):
    model = linear(ndim).model
    samples, chi2, info = exact_run(ndim)
    assert samples.shape == (1, B_EXACT, ndim) and chi2.shape == (1, B_EXACT) and not info['nout'].any() and not info['status'].any()
    w = model.whiten(samples[0])
    mean, cov = w.mean(axis=0), np.cov(w.T, bias=True)
    print('ndim = %d: |mean| at most %.3f, covariance at most %.3f from the identity, acceptance %.3f' % (ndim, np.abs(mean).max(), np.abs(cov - np.eye(ndim)).max(),
                                                                                                          info['acceptance'].mean()))
    assert np.abs(mean).max() < 5. / np.sqrt(B_EXACT) and np.abs(cov - np.eye(ndim)).max() < 5. * np.sqrt(2. / B_EXACT)
    assert info['acceptance'].mean() > 0.9 and np.abs(info['acceptance'] - info['naccepted'] / 21.).max() < 1e-15      # (the device's division, numpy's)
    again = linear(ndim).hmc()      # deterministic under its seed
    assert np.array_equal(again[0], samples) and np.array_equal(again[1], chi2) and np.array_equal(again[2]['naccepted'], info['naccepted'])
    # chi2 is the emulator's at the samples and the default metric the Fisher matrix at the start: the model's, as far as finite differences go
    assert np.abs(chi2[0] - model.evaluate(samples[0])[2]).max() < 1e-3 * chi2.max()
    assert np.abs(info['metric'] - model.fisher).max() < 1e-3 * np.abs(model.fisher).max() and (info['step_size'] == 0.25).all()
    # the first chains of the batch are the chains of a shorter batch
    few = linear(ndim).hmc(B=100)
    assert np.array_equal(few[0][0], samples[0, :100]) and np.array_equal(few[2]['naccepted'], info['naccepted'][:100])


def test_box():
    setup = linear(2)
    mode0 = float(setup.mode[0])
    bounds = {'p0': (setup.limits['p0'][0], mode0)}      # the upper half of p0 is cut away: the bound goes through the mode
    samples, chi2, info = setup.hmc(nsamples=4, nwarmup=5, bounds=bounds)
    assert samples.shape == (4, B_EXACT, 2) and (samples[..., 0] <= mode0).all() and (samples[..., 0] >= setup.limits['p0'][0]).all()
    assert (samples[..., 1] >= setup.limits['p1'][0]).all() and (samples[..., 1] <= setup.limits['p1'][1]).all()
    free = exact_run(2)[2]
    print('a bound through the mode: %d of %d trajectories left the box, acceptance %.3f against %.3f' % (info['nout'].sum(), 9 * B_EXACT, info['acceptance'].mean(),
                                                                                                          free['acceptance'].mean()))
    assert info['nout'].sum() > 0 and (info['nout'] + info['naccepted'] <= 9).all() and info['acceptance'].mean() < free['acceptance'].mean()
    assert (samples[-1, :, 0] < mode0).mean() > 0.9 and not info['status'].any()      # the chains have left the bound they started on
    with pytest.raises(KeyError):
        setup.hmc(B=4, bounds={'q': (0., 1.)})


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_seeds(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    one, two, other = (emulator.hmc(start, weights, data, **dict(RUN, seed=seed)) for seed in (11, 11, 12))
    assert np.array_equal(stacked(one[0]), stacked(two[0])) and np.array_equal(one[1], two[1]) and np.array_equal(one[2]['naccepted'], two[2]['naccepted'])
    assert not np.array_equal(stacked(one[0]), stacked(other[0])) and (stacked(one[0])[0] != stacked(other[0])[0]).any(axis=-1).mean() > 0.5
    # a seed beyond 32 bits reaches the key's second word
    assert not np.array_equal(stacked(emulator.hmc(start, weights, data, **dict(RUN, seed=11 + 2**32))[0]), stacked(one[0]))


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_precision(emulators, which):      # noqa: F811
    """One trajectory under ``precision=np.diag(w)`` against the restatement (float64, and longdouble for the truth) of the same trajectory on what
    ``gauss_newton`` returns by the ``weights`` route: a block is one chain's sample."""
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    precision = np.diag(np.concatenate([np.ravel(weights[key][0]) for key in KEYS]))

    def evaluate(x):
        fisher, gradient, chi2 = emulator.gauss_newton({name: x[:, i] for i, name in enumerate(NAMES)}, weights, data=data)
        return fisher, stacked(gradient), chi2

    run = dict(nsamples=1, nwarmup=0, nleapfrog=6, seed=5)
    x0 = stacked(start)
    (s64, c64, state64), (sld, cld, stateld) = (hr.run(evaluate, x0, LO, HI, dtype=dtype, **run) for dtype in ('f8', LD))
    assert np.array_equal(state64['naccepted'], stateld['naccepted']) and np.array_equal(state64['nout'], stateld['nout'])
    diagonal = emulator.hmc(start, weights, data, **run)
    dense = emulator.hmc(start, KEYS, data, precision=precision, **run)
    for name, result in (('weights', diagonal), ('precision', dense)):
        assert np.array_equal(result[2]['naccepted'], state64['naccepted']) and np.array_equal(result[2]['nout'], state64['nout']), name
        hr.assert_levels(stacked(result[0])[0], sld[0], s64[0], '%s, %s: a sample after one trajectory' % (which, name))
    assert state64['naccepted'].sum() > len(x0) // 2 and (state64['naccepted'] + state64['nout'] <= 1).all()      # (the toy's box is narrow: some chains leave it)
    with pytest.raises(TypeError):
        emulator.hmc(start, weights, data, precision=precision, **run)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_scalar_parameters_and_errors(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    at = lambda d: {key: value[5] for key, value in d.items()}      # noqa: E731
    point = {name: float(np.clip(start[name][5], *mr.TOY_LIMITS[name])) for name in NAMES}
    samples, chi2, info = emulator.hmc(point, at(weights), at(data), nsamples=4, nwarmup=1, nleapfrog=2)
    assert list(samples) == NAMES and all(value.shape == (4,) for value in samples.values()) and chi2.shape == (4,)
    assert info['metric'].shape == (3, 3) and all(info[name].shape == () for name in ('naccepted', 'nout', 'status', 'acceptance', 'step_size'))
    assert np.isfinite(chi2).all() and info['status'] == 0 and abs(info['acceptance'] - info['naccepted'] / 5.) < 1e-15
    few = dict(nsamples=1, nwarmup=0, nleapfrog=1)
    with pytest.raises(KeyError):
        emulator.hmc(start, dict(weights, heads=1.), data, **few)
    with pytest.raises(KeyError):
        emulator.hmc(start, {'head': 1.}, {'head': 1., 'tail': 1.}, **few)
    with pytest.raises(KeyError):
        emulator.hmc(start, weights, data, bounds={'d': (0., 1.)}, **few)
    with pytest.raises(ValueError):
        emulator.hmc(start, weights, {'head': 1.}, **few)
    with pytest.raises(ValueError):
        emulator.hmc(start, weights, None, **few)
    with pytest.raises(ValueError):
        emulator.hmc({'a': 1.}, weights, data, **few)
    B = len(start['a'])
    for metric in (np.eye(2), np.ones((B, 3)), np.ones((B + 1, 3, 3)), np.ones((B, 3, 2)), 1.):      # a metric of a wrong shape
        with pytest.raises(ValueError):
            emulator.hmc(start, weights, data, metric=metric, **few)
    for bad in (dict(nsamples=0), dict(thin=0), dict(nleapfrog=0), dict(nwarmup=-1), dict(jitter=1.), dict(jitter=-0.5), dict(step_size=np.ones(B + 1))):
        with pytest.raises(ValueError):
            emulator.hmc(start, weights, data, **dict(few, **bad))
    # a metric of the caller, shared or per chain; a step size per chain; a chain that cannot run stays at its start
    fisher = emulator.least_squares(start, weights, data)[2]['fisher']
    shared = emulator.hmc(start, weights, data, metric=fisher[0], **RUN)
    each = emulator.hmc(start, weights, data, metric=fisher, step_size=np.full(B, 0.25), **RUN)
    assert np.array_equal(stacked(shared[0])[:, 0], stacked(each[0])[:, 0]) and np.array_equal(shared[2]['metric'][3], fisher[0]) and np.array_equal(each[2]['metric'], fisher)
    size = np.full(B, 0.25)
    size[1], fisher[2] = np.nan, -fisher[2]
    stuck = emulator.hmc(start, weights, data, metric=fisher, step_size=size, **RUN)
    x0 = np.clip(stacked(start), LO, HI)
    assert list(stuck[2]['status'][:4]) == [0, 3, 3, 0] and all(np.array_equal(stacked(stuck[0])[s, 1:3], x0[1:3]) for s in range(3))
    assert np.array_equal(stacked(stuck[0])[:, 0], stacked(each[0])[:, 0]) and not stuck[2]['naccepted'][1:3].any()


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_no_host_synchronisation(emulators, which):      # noqa: F811
    import torch
    from test_no_host_sync_gpu import capture_and_compare
    emulator = emulators[which]
    dev = torch.device('cuda', 0)
    start, weights, data = problem(emulator, noise=1.)
    static = {name: torch.as_tensor(value[:17], device=dev) for name, value in start.items()}
    fresh = {name: torch.as_tensor(np.clip(value[17:34], *mr.TOY_LIMITS[name]), device=dev) for name, value in start.items()}
    weights, data = ({key: torch.as_tensor(value[:17], device=dev) for key, value in d.items()} for d in (weights, data))

    def fn():
        samples, chi2, info = emulator.hmc({name: v[:] for name, v in static.items()}, weights, data, nsamples=2, nwarmup=1, nleapfrog=2, device=True)
        assert chi2.is_cuda and tuple(info['metric'].shape) == (17, 3, 3)
        rows = lambda v: v.to(torch.float64)[None].expand(2, 17)      # noqa: E731
        return torch.cat([stacked(samples).reshape(2, 17 * 3), chi2] + [rows(info[name]) for name in ('naccepted', 'nout', 'status', 'acceptance', 'step_size')], dim=1)

    capture_and_compare(torch, fn, static, fresh)
