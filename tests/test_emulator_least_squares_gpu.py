"""GPU: Emulator.least_squares on the emulators of tests/test_emulator_gauss_newton_gpu.py (a Taylor emulator of order 3 and the golden MLP on the toy
calculator, its curve cut into 'head', 'middle', 'tail' beside 'product'): 64 Levenberg-Marquardt fits at once.  Noise-free data (that file's setup) comes
down by the project's four decades in every fit; with noise of 1 % of the mean output the results are the bits ``gauss_newton`` returns at the best point,
``covariance @ fisher`` is the identity by the level rule of tests/lm_reference.py and every parameter is inside its bounds; with the truth of ``c`` outside
the box the fit ends exactly on the bound with the gradient pointing out; ``least_squares`` is the alternation of ``gauss_newton(device=True)`` and
``lm_step`` bit for bit; a converged fit is left alone by further iterations; and ``device=True`` records into a HIP graph (no host synchronisation)."""
import numpy as np
import pytest

import lm_reference as lr
import mlp_reference as mr
from test_emulator_gauss_newton_gpu import KEYS, NAMES, batch, emulators  # noqa: F401

pytestmark = pytest.mark.gpu
LD = np.longdouble
B = 64
LO, HI = (np.array([mr.TOY_LIMITS[name][side] for name in NAMES]) for side in (0, 1))


def problem(emulator, noise=0., outside=False):
    """(start, weights, data) of the 64 fits: the data is the emulator's own prediction at 64 points (``outside``: ``c`` at 0.65, beyond its box, for the odd
    fits) plus ``noise`` standard deviations, the weights 1 / (1 % of the mean output)^2, the starts those points moved by up to 5 % of each range."""
    truth = batch(B, seed=7)
    start = {name: truth[name] + 0.05 * (mr.TOY_LIMITS[name][1] - mr.TOY_LIMITS[name][0]) * np.random.default_rng(8).uniform(-1., 1., B) for name in NAMES}
    if outside:
        truth['c'][1::2] = 0.65
    data = emulator.predict(truth, keys=KEYS)
    sigma = {key: 1e-2 * np.abs(data[key]).mean() for key in KEYS}
    rng = np.random.default_rng(9)
    weights = {key: np.full(data[key].shape, 1. / sigma[key]**2) for key in KEYS}
    data = {key: data[key] + noise * sigma[key] * rng.standard_normal(data[key].shape) for key in KEYS}
    return start, weights, data


def clipped(start):
    return {name: np.clip(start[name], *mr.TOY_LIMITS[name]) for name in NAMES}


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_noise_free_data(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator)
    before = emulator.gauss_newton(clipped(start), weights, data=data)[2]
    best, chi2, info = emulator.least_squares(start, weights, data)
    print('%s: chi2 from %.3g .. %.3g to %.3g .. %.3g, status %s, at least %d acceptances' % (which, before.min(), before.max(), chi2.min(), chi2.max(),
                                                                                              np.bincount(info['status'], minlength=4), info['naccepted'].min()))
    assert isinstance(chi2, np.ndarray) and chi2.shape == (B,) and list(best) == NAMES and all(value.shape == (B,) for value in best.values())
    assert info['fisher'].shape == info['covariance'].shape == (B, 3, 3) and list(info['gradient']) == NAMES and info['status'].dtype == np.int32
    assert sorted(info) == ['covariance', 'fisher', 'gradient', 'lambda', 'naccepted', 'status']
    assert (before > 0).all() and (chi2 <= 1e-4 * before).all() and (chi2 <= before).all()
    assert (info['naccepted'] >= 2).all() and (info['status'] != 3).all()


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_noisy_data(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    best, chi2, info = emulator.least_squares(start, weights, data)
    fisher, gradient, again = emulator.gauss_newton(best, weights, data=data)
    assert np.array_equal(again, chi2) and np.array_equal(fisher, info['fisher']) and all(np.array_equal(gradient[name], info['gradient'][name]) for name in NAMES)
    assert all((best[name] >= mr.TOY_LIMITS[name][0]).all() and (best[name] <= mr.TOY_LIMITS[name][1]).all() for name in NAMES)
    assert (info['status'] == 1).sum() > B // 2 and np.isfinite(chi2).all()
    # covariance @ fisher against the identity: the products in longdouble, of the longdouble inverse (the truth), of the float64 restatement and of the device's
    product = lambda inverse: np.einsum('bij,bjk->bik', np.asarray(inverse).astype(LD), fisher.astype(LD))      # noqa: E731
    (inv64, info64), (invld, infold) = lr.spd_inverse(fisher, 'f8'), lr.spd_inverse(fisher, LD)
    assert not info64.any() and np.array_equal(info['covariance'], info['covariance'].transpose(0, 2, 1))
    assert np.abs(product(invld) - np.eye(3)).max() < 1e-12
    lr.assert_within(product(info['covariance']), product(invld), product(inv64), '%s: covariance @ fisher' % which)
    lr.assert_within(info['covariance'], invld, inv64, '%s: covariance' % which)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_bounds(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, outside=True)
    best, chi2, info = emulator.least_squares(start, weights, data, niterations=30)
    # on the bound, the gradient component pointing out of the box.  The Taylor emulator follows the toy, which grows with c: the upper bound.  The golden
    # MLP is a network that was never trained on the toy and is not monotone in c: which bound a fit meets is the network's affair
    c, g = best['c'][1::2], info['gradient']['c'][1::2]
    low, high = mr.TOY_LIMITS['c']
    print('%s: %d fits end on the upper bound of c, %d on the lower' % (which, (c == high).sum(), (c == low).sum()))
    assert (((c == high) & (g > 0.)) | ((c == low) & (g < 0.))).all()
    if which == 'taylor':
        assert (c == high).all()
    assert all((best[name] >= mr.TOY_LIMITS[name][0]).all() and (best[name] <= mr.TOY_LIMITS[name][1]).all() for name in NAMES)
    before = emulator.gauss_newton(clipped(start), weights, data=data)[2]
    assert (chi2[0::2] <= 1e-4 * before[0::2]).all() and (chi2 <= before).all()      # the even fits hold their truth inside
    # bounds of the caller: a narrower box for b, an open one for a; the start is clipped to them
    bounds = {'b': (1.9, 2.1), 'a': (-np.inf, np.inf)}
    best, chi2, info = emulator.least_squares(start, weights, data, bounds=bounds, niterations=5)
    assert (best['b'] >= 1.9).all() and (best['b'] <= 2.1).all() and (best['c'] <= mr.TOY_LIMITS['c'][1]).all()
    best0, chi0, info0 = emulator.least_squares(start, weights, data, bounds=bounds, niterations=1)
    assert np.array_equal(best0['b'], np.clip(start['b'], 1.9, 2.1)) and np.array_equal(best0['a'], start['a']) and (info0['naccepted'] == 1).all()
    with pytest.raises(KeyError):
        emulator.least_squares(start, weights, data, bounds={'d': (0., 1.)})


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_composition_and_frozen_fits(emulators, which):      # noqa: F811
    import torch
    from cosmoprimo_amd.emulators.tools import lm_state, lm_step
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    N = 4
    best, chi2, info = emulator.least_squares(start, weights, data, niterations=N, device=True)
    assert all(torch.is_tensor(value) and value.is_cuda for value in list(best.values()) + [chi2, info['fisher'], info['covariance'], info['status'], info['gradient']['a']])
    lo, hi = torch.as_tensor(LO, device='cuda:0'), torch.as_tensor(HI, device='cuda:0')
    x = torch.clamp(torch.as_tensor(np.stack([start[name] for name in NAMES], axis=1), device='cuda:0'), min=lo, max=hi)
    state = lm_state(x, lambda0=1e-3)
    for iteration in range(N):
        fisher, gradient, c = emulator.gauss_newton({name: x[:, i] for i, name in enumerate(NAMES)}, weights, data=data, device=True)
        x = lm_step(state, {'x': x, 'fisher': fisher, 'gradient': torch.stack([gradient[name] for name in NAMES], dim=1), 'chi2': c}, lo, hi)
    assert torch.equal(state['x'], torch.stack([best[name] for name in NAMES], dim=1)) and torch.equal(state['chi2'], chi2) and torch.equal(state['fisher'], info['fisher'])
    assert torch.equal(state['gradient'], torch.stack([info['gradient'][name] for name in NAMES], dim=1))
    assert all(torch.equal(state[name], info[name]) for name in ('status', 'naccepted', 'lambda'))
    assert int(state['naccepted'].min()) >= 2
    # a fit that has converged after 10 iterations is the same after 15, bit for bit
    ten, fifteen = (emulator.least_squares(start, weights, data, niterations=n) for n in (10, 15))
    done = ten[2]['status'] == 1
    assert done.sum() > B // 2
    flat = lambda result: [result[0][name] for name in NAMES] + [result[1]] + [result[2][name] for name in ('fisher', 'covariance', 'status', 'naccepted', 'lambda')] \
        + [result[2]['gradient'][name] for name in NAMES]      # noqa: E731
    assert all(np.array_equal(a[done], b[done]) for a, b in zip(flat(ten), flat(fifteen)))
    with pytest.raises(ValueError):      # the state is written in place: taken as it is or not at all
        lm_step(dict(state, status=state['status'].to(torch.int64)), {'x': x, 'fisher': fisher, 'gradient': state['gradient'], 'chi2': c}, lo, hi)


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_scalar_parameters_and_errors(emulators, which):      # noqa: F811
    emulator = emulators[which]
    start, weights, data = problem(emulator, noise=1.)
    at = lambda d: {key: value[5] for key, value in d.items()}      # noqa: E731
    point = {name: float(start[name][5]) for name in NAMES}
    best, chi2, info = emulator.least_squares(point, at(weights), at(data))
    assert all(value.shape == () for value in best.values()) and chi2.shape == () and info['fisher'].shape == (3, 3) and info['covariance'].shape == (3, 3)
    assert info['status'].shape == () and info['naccepted'].shape == () and info['lambda'].shape == () and all(g.shape == () for g in info['gradient'].values())
    assert np.isfinite(chi2) and info['status'] == 1
    with pytest.raises(KeyError):
        emulator.least_squares(start, dict(weights, heads=1.), data)
    with pytest.raises(KeyError):
        emulator.least_squares(start, {'head': 1.}, {'head': 1., 'tail': 1.})
    with pytest.raises(ValueError):
        emulator.least_squares(start, weights, {'head': 1.})
    with pytest.raises(ValueError):
        emulator.least_squares(start, weights, None)
    with pytest.raises(ValueError):
        emulator.least_squares({'a': 1.}, weights, data)


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
        best, chi2, info = emulator.least_squares({name: v[:] for name, v in static.items()}, weights, data, niterations=6, device=True)
        assert chi2.is_cuda and tuple(info['covariance'].shape) == (17, 3, 3)
        return torch.cat([torch.stack([best[name] for name in NAMES], dim=1), chi2[:, None], info['lambda'][:, None], info['status'][:, None].to(torch.float64),
                          info['naccepted'][:, None].to(torch.float64), info['fisher'].reshape(17, 9), info['covariance'].reshape(17, 9)], dim=1)

    capture_and_compare(torch, fn, static, fresh)
