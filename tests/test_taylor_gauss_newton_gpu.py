"""GPU: cp_taylor_gauss_newton (csrc/cp_taylor_gauss_newton.hip, taylor_gn_kernel; csrc/cp_gauss_newton.h) against the longdouble contraction of the
longdouble Jacobian and value of the polynomial (tests/gauss_newton_reference.py).

Tolerance (the rule of tests/jacobian_reference.py): per block -- one (i, j) entry of fisher, one i of grad, or chi2, over the batch -- the level is the float64
restatement's largest distance from the truth relative to the block's largest magnitude, floored at 1.1e-16 (held to at most 32 x that floor for every
case here by tests/test_gauss_newton_host.py); the device is allowed 16 x that level.  The cases' polynomials are dyadic, so the Jacobian and the value
are exact in float64 and the level is the contraction's alone.

Every call goes through tests/gauss_newton_device.py ``run``: padded strides, NaN-filled workspace of exactly the announced size, sentinels behind every
output, two calls with the same bits, exact symmetry, fisher without data bit for bit, the value bit for bit cp_taylor_predict_columns (the same kernel
is launched).  The device always gets the poisoned copy of the case: 1e300 in the derivatives outside the range of columns.

Cases (gauss_newton_reference.TAYLOR_CASES), one thing at a time from B = 9, ndim = 3, T = 20 terms of order 3, columns [3, 20) of 25: points per tile (ndim
1, 3, 7, 8, 32 with one tile, one tile + 1 point, idle rows), ncols in {1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 520}, col0 in {0, 3}, shared and per-point
weights and data, orders 1 to 3, T in {1, 20, 31, 32, 33, 70}.  There is one kernel for every B (no switch) and its grid is not capped.  Then: a weight of
exactly 0 on columns of NaN data and infinite derivatives, a NaN parameter under power 0 and under a positive power, the engine, the memory of a call."""
import numpy as np
import pytest

import gauss_newton_device as gd
import gauss_newton_reference as gr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('options', gr.TAYLOR_CASES, ids=[gr.case_id(case) for case in gr.TAYLOR_CASES])
def test_against_truth(options):
    cfg = gr.taylor_config(**options)
    truth, restated, value_ld = gr.taylor_truth(cfg)
    fisher, grad, chi2, value = gd.run('taylor', gr.taylor_poisoned(cfg))
    gr.assert_within((fisher, grad, chi2), truth, restated, str(options))
    if options.get('T', 0) == 1:      # the constant alone
        assert not fisher.any() and not grad.any() and chi2.all()


def test_zero_weight_drops_its_column():
    """Weight exactly 0 on columns whose data is NaN and whose derivatives are infinite (value and Jacobian Inf or NaN): they contribute exactly 0 -- the
    results are finite, within the rule of the truth without those columns, and have the bits of the call where the same columns hold ordinary numbers."""
    cfg = gr.taylor_config(B=22, ncols=65)
    gr.taylor_truth(cfg)      # draws the operands
    a, b = cfg['columns']
    dropped = np.array([0, 15, 16, 40, 63, 64])
    cfg['weights'][:, dropped] = 0.
    cfg['weights'][5, :] = 0.      # and a whole point
    truth, restated, value_ld = gr.taylor_truth(cfg)
    clean = gd.run('taylor', gr.taylor_poisoned(cfg))
    gr.assert_within(clean[:3], truth, restated, 'zero weights')
    assert not clean[0][5].any() and not clean[1][5].any() and clean[2][5] == 0.
    bad = gr.taylor_poisoned(cfg)
    bad['data'] = cfg['data'].copy()
    bad['data'][:, dropped] = np.nan
    bad['data'][5, :] = np.inf
    bad['derivatives'][:, a + dropped] = np.inf
    got = gd.call('taylor', bad)
    assert all(np.isfinite(r).all() for r in got[:3])
    assert not np.isfinite(got[3][:, dropped]).any()
    assert all(same_bits(x, y) for x, y in zip(got[:3], clean[:3]))


def test_nan_parameter():
    """Parameter 2 only ever has power 0: a NaN there (point 3) changes no bit.  A NaN in a parameter that terms hold (points 7 and 21, the first point of
    the second tile) makes those points' results NaN, and every other point keeps its bits."""
    cfg = gr.taylor_config(B=22)
    cfg['powers'][:, 2] = 0
    gr.taylor_truth(cfg)
    clean = gd.run('taylor', gr.taylor_poisoned(cfg))
    X = cfg['X'].copy()
    X[3, 2] = np.nan
    got = gd.call('taylor', gr.taylor_poisoned(dict(cfg, X=X)))
    assert all(same_bits(g, c) for g, c in zip(got, clean))
    assert cfg['powers'][:, 0].any() and cfg['powers'][:, 1].any()
    X[7, 0] = X[21, 1] = np.nan
    got = gd.call('taylor', gr.taylor_poisoned(dict(cfg, X=X)))
    hit = np.zeros(22, dtype=bool)
    hit[[7, 21]] = True
    for name, g, c in zip(('fisher', 'grad', 'chi2', 'value'), got, clean):
        assert np.isnan(g[hit]).any(axis=tuple(range(1, g.ndim))).all() if g.ndim > 1 else np.isnan(g[hit]).all(), name
        assert same_bits(g[~hit], c[~hit]), name


def test_engine():
    """TaylorEmulatorEngine.gauss_newton: shapes, ``columns``, ``return_value`` equal to ``predict``, host and device operands, shared rows and rows of a
    larger stride, and the refusals."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    cfg = gr.taylor_config(B=22, ncols=65)
    truth, restated, value_ld = gr.taylor_truth(cfg)
    engine = TaylorEmulatorEngine.from_state({'center': cfg['center'], 'powers': cfg['powers'], 'derivatives': cfg['derivatives']}, device='cuda:0')
    a, b = cfg['columns']
    X, ndim = cfg['X'], cfg['X'].shape[1]
    value, fisher, grad, chi2 = engine.gauss_newton(X, cfg['weights'], data=cfg['data'], columns=(a, b), return_value=True)
    assert all(isinstance(r, torch.Tensor) and r.is_cuda and r.is_contiguous() for r in (value, fisher, grad, chi2))
    assert tuple(fisher.shape) == (22, ndim, ndim) and tuple(grad.shape) == (22, ndim) and tuple(chi2.shape) == (22,)
    assert torch.equal(value, engine.predict(X, columns=(a, b)))
    gr.assert_within((fisher.cpu().numpy(), grad.cpu().numpy(), chi2.cpu().numpy()), truth, restated, 'engine')
    only = engine.gauss_newton(torch.as_tensor(X, device='cuda:0'), torch.as_tensor(cfg['weights'], device='cuda:0'), columns=(a, b))
    assert isinstance(only, torch.Tensor) and torch.equal(only, fisher)
    wide = torch.zeros((22, b - a + 9), dtype=torch.float64, device='cuda:0')      # rows of a larger stride, read in place
    wide[:, :b - a] = torch.as_tensor(cfg['weights'], device='cuda:0')
    f2, g2, c2 = engine.gauss_newton(X, wide[:, :b - a], data=cfg['data'], columns=(a, b))
    assert torch.equal(f2, fisher) and torch.equal(g2, grad) and torch.equal(c2, chi2)
    M = cfg['derivatives'].shape[1]      # every column, one shared row of weights and of data
    w, d = np.linspace(0.5, 2., M), np.asarray(engine.predict(X).cpu().numpy()[0]) * 1.01
    f3, g3, c3 = engine.gauss_newton(X, w, data=d)
    f4, g4, c4 = engine.gauss_newton(X, np.tile(w, (22, 1)), data=np.tile(d, (22, 1)))
    assert torch.equal(f3, f4) and torch.equal(g3, g4) and torch.equal(c3, c4) and bool(torch.isfinite(f3).all())
    with pytest.raises(ValueError):
        engine.gauss_newton(X, cfg['weights'], columns=(3, 3))
    with pytest.raises(ValueError):
        engine.gauss_newton(X, cfg['weights'][:, :-1], columns=(a, b))
    with pytest.raises(ValueError):
        engine.gauss_newton(X, cfg['weights'], data=cfg['data'][:-1], columns=(a, b))


def test_no_jacobian_in_memory():
    """At B = 4096, ndim = 8, ncols = 1024 the peak of allocated memory over a call rises by less than half of the B ndim ncols doubles of a Jacobian: the value
    is an eighth of it and the column tiles' partial sums about 3 %."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    B, ndim, M = 4096, 8, 1024
    cfg = gr.taylor_config(B=B, ndim=ndim, T=45, order=2, col0=0, ncols=M - 5)
    engine = TaylorEmulatorEngine.from_state({'center': cfg['center'], 'powers': cfg['powers'], 'derivatives': cfg['derivatives']}, device='cuda:0')
    X = torch.as_tensor(cfg['X'], device='cuda:0')
    w, d = torch.ones((M,), dtype=torch.float64, device='cuda:0'), torch.zeros((M,), dtype=torch.float64, device='cuda:0')
    engine.gauss_newton(X, w, data=d)      # (the device state is set)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = engine.gauss_newton(X, w, data=d, return_value=True)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print('peak rise %.1f MB, a Jacobian %.1f MB' % (rise / 1e6, B * ndim * M * 8 / 1e6))
    assert rise < B * ndim * M * 8 // 2 and bool(torch.isfinite(out[1]).all())
