"""GPU: cp_taylor_vjp (csrc/cp_taylor.hip: the GEMM with the front end of the fit on the transposed derivatives, then taylor_input_grad_kernel) against
the longdouble reverse pass of tests/vjp_reference.py.

Tolerance: the rule of tests/test_mlp_vjp_gpu.py (vjp_reference.assert_within): per entry 16 level 2^-53 A[b, i], A the magnitude
pass sum_t |d mono_t / d x_i| sum_c |cot| |D|, level measured over three float64 orders for the very case.  Every call (``run``) reads a cotangent with the
row stride ncols + 3 (the padding NaN), writes G followed by 64 sentinels and gets a workspace of exactly cp_taylor_vjp_workspace_doubles filled with
NaN and followed by 64 sentinels; a second call must give the same bits and the inputs must be unchanged.

Cases, one dimension at a time from B = 65, ndim = 3, T = 65, M = 257 (the polynomial of tests/test_taylor_jacobian_gpu.py): B in {1, 64}, ndim in
{1, 32}, T in {1, 32, 33, 64, 257} (the 64 columns of a wave of the first GEMM, a second column tile), M in {1, 4, 5} (one MFMA step of the contraction,
a masked one), and the column ranges (0, 1), (255, 257), (16, 200)."""
import numpy as np
import pytest

import vjp_reference as vr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def run(cfg, cot=None, columns=None):
    """G (B, ndim) of one call of cp_taylor_vjp, with everything the module docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    (B, ndim), (T, M) = cfg['X'].shape, cfg['derivatives'].shape
    col0, stop = columns or (0, M)
    ncols = stop - col0
    cot = cfg['cot'][:, col0:stop] if cot is None else cot
    ld = ncols + PAD
    padded = np.full((B, ld), np.nan)
    padded[:, :ncols] = cot
    names = ('X', 'center', 'powers', 'derivatives_t', 'cot')
    host = [np.ascontiguousarray(cfg[name]) for name in names[:3]] + [np.ascontiguousarray(cfg['derivatives'].T), padded]
    X, center, powers, derivatives_t, cotd = t = [torch.as_tensor(a, device=device) for a in host]
    assert powers.dtype == torch.int32 and X.dtype == torch.float64
    need = int(lib.cp_taylor_vjp_workspace_doubles(B, T))
    assert need == B * T
    results = []
    for _ in range(2):
        grad = torch.full((B * ndim + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        work = torch.full((need + TAIL,), np.nan, dtype=torch.float64, device=device)
        work[need:] = SENTINEL
        _lib.check(lib.cp_taylor_vjp(X.data_ptr(), B, center.data_ptr(), powers.data_ptr(), ndim, T, int(cfg['powers'].max()), derivatives_t.data_ptr(), M, col0, ncols,
                                     cotd.data_ptr(), ld, grad.data_ptr(), work.data_ptr(), need, 0, dv.stream_of(device)))
        torch.cuda.synchronize(device)
        grad, work = grad.cpu().numpy(), work.cpu().numpy()
        assert (grad[B * ndim:] == SENTINEL).all() and (work[need:] == SENTINEL).all(), 'written past the end'
        results.append(grad[:B * ndim].reshape(B, ndim).copy())
    assert same_bits(results[0], results[1]), 'two calls differ'
    for name, before, after in zip(names, host, t):
        assert np.array_equal(before, after.cpu().numpy(), equal_nan=True), name      # the inputs are read only
    return results[0]


@pytest.mark.parametrize('options', vr.TAYLOR_CASES, ids=[vr.case_id(case) for case in vr.TAYLOR_CASES])
def test_against_truth(options):
    cfg = vr.taylor_config(**options)
    G_ld, A, level = vr.taylor_case(cfg, cfg['cot'])
    G = run(cfg)
    if cfg['powers'].shape[0] == 1:      # the constant alone: its derivative is exactly 0
        assert not G.any() and not G_ld.any()
    vr.assert_within(G, G_ld, A, level, str(options))


def test_column_ranges():
    cfg = vr.taylor_config()
    for a, b in ((0, 1), (255, 257), (16, 200)):
        cot = cfg['cot'][:, a:b]
        G_ld, A, level = vr.taylor_case(cfg, cot, columns=(a, b))
        vr.assert_within(run(cfg, columns=(a, b)), G_ld, A, level, 'columns [%d, %d)' % (a, b))
        full = np.zeros_like(cfg['cot'])
        full[:, a:b] = cot
        vr.assert_within(run(cfg, cot=full), G_ld, A, level, 'the full call, zero outside [%d, %d)' % (a, b))


def test_all_zero_powers():
    """Every power 0: the polynomial is a constant and G exactly 0, whatever the coefficients, the cotangent and the points hold."""
    cfg = vr.taylor_config(B=22, T=33)
    cfg['powers'][:] = 0
    cfg['X'][3] = np.nan
    cfg['cot'][5, 7] = np.inf
    cfg['derivatives'][4, 9] = np.nan
    assert not run(cfg).any()


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_nan_and_inf_in_a_parameter(bad):
    """Parameter 1 is under power 0 in every term: NaN / Inf in it leaves G what it was, bit for bit, its own entry exactly 0.  Parameter 2 is under powers
    <= 1: with NaN / Inf in it at point 21 the entry of parameter 2 itself drops the factor and stays finite and within the rule, the other entries of the
    point take it; no other point is touched."""
    cfg = vr.taylor_config(B=22)
    cfg['powers'][:, 1] = 0
    cfg['powers'][:, 2] = np.minimum(cfg['powers'][:, 2], 1)
    clean = run(cfg)
    assert not clean[:, 1].any()
    X = cfg['X'].copy()
    X[7, 1] = bad
    assert same_bits(run(dict(cfg, X=X)), clean)
    X[21, 2] = bad
    G = run(dict(cfg, X=X))
    keep = np.arange(22) != 21
    assert same_bits(G[keep], clean[keep])
    assert not np.isfinite(G[21, 0]) and G[21, 1] == 0. and np.isfinite(G[21, 2])
    with np.errstate(invalid='ignore'):
        G_ld, A, level = vr.taylor_case(dict(cfg, X=np.where(np.isfinite(X), X, 0.)), cfg['cot'])      # (entry (21, 2) holds no factor of x_2)
    assert abs(G[21, 2] - G_ld[21, 2]) <= vr.ALLOW * level * vr.EPS * A[21, 2]


def test_nan_in_the_cotangent():
    cfg = vr.taylor_config(B=66)
    clean = run(cfg)
    cot = cfg['cot'].copy()
    cot[64, 3] = np.nan
    G = run(cfg, cot=cot)
    keep = np.arange(66) != 64
    assert np.isnan(G[64]).all() and same_bits(G[keep], clean[keep])


def test_engine(golden):
    """TaylorEmulatorEngine.vjp: shapes, ``columns``, ``return_value``, a strided cotangent, and the truth on a golden (fitted) configuration."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    g = golden('taylor')
    engine = TaylorEmulatorEngine.from_state({'center': g['c0_center'], 'powers': g['c0_powers'], 'derivatives': g['c0_derivatives']}, device='cuda:0')
    X = g['c0_Xq']
    M = g['c0_derivatives'].shape[1]
    cot = np.random.default_rng(0).normal(0., 1., (len(X), M))
    G = engine.vjp(X, cot)
    assert isinstance(G, torch.Tensor) and G.is_cuda and tuple(G.shape) == (len(X), 3) and G.is_contiguous()
    value, G2 = engine.vjp(X, cot, return_value=True)
    assert torch.equal(G2, G) and torch.equal(value, engine.predict(X))
    cotd = torch.as_tensor(cot, device='cuda:0')
    value, Gc = engine.vjp(torch.as_tensor(X, device='cuda:0'), cotd[:, 2:M - 1], columns=(2, M - 1), return_value=True)      # (a view with the row stride M)
    assert torch.equal(value, engine.predict(X, columns=(2, M - 1))) and torch.equal(Gc, engine.vjp(X, cot[:, 2:M - 1].copy(), columns=(2, M - 1)))
    c = dict(center=g['c0_center'], powers=g['c0_powers'], derivatives=g['c0_derivatives'], X=X)
    G_ld, A, level = vr.taylor_case(c, cot)
    vr.assert_within(G.cpu().numpy(), G_ld, A, level, 'golden configuration 0')
    G_ld, A, level = vr.taylor_case(c, cot[:, 2:M - 1], columns=(2, M - 1))
    vr.assert_within(Gc.cpu().numpy(), G_ld, A, level, 'golden configuration 0, columns')
    with pytest.raises(ValueError):
        engine.vjp(X, cot[:, :0], columns=(3, 3))
    with pytest.raises(ValueError):
        engine.vjp(X, cot[:, 1:])
