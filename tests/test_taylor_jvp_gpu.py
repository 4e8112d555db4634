"""GPU: cp_taylor_jvp (csrc/cp_taylor.hip, taylor_jvp_kernel) against the longdouble tangents contracted with the longdouble derivative of the polynomial
(tests/jvp_reference.py).

Tolerance: the rule of tests/test_mlp_jvp_gpu.py (jacobian_reference.assert_within): per (direction, output column) block the device
is allowed 16 x the rounding level of the float64 restatement, floored at 1.1e-16.  Every call (``run``) goes into a buffer with the row stride
ldo = ncols + 3 followed by 64 doubles, all holding a sentinel that must survive; a second call must give the same bits; the inputs must be unchanged.

Cases (jvp_reference.TAYLOR_CASES), one dimension at a time from B = 65, ndim = 3, K = 2, T = 65, M = 257, powers drawn from {0, 1, 2, 3} with one term at
power 15 and term 0 the constant: (B, K) in (63, 1), (64, 1), (22, 3), (43, 3), K in {1, 5, 7, 64, 65}, ndim in {1, 2, 32}, T in {1, 31, 32, 33} (the LDS chunk of
32 terms), M in {1, 255, 256}, and the column ranges (0, 1), (255, 257), (16, 17), which must give the bits of the same columns of the full call.  Then:
identity tangents against cp_taylor_jacobian bit for bit, all-zero powers, NaN / Inf in a parameter or in its tangent component under power 0 (bit for
bit no change) and under power 1 (they propagate)."""
import numpy as np
import pytest

import jacobian_reference as jr
import jvp_reference as pr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def run(cfg, columns=None):
    """out (B, K, ncols) of one call of cp_taylor_jvp, with everything the module docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    (B, K, ndim), (T, M) = cfg['tan'].shape, cfg['derivatives'].shape
    col0, stop = columns or (0, M)
    ncols = stop - col0
    names = ('X', 'center', 'powers', 'derivatives', 'tan')
    host = [np.ascontiguousarray(cfg[name]) for name in names]
    X, center, powers, derivatives, tan = t = [torch.as_tensor(a, device=device) for a in host]
    assert powers.dtype == torch.int32 and X.dtype == torch.float64 and tan.dtype == torch.float64
    ld = ncols + PAD
    results = []
    for _ in range(2):
        out = torch.full((B * K * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        _lib.check(lib.cp_taylor_jvp(X.data_ptr(), B, center.data_ptr(), powers.data_ptr(), ndim, T, int(cfg['powers'].max()), derivatives.data_ptr(), M, col0, ncols,
                                     tan.data_ptr(), K, out.data_ptr(), ld, 0, dv.stream_of(device)))
        torch.cuda.synchronize(device)
        out = out.cpu().numpy()
        assert (out[B * K * ld:] == SENTINEL).all(), 'written past the end'
        out = out[:B * K * ld].reshape(B, K, ld)
        assert (out[:, :, ncols:] == SENTINEL).all(), 'padding overwritten'
        results.append(out[:, :, :ncols].copy())
    assert same_bits(results[0], results[1]), 'two calls differ'
    for name, before, after in zip(names, host, t):
        assert np.array_equal(before, after.cpu().numpy(), equal_nan=True), name      # the inputs are read only
    return results[0]


def jacobian(cfg):
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    device = torch.device('cuda', 0)
    (B, ndim), (T, M) = cfg['X'].shape, cfg['derivatives'].shape
    X, center, powers, derivatives = [torch.as_tensor(np.ascontiguousarray(cfg[name]), device=device) for name in ('X', 'center', 'powers', 'derivatives')]
    jac = torch.empty((B, ndim, M), dtype=torch.float64, device=device)
    _lib.check(_lib.load().cp_taylor_jacobian(X.data_ptr(), B, center.data_ptr(), powers.data_ptr(), ndim, T, int(cfg['powers'].max()), derivatives.data_ptr(), M, 0, M,
                                              jac.data_ptr(), M, 0, dv.stream_of(device)))
    return jac.cpu().numpy()


@pytest.mark.parametrize('options', pr.TAYLOR_CASES, ids=[pr.case_id(case) for case in pr.TAYLOR_CASES])
def test_against_truth(options):
    cfg = pr.taylor_config(**options)
    out_ld, out_64 = pr.taylor_truth(cfg)
    out = run(cfg)
    if cfg['powers'].shape[0] == 1:      # the constant alone: its derivative is exactly 0
        assert not out.any() and not out_ld.any()
    jr.assert_within(out, out_ld, out_64, str(options))


def test_column_ranges():
    cfg = pr.taylor_config()
    out_ld, out_64 = pr.taylor_truth(cfg)
    out = run(cfg)
    for a, b in ((0, 1), (255, 257), (16, 17)):
        o = run(cfg, columns=(a, b))
        assert same_bits(o, out[:, :, a:b]), (a, b)
        jr.assert_within(o, out_ld[:, :, a:b], out_64[:, :, a:b], 'columns [%d, %d)' % (a, b))


def test_identity_tangents_are_the_jacobian():
    """K = ndim identity tangents: the bits of cp_taylor_jacobian (the rows are wired to the right points and directions)."""
    for options in (dict(K=3), dict(B=22, K=3), dict(ndim=32, K=32, B=5), dict(ndim=2, K=2, T=33)):
        cfg = pr.taylor_config(**options)
        B, ndim = cfg['X'].shape
        cfg['tan'] = np.broadcast_to(np.eye(ndim), (B, ndim, ndim)).copy()
        assert same_bits(run(cfg), jacobian(cfg)), options


def test_all_zero_powers():
    """A term with every power 0 gives a zero column of the left operand: coefficients of 1e300 in such terms leave the bits of the result as they are with
    coefficients 0 (NaN coefficients would not: 0 x NaN); and a polynomial of such terms alone has the derivative exactly 0."""
    cfg = pr.taylor_config(B=22, K=3, T=33)
    cfg['powers'][[0, 7, 32]] = 0
    zero, huge = cfg['derivatives'].copy(), cfg['derivatives'].copy()
    zero[[0, 7, 32]], huge[[0, 7, 32]] = 0., 1e300
    assert same_bits(run(dict(cfg, derivatives=zero)), run(dict(cfg, derivatives=huge)))
    cfg['powers'][:] = 0
    assert not run(cfg).any()


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_nan_and_inf_under_power_0_and_1(bad):
    """Parameter 1 only ever has power 0: NaN / Inf in it, or in its tangent component, change no bit.  Parameter 2 has powers 0 and 1 only: a bad value
    in it at point 7 reaches the rows of point 7 (through the terms of the other parameters that carry it as a factor) and no other point; a bad tangent
    component (21, 1, 2) -- row 64, the first of the second tile -- reaches exactly that row."""
    cfg = pr.taylor_config(B=22, K=3)
    cfg['powers'][:, 1] = 0
    cfg['powers'][:, 2] = np.minimum(cfg['powers'][:, 2], 1)
    assert (cfg['powers'][:, 2] == 1).any() and (cfg['powers'][cfg['powers'][:, 2] == 1, 0] > 0).any()
    clean = run(cfg)
    assert np.isfinite(clean).all()
    X, tan = cfg['X'].copy(), cfg['tan'].copy()
    X[7, 1] = X[21, 1] = bad
    tan[3, :, 1] = tan[21, 1, 1] = bad
    assert same_bits(run(dict(cfg, X=X, tan=tan)), clean)
    X = cfg['X'].copy()
    X[7, 2] = bad
    out = run(dict(cfg, X=X))
    hit = np.arange(22) == 7
    assert not np.isfinite(out[hit]).any() and same_bits(out[~hit], clean[~hit])
    tan = cfg['tan'].copy()
    tan[21, 1, 2] = bad
    out = run(dict(cfg, tan=tan))
    hit = np.zeros((22, 3), dtype=bool)
    hit[21, 1] = True
    assert not np.isfinite(out[hit]).any() and same_bits(out[~hit], clean[~hit])


def test_engine(golden):
    """TaylorEmulatorEngine.jvp: shapes, ``columns``, ``return_value``, host and device tangents, and the truth on a golden (fitted) configuration."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    g = golden('taylor')
    engine = TaylorEmulatorEngine.from_state({'center': g['c0_center'], 'powers': g['c0_powers'], 'derivatives': g['c0_derivatives']}, device='cuda:0')
    X = g['c0_Xq']
    M = g['c0_derivatives'].shape[1]
    tan = np.random.default_rng(0).normal(0., 1., (len(X), 4, 3))
    out = engine.jvp(X, tan)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (len(X), 4, M) and out.is_contiguous()
    value, out2 = engine.jvp(X, torch.as_tensor(tan, device='cuda:0'), return_value=True)
    assert torch.equal(out2, out) and torch.equal(value, engine.predict(X))
    single = engine.jvp(X, tan[:, 2])
    assert tuple(single.shape) == (len(X), M) and torch.equal(single, out[:, 2])
    value, outc = engine.jvp(torch.as_tensor(X, device='cuda:0'), tan, columns=(2, M - 1), return_value=True)
    assert torch.equal(outc, out[:, :, 2:M - 1]) and torch.equal(value, engine.predict(X, columns=(2, M - 1)))
    assert torch.equal(engine.jvp(X, np.broadcast_to(np.eye(3), (len(X), 3, 3))), engine.jacobian(X))
    out_ld, out_64 = pr.taylor_truth(dict(center=g['c0_center'], powers=g['c0_powers'], derivatives=g['c0_derivatives'], X=X, tan=tan))
    jr.assert_within(out.cpu().numpy(), out_ld, out_64, 'golden configuration 0')
    with pytest.raises(ValueError):
        engine.jvp(X, tan, columns=(3, 3))
    with pytest.raises(ValueError):
        engine.jvp(X, tan[:, :, :-1])
