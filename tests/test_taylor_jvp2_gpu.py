"""GPU: cp_taylor_jvp2 (csrc/cp_taylor.hip, the TY_JVP2 front end of csrc/cp_taylor_gemm.h) against the longdouble second directional derivatives of the
polynomial (tests/jvp2_reference.py).

Tolerance: the rule of tests/test_mlp_jvp2_gpu.py (jacobian_reference.assert_within, unchanged): per (pair of directions, output column)
block the device is allowed 16 x the rounding level of the float64 restatement, floored at 1.1e-16 (held to at most 32 floors by tests/test_jvp2_host.py).
Every call (``run``) goes into a buffer with the row stride ldo = ncols + 3 followed by 64 doubles, all holding a sentinel that must survive; a second
call must give the same bits, exchanging the two tangent sets must give the same bits, and the inputs must be unchanged.

Cases (jvp2_reference.TAYLOR_CASES: the shapes of jvp_reference.TAYLOR_CASES, each with v = u and with a second tangent set), one dimension at a time from
B = 65, ndim = 3, K = 2, T = 65, M = 257, powers drawn from {0, 1, 2, 3} with one term at power 15 and term 0 the constant; the column ranges (0, 1),
(255, 257), (16, 17) must give the bits of the same columns of the full call.  Then: unit pairs against the second derivatives of single monomials, exactly;
terms of total order < 2 contribute exactly 0 (T = 1: the constant alone); NaN / Inf in a parameter or in its tangent components under power 0 (bit for bit
no change, the result finite) and under a positive power (they stay in their rows)."""
import numpy as np
import pytest

import jacobian_reference as jr
import jvp2_reference as sr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def call(cfg, columns, tan_u, tan_v):
    """out (B, K, ncols) of one call of cp_taylor_jvp2 with the sentinels checked"""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    (B, K, ndim), (T, M) = tan_u.shape, cfg['derivatives'].shape
    col0, stop = columns or (0, M)
    ncols = stop - col0
    names = ('X', 'center', 'powers', 'derivatives')
    host = [np.ascontiguousarray(cfg[name]) for name in names] + [np.ascontiguousarray(a) for a in (tan_u, tan_v) if a is not None]
    t = [torch.as_tensor(a, device=device) for a in host]
    X, center, powers, derivatives, u = t[:5]
    assert powers.dtype == torch.int32 and X.dtype == torch.float64 and u.dtype == torch.float64
    ld = ncols + PAD
    out = torch.full((B * K * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
    _lib.check(lib.cp_taylor_jvp2(X.data_ptr(), B, center.data_ptr(), powers.data_ptr(), ndim, T, int(cfg['powers'].max()), derivatives.data_ptr(), M, col0, ncols,
                                  u.data_ptr(), t[5].data_ptr() if tan_v is not None else None, K, out.data_ptr(), ld, 0, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    out = out.cpu().numpy()
    assert (out[B * K * ld:] == SENTINEL).all(), 'written past the end'
    out = out[:B * K * ld].reshape(B, K, ld)
    assert (out[:, :, ncols:] == SENTINEL).all(), 'padding overwritten'
    for before, after in zip(host, t):
        assert np.array_equal(before, after.cpu().numpy(), equal_nan=True)      # the inputs are read only
    return out[:, :, :ncols].copy()


def run(cfg, mixed, columns=None):
    """out of cp_taylor_jvp2 along (tan, tan2) (``mixed``) or (tan, tan), with everything the module docstring says asserted."""
    u, v = cfg['tan'], cfg['tan2'] if mixed else None
    out = call(cfg, columns, u, v)
    assert same_bits(call(cfg, columns, u, v), out), 'two calls differ'
    assert same_bits(call(cfg, columns, v, u) if mixed else call(cfg, columns, u, u), out), 'exchanging u and v (or giving v = u) changes bits'
    return out


@pytest.mark.parametrize('mixed', [False, True], ids=['v=u', 'mixed'])
@pytest.mark.parametrize('options', sr.TAYLOR_CASES, ids=[sr.case_id(case) for case in sr.TAYLOR_CASES])
def test_against_truth(options, mixed):
    cfg = sr.taylor_config(**options)
    out_ld, out_64 = sr.taylor_truth(cfg, mixed)
    out = run(cfg, mixed)
    if cfg['powers'].shape[0] == 1:      # the constant alone: exactly 0
        assert not out.any() and not out_ld.any()
    jr.assert_within(out, out_ld, out_64, '%s, %s' % (options, 'mixed' if mixed else 'v = u'))


def test_column_ranges():
    cfg = sr.taylor_config()
    for mixed in (False, True):
        out_ld, out_64 = sr.taylor_truth(cfg, mixed)
        out = run(cfg, mixed)
        for a, b in sr.MLP_RANGES:
            o = run(cfg, mixed, columns=(a, b))
            assert same_bits(o, out[:, :, a:b]), (a, b)
            jr.assert_within(o, out_ld[:, :, a:b], out_64[:, :, a:b], 'columns [%d, %d)' % (a, b))


def test_unit_pairs_of_single_monomials():
    """One term per column (derivatives the identity), x - center small integers, unit pairs (e_i, e_j): every entry is a product of small integers, exact in
    float64 -- p (p - 1) d^(p - 2) on the diagonal, p_i d_i^(p_i - 1) p_j d_j^(p_j - 1) off it, times the other factors; 0 for a term that does not hold
    i or j, or holds i to the first power on the diagonal."""
    powers = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0], [1, 1, 1], [3, 2, 0], [0, 2, 4], [2, 1, 3]], dtype='i4')
    T, ndim = powers.shape
    d = np.array([[2., -3., 1.], [-1., 2., 3.]])
    pairs = [(i, j) for i in range(ndim) for j in range(ndim)]
    u, v = (np.broadcast_to(np.eye(ndim)[[pair[side] for pair in pairs]], (len(d), len(pairs), ndim)).copy() for side in range(2))
    cfg = dict(center=np.array([0.5, -1., 2.]), powers=powers, derivatives=np.eye(T))
    cfg['X'] = cfg['center'] + d
    out = call(cfg, None, u, v)
    want = np.zeros((len(d), len(pairs), T))
    for k, (i, j) in enumerate(pairs):
        for t, power in enumerate(powers):
            reduced, coefficient = power.copy(), 1.
            for q in (i, j):
                coefficient *= reduced[q]
                reduced[q] = max(reduced[q] - 1, 0)
            want[:, k, t] = coefficient * np.prod(d**reduced, axis=1)
    assert np.array_equal(out, want)
    assert not out[:, :, :3].any()      # total order < 2


def test_total_order_below_two_contributes_exactly_zero():
    """Constant and linear terms with coefficients of 1e300 leave the bits of the result as they are with coefficients 0; a polynomial of such terms alone
    has the second derivative exactly 0."""
    cfg = sr.taylor_config(B=22, K=3, T=33)
    low = [0, 7, 32]
    cfg['powers'][low] = 0
    cfg['powers'][7, 1] = cfg['powers'][32, 2] = 1
    zero, huge = cfg['derivatives'].copy(), cfg['derivatives'].copy()
    zero[low], huge[low] = 0., 1e300
    assert same_bits(run(dict(cfg, derivatives=zero), True), run(dict(cfg, derivatives=huge), True))
    cfg['powers'][:] = 0
    cfg['powers'][::2, 0] = 1
    assert not run(cfg, True).any() and not run(cfg, False).any()


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_nan_and_inf_under_power_0_and_above(bad):
    """Parameter 1 only ever has power 0: NaN / Inf in it, or in its tangent components of either set, change no bit and the result stays finite.  A bad value
    in parameter 2 at point 7 reaches the rows of point 7 and no other point; a bad tangent component (21, 1, 2) of the second set -- row 64, the first of the
    second tile -- reaches exactly that row."""
    cfg = sr.taylor_config(B=22, K=3)
    cfg['powers'][:, 1] = 0
    assert (cfg['powers'][:, 2] >= 2).any() and ((cfg['powers'][:, 2] >= 1) & (cfg['powers'][:, 0] >= 2)).any()
    clean = run(cfg, True)
    assert np.isfinite(clean).all()
    X, tan, tan2 = cfg['X'].copy(), cfg['tan'].copy(), cfg['tan2'].copy()
    X[7, 1] = X[21, 1] = bad
    tan[3, :, 1] = tan2[21, 1, 1] = tan2[4, 0, 1] = bad
    out = run(dict(cfg, X=X, tan=tan, tan2=tan2), True)
    assert same_bits(out, clean) and np.isfinite(out).all()
    X = cfg['X'].copy()
    X[7, 2] = bad
    out = run(dict(cfg, X=X), True)
    hit = np.arange(22) == 7
    assert not np.isfinite(out[hit]).any() and same_bits(out[~hit], clean[~hit])
    tan2 = cfg['tan2'].copy()
    tan2[21, 1, 2] = bad
    out = run(dict(cfg, tan2=tan2), True)
    hit = np.zeros((22, 3), dtype=bool)
    hit[21, 1] = True
    assert not np.isfinite(out[hit]).any() and same_bits(out[~hit], clean[~hit])


def test_engine(golden):
    """TaylorEmulatorEngine.jvp2: shapes, ``columns``, ``return_value``, ``return_first``, host and device tangents, and the truth on a golden (fitted)
    configuration."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    g = golden('taylor')
    engine = TaylorEmulatorEngine.from_state({'center': g['c0_center'], 'powers': g['c0_powers'], 'derivatives': g['c0_derivatives']}, device='cuda:0')
    X = g['c0_Xq']
    M = g['c0_derivatives'].shape[1]
    rng = np.random.default_rng(0)
    tan, tan2 = (rng.normal(0., 1., (len(X), 4, 3)) for _ in range(2))
    out = engine.jvp2(X, tan, tan2)
    assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (len(X), 4, M) and out.is_contiguous()
    assert torch.equal(engine.jvp2(X, tan2, tan), out)
    value, fu, fv, out2 = engine.jvp2(X, torch.as_tensor(tan, device='cuda:0'), tan2, return_value=True, return_first=True)
    assert torch.equal(out2, out) and torch.equal(value, engine.predict(X)) and torch.equal(fu, engine.jvp(X, tan)) and torch.equal(fv, engine.jvp(X, tan2))
    same = engine.jvp2(X, tan)
    fu, same2 = engine.jvp2(X, tan, return_first=True)
    assert torch.equal(same, same2) and torch.equal(fu, engine.jvp(X, tan)) and torch.equal(engine.jvp2(X, tan, tan), same)
    single = engine.jvp2(X, tan[:, 2], tan2[:, 2])
    assert tuple(single.shape) == (len(X), M) and torch.equal(single, out[:, 2])
    value, outc = engine.jvp2(torch.as_tensor(X, device='cuda:0'), tan, tan2, columns=(2, M - 1), return_value=True)
    assert torch.equal(outc, out[:, :, 2:M - 1]) and torch.equal(value, engine.predict(X, columns=(2, M - 1)))
    c = dict(center=g['c0_center'], powers=g['c0_powers'], derivatives=g['c0_derivatives'], X=X, tan=tan, tan2=tan2)
    for mixed, got in ((True, out), (False, same)):
        out_ld, out_64 = sr.taylor_truth(c, mixed)
        jr.assert_within(got.cpu().numpy(), out_ld, out_64, 'golden configuration 0, %s' % ('mixed' if mixed else 'v = u'))
    with pytest.raises(ValueError):
        engine.jvp2(X, tan, columns=(3, 3))
    with pytest.raises(ValueError):
        engine.jvp2(X, tan, tan2[:, :2])
