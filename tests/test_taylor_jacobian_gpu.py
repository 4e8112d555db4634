"""GPU: cp_taylor_jacobian (csrc/cp_taylor.hip, the derivative front end of taylor_gemm_kernel) against the longdouble derivative of the polynomial of
tests/jacobian_reference.py.

Tolerance: the rule of tests/test_mlp_jacobian_gpu.py (jacobian_reference.assert_within): per (parameter, output column) block the
device is allowed 16 x the rounding level of the float64 restatement, floored at 1.1e-16.  Every call (``run``) goes into a buffer with the row stride
ldj = ncols + 3 followed by 64 doubles, all holding a sentinel that must survive; a second call must give the same bits; the inputs must be unchanged.

Cases, one dimension at a time from B = 65, ndim = 3, T = 65, M = 257, powers drawn from {0, 1, 2, 3} with one term at power 15 and term 0 the constant
(every power 0: a zero column of the left operand): B in {1, 21, 22, 64}, ndim in {1, 2, 32}, T in {1, 31, 32, 33} (the LDS chunk of 32 terms),
M in {1, 255, 256}, and the column ranges (0, 1), (255, 257), (16, 17), which must give the bits of the same columns of the full call."""
import numpy as np
import pytest

import jacobian_reference as jr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def config(B=65, ndim=3, T=65, M=257):
    rng = np.random.default_rng(1000 * B + 100 * ndim + 10 * T + M)
    powers = rng.integers(0, 4, (T, ndim)).astype('i4')
    powers[0] = 0
    if T > 1:
        powers[T // 2, rng.integers(ndim)] = 15
    return dict(center=rng.uniform(-0.5, 0.5, ndim), powers=powers, derivatives=rng.normal(0., 1., (T, M)), X=rng.uniform(-1., 1., (B, ndim)))


def run(cfg, columns=None):
    """J (B, ndim, ncols) of one call of cp_taylor_jacobian, with everything the module docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    (B, ndim), (T, M) = cfg['X'].shape, cfg['derivatives'].shape
    col0, stop = columns or (0, M)
    ncols = stop - col0
    names = ('X', 'center', 'powers', 'derivatives')
    host = [np.ascontiguousarray(cfg[name]) for name in names]
    X, center, powers, derivatives = t = [torch.as_tensor(a, device=device) for a in host]
    assert powers.dtype == torch.int32 and X.dtype == torch.float64
    ld = ncols + PAD
    results = []
    for _ in range(2):
        jac = torch.full((B * ndim * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        _lib.check(lib.cp_taylor_jacobian(X.data_ptr(), B, center.data_ptr(), powers.data_ptr(), ndim, T, int(cfg['powers'].max()), derivatives.data_ptr(), M, col0, ncols,
                                          jac.data_ptr(), ld, 0, dv.stream_of(device)))
        torch.cuda.synchronize(device)
        jac = jac.cpu().numpy()
        assert (jac[B * ndim * ld:] == SENTINEL).all(), 'written past the end'
        jac = jac[:B * ndim * ld].reshape(B, ndim, ld)
        assert (jac[:, :, ncols:] == SENTINEL).all(), 'padding overwritten'
        results.append(jac[:, :, :ncols].copy())
    assert same_bits(results[0], results[1]), 'two calls differ'
    for name, before, after in zip(names, host, t):
        assert np.array_equal(before, after.cpu().numpy(), equal_nan=True), name      # the inputs are read only
    return results[0]


def truth(cfg):
    args = (cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'])
    with np.errstate(invalid='ignore'):      # (Inf - Inf where a test puts Inf into X)
        return jr.taylor_jacobian(*args, dtype=jr.LD), jr.taylor_jacobian(*args, dtype='f8')


CASES = ([dict()] + [dict(B=B) for B in (1, 21, 22, 64)] + [dict(ndim=n) for n in (1, 2, 32)] + [dict(T=T) for T in (1, 31, 32, 33)] + [dict(M=M) for M in (1, 255, 256)])


@pytest.mark.parametrize('options', CASES, ids=['-'.join('%s=%s' % item for item in case.items()) or 'base' for case in CASES])
def test_against_truth(options):
    cfg = config(**options)
    J_ld, J_64 = truth(cfg)
    J = run(cfg)
    if cfg['powers'].shape[0] == 1:      # the constant alone: its derivative is exactly 0
        assert not J.any() and not J_ld.any()
    jr.assert_within(J, J_ld, J_64, str(options))


def test_column_ranges():
    cfg = config()
    J_ld, J_64 = truth(cfg)
    J = run(cfg)
    for a, b in ((0, 1), (255, 257), (16, 17)):
        j = run(cfg, columns=(a, b))
        assert same_bits(j, J[:, :, a:b]), (a, b)
        jr.assert_within(j, J_ld[:, :, a:b], J_64[:, :, a:b], 'columns [%d, %d)' % (a, b))


def test_zero_rows_of_the_left_operand():
    """A term with every power 0 gives a zero row of the left operand: with NaN coefficients in such terms alone the product is NaN everywhere (0 x NaN), so
    instead they get coefficients of 1e300, which must leave the bits of the result as they are with coefficients 0."""
    cfg = config(B=22, T=33)
    cfg['powers'][[0, 7, 32]] = 0
    zero, huge = cfg['derivatives'].copy(), cfg['derivatives'].copy()
    zero[[0, 7, 32]], huge[[0, 7, 32]] = 0., 1e300
    assert same_bits(run(dict(cfg, derivatives=zero)), run(dict(cfg, derivatives=huge)))


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_nan_and_inf_in_a_parameter(bad):
    """Parameter 1 of point 7 and parameter 2 of point 21 (rows 63 .. 65: two tiles) are NaN / Inf.  Terms are restricted to powers <= 1 in those two
    parameters, so that both rules show: under power 0 the factor is skipped, under power 1 the row of that parameter itself drops the factor -- its row
    stays finite and equals the truth -- while the other rows of the point take it.  No other point is touched, and a NaN column of the derivatives stays
    in its column."""
    cfg = config(B=22)
    cfg['powers'][:, 1:] = np.minimum(cfg['powers'][:, 1:], 1)
    clean = run(cfg)
    X = cfg['X'].copy()
    X[7, 1] = X[21, 2] = bad
    cfg_bad = dict(cfg, X=X)
    J = run(cfg_bad)
    J_ld, J_64 = truth(cfg_bad)
    hit = np.zeros(22, dtype=bool)
    hit[[7, 21]] = True
    assert same_bits(J[~hit], clean[~hit])
    assert np.isfinite(J[7, 1]).all() and np.isfinite(J[21, 2]).all() and not np.isfinite(J[7, [0, 2]]).any() and not np.isfinite(J[21, [0, 1]]).any()
    finite = np.isfinite(np.asarray(J_ld, dtype='f8'))
    assert np.array_equal(np.isfinite(J), finite) and np.array_equal(np.isnan(J), np.isnan(np.asarray(J_ld, dtype='f8')))
    assert np.array_equal(J[np.isinf(J)], np.asarray(J_ld, dtype='f8')[np.isinf(J)])      # (the signs of the infinities)
    mask = lambda a: np.where(finite, a, 0)      # noqa: E731
    jr.assert_within(mask(J), mask(J_ld), mask(J_64), 'finite entries next to %s' % bad)
    derivatives = cfg['derivatives'].copy()
    derivatives[:, 100] = np.nan
    J = run(dict(cfg, derivatives=derivatives))
    keep = np.arange(257) != 100
    assert np.isnan(J[:, :, 100]).all() and same_bits(J[:, :, keep], clean[:, :, keep])


def test_engine(golden):
    """TaylorEmulatorEngine.jacobian: shapes, ``columns``, ``return_value``, and the truth on a golden (fitted) configuration."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    g = golden('taylor')
    engine = TaylorEmulatorEngine.from_state({'center': g['c0_center'], 'powers': g['c0_powers'], 'derivatives': g['c0_derivatives']}, device='cuda:0')
    X = g['c0_Xq']
    M = g['c0_derivatives'].shape[1]
    J = engine.jacobian(X)
    assert isinstance(J, torch.Tensor) and J.is_cuda and tuple(J.shape) == (len(X), 3, M) and J.is_contiguous()
    value, J2 = engine.jacobian(X, return_value=True)
    assert torch.equal(J2, J) and torch.equal(value, engine.predict(X))
    value, Jc = engine.jacobian(torch.as_tensor(X, device='cuda:0'), columns=(2, M - 1), return_value=True)
    assert torch.equal(Jc, J[:, :, 2:M - 1]) and torch.equal(value, engine.predict(X, columns=(2, M - 1)))
    args = (g['c0_center'], g['c0_powers'], g['c0_derivatives'], X)
    jr.assert_within(J.cpu().numpy(), jr.taylor_jacobian(*args, dtype=jr.LD), jr.taylor_jacobian(*args, dtype='f8'), 'golden configuration 0')
    with pytest.raises(ValueError):
        engine.jacobian(X, columns=(3, 3))
