"""GPU: cp_mlp_jacobian (csrc/cp_mlp.hip, mlp_tangent_kernel) against the longdouble forward-mode pass of tests/jacobian_reference.py.

Tolerance (the rule of the gradient of cp_mlp_loss_grad; jacobian_reference.assert_within): per block -- one (parameter, output
column) pair over the batch; columns behind 10^v differ by orders of magnitude, a coarser block would hide the small ones -- the rounding level is the
float64 restatement's largest distance from the truth relative to the block's largest entry, floored at 1.1e-16; the device is allowed 16 x that level.

Every call here (``run``) goes into buffers with row strides ldv, ldj = ncols + 3 followed by 64 doubles, all holding a sentinel that must survive;
d_value must equal cp_mlp_predict_columns bit for bit, a second call must give the same bits, and the inputs must be unchanged afterwards.

Cases, one dimension at a time from B = 65, ndim = 3, widths (5, 17), M = 257, silu, no y function: B in {1, 21, 22, 64} (21 x 3 = 63 and 22 x 3 = 66 rows:
the last row of a tile, a point split across two tiles), ndim in {1, 2, 5, 32}, last width in {3, 8, 9, 33, 64} (masked inner indices of an MFMA pair, more
than 64 KB of LDS), first width in {1, 64}, M in {1, 16, 255, 256}, depth in {1, 8}, every activation, every y function, and the column ranges (0, 1),
(255, 257), (16, 17), which must give the bits of the same columns of the full call."""
import ctypes

import numpy as np
import pytest

import jacobian_reference as jr
import mlp_reference as mr
from mlp_device import draw_network, same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def config(B=65, ndim=3, widths=(5, 17), M=257, activations='silu', yfunction='', seed=0):
    rng = np.random.default_rng(1000 * B + 100 * ndim + 10 * sum(widths) + M + seed)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = [activations] * len(widths) if isinstance(activations, str) else list(activations)
    lo, xscale = rng.uniform(-1., 1., ndim), rng.uniform(0.5, 2., ndim)
    cfg = dict(dims=dims, activations=activations, packed=draw_network(rng, dims), yfunction=yfunction, xoffset=lo, xscale=xscale,
               yoffset=rng.normal(0., 1., M), yscale=rng.uniform(0.5, 2., M))
    cfg['X'] = lo + xscale * rng.uniform(0., 1., (B, ndim))
    return cfg


def run(cfg, columns=None, check_value=True):
    """(value (B, ncols), J (B, ndim, ncols)) of one call of cp_mlp_jacobian, with everything the module docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    dims, (B, ndim) = cfg['dims'], cfg['X'].shape
    L, M = len(dims) - 2, dims[-1]
    col0, stop = columns or (0, M)
    ncols = stop - col0
    widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']])
    yfunction = _lib.MLP_YFUNCTIONS[cfg['yfunction'] or None]
    names = ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale')
    host = [np.ascontiguousarray(cfg[name], dtype='f8') for name in names]
    X, packed, xoffset, xscale, yoffset, yscale = t = [torch.as_tensor(a, device=device) for a in host]
    ld = ncols + PAD
    net = (B, ndim, L, widths, acts, M, packed.data_ptr(), xoffset.data_ptr(), xscale.data_ptr(), yoffset.data_ptr(), yscale.data_ptr(), yfunction, col0, ncols)
    results = []
    for _ in range(2):
        value = torch.full((B * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        jac = torch.full((B * ndim * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        _lib.check(lib.cp_mlp_jacobian(X.data_ptr(), *net, value.data_ptr(), ld, jac.data_ptr(), ld, 0, dv.stream_of(device)))
        torch.cuda.synchronize(device)
        value, jac = value.cpu().numpy(), jac.cpu().numpy()
        assert (value[B * ld:] == SENTINEL).all() and (jac[B * ndim * ld:] == SENTINEL).all(), 'written past the end'
        value, jac = value[:B * ld].reshape(B, ld), jac[:B * ndim * ld].reshape(B, ndim, ld)
        assert (value[:, ncols:] == SENTINEL).all() and (jac[:, :, ncols:] == SENTINEL).all(), 'padding overwritten'
        results.append((value[:, :ncols].copy(), jac[:, :, :ncols].copy()))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1]), 'two calls differ'
    for name, before, after in zip(names, host, t):
        assert same_bits(before, after.cpu().numpy()), name      # the inputs are read only
    if check_value:
        want = torch.empty((B, ncols), dtype=torch.float64, device=device)
        _lib.check(lib.cp_mlp_predict_columns(X.data_ptr(), *net, want.data_ptr(), ncols, 0, dv.stream_of(device)))
        assert same_bits(results[0][0], want.cpu().numpy()), 'value is not cp_mlp_predict_columns'
    return results[0]


def truth(cfg):
    args = (cfg['packed'], cfg['dims'], cfg['activations'], cfg['X'], cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])
    return jr.mlp_jacobian(*args, dtype=jr.LD)[1], jr.mlp_jacobian(*args, dtype='f8')[1]


CASES = ([dict()] + [dict(B=B) for B in (1, 21, 22, 64)] + [dict(ndim=n) for n in (1, 2, 5, 32)] + [dict(widths=(5, w)) for w in (3, 8, 9, 33, 64)]
         + [dict(widths=(w, 17)) for w in (1, 64)] + [dict(M=M) for M in (1, 16, 255, 256)] + [dict(widths=(17,)), dict(widths=(5, 9, 17, 6, 33, 12, 7, 17))]
         + [dict(activations=a) for a in ('relu', 'tanh', 'identity-silu')] + [dict(activations=['identity-silu', 'relu', 'tanh', 'silu'], widths=(9, 12, 7, 17))]
         + [dict(yfunction=y) for y in ('log10', 'arcsinh')] + [dict(yfunction='log10', activations='identity-silu', widths=(33, 64))])


@pytest.mark.parametrize('options', CASES, ids=['-'.join('%s=%s' % item for item in case.items()).replace(' ', '') or 'base' for case in CASES])
def test_against_truth(options):
    cfg = config(**options)
    J_ld, J_64 = truth(cfg)
    value, J = run(cfg)
    jr.assert_within(J, J_ld, J_64, str(options))


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_column_ranges(yfunction):
    cfg = config(yfunction=yfunction, activations='tanh')
    J_ld, J_64 = truth(cfg)
    value, J = run(cfg)
    for a, b in ((0, 1), (255, 257), (16, 17)):
        v, j = run(cfg, columns=(a, b))
        assert same_bits(v, value[:, a:b]) and same_bits(j, J[:, :, a:b]), (a, b)
        jr.assert_within(j, J_ld[:, :, a:b], J_64[:, :, a:b], 'columns [%d, %d)' % (a, b))


def test_nan_contract():
    """A NaN in row b of X makes the ndim rows of point b NaN (for every activation, relu with its comparison included) and touches no other point; a NaN
    column of the output kernel stays in its column."""
    for activation in mr.ACTIVATIONS:
        cfg = config(B=22, activations=activation, yfunction='arcsinh')
        value, J = run(cfg)
        assert np.isfinite(J).all()
        X = cfg['X'].copy()
        X[7, 1] = X[21, 2] = np.nan      # (point 21: rows 63 .. 65, in two tiles)
        v, j = run(dict(cfg, X=X))
        hit = np.zeros(22, dtype=bool)
        hit[[7, 21]] = True
        assert np.isnan(j[hit]).all() and np.isnan(v[hit]).all(), activation
        assert same_bits(j[~hit], J[~hit]) and same_bits(v[~hit], value[~hit]), activation
    cfg = config(B=22)
    value, J = run(cfg)
    packed = cfg['packed'].copy()
    packed[mr.blocks(cfg['dims'])['kernel2']].reshape(17, 257)[:, 100] = np.nan      # (a view into packed)
    v, j = run(dict(cfg, packed=packed))
    keep = np.arange(257) != 100
    assert np.isnan(j[:, :, 100]).all() and same_bits(j[:, :, keep], J[:, :, keep]) and same_bits(v[:, keep], value[:, keep])


def test_relu_at_zero():
    """A pre-activation exactly 0 gives the tangent 0: one input x = 1 (offset 0, scale 1), neuron 0 with z = 0.5 x - 0.5 = 0, neuron 1 with
    z = 0.25 x + 0.125 > 0; the derivative of output c is 0.25 W_out[1, c], exactly, with nothing of 0.5 W_out[0, c]."""
    dims = (1, 2, 5)
    packed = np.zeros(mr.nparams(dims))
    sl = mr.blocks(dims)
    packed[sl['kernel0']], packed[sl['bias0']] = [0.5, 0.25], [-0.5, 0.125]
    wout = np.random.default_rng(5).normal(0., 1., (2, 5))
    packed[sl['kernel1']], packed[sl['bias1']] = wout.ravel(), np.arange(5.)
    cfg = dict(dims=dims, activations=['relu'], packed=packed, yfunction='', xoffset=np.zeros(1), xscale=np.ones(1), yoffset=np.zeros(5), yscale=np.ones(5), X=np.ones((1, 1)))
    value, J = run(cfg)
    assert np.array_equal(J[0, 0], 0.25 * wout[1]) and np.array_equal(value[0], 0.375 * wout[1] + np.arange(5.))


def test_engine(golden):
    """MLPEmulatorEngine.jacobian: shapes, ``columns``, ``return_value`` equal to ``predict`` bit for bit, the truth of a golden (trained) configuration."""
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    for i in range(2):
        cfg = mr.golden_config(golden('mlp'), i)
        engine = MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')
        X, (ndim, M) = cfg['Xq'], (cfg['dims'][0], cfg['dims'][-1])
        J = engine.jacobian(X)
        assert isinstance(J, torch.Tensor) and J.is_cuda and tuple(J.shape) == (len(X), ndim, M) and J.is_contiguous()
        value, J2 = engine.jacobian(X, return_value=True)
        assert torch.equal(J2, J) and torch.equal(value, engine.predict(X))
        a, b = M // 3, M - 1
        value, Jc = engine.jacobian(torch.as_tensor(X, device='cuda:0'), columns=(a, b), return_value=True)
        assert torch.equal(Jc, J[:, :, a:b]) and torch.equal(value, engine.predict(X, columns=(a, b)))
        args = (cfg['packed'], cfg['dims'], cfg['activations'], X, cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])
        jr.assert_within(J.cpu().numpy(), jr.mlp_jacobian(*args, dtype=jr.LD)[1], jr.mlp_jacobian(*args, dtype='f8')[1], 'golden configuration %d' % i)
        with pytest.raises(ValueError):
            engine.jacobian(X, columns=(3, 3))
        with pytest.raises(ValueError):
            engine.jacobian(X[:, :-1])
