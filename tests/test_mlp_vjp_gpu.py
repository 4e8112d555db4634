"""GPU: cp_mlp_vjp (csrc/cp_mlp.hip: mlp_forward_kernel in its vjp modes, mlp_dh_kernel, mlp_input_grad_kernel) against the longdouble reverse pass of
tests/vjp_reference.py.

Tolerance (vjp_reference.assert_within): per entry |G - G_ld| <= 16 level 2^-53 A[b, i], A the magnitude pass (the reverse pass with
every factor replaced by its absolute value) and level = max(1, the largest error of three float64 evaluation orders in units of 2^-53 A), measured
here for the very case.  Weights from N(0, 0.4), the output kernel x 0.1 under a y function, the cotangent from N(0, 1).

Every call (``run``) reads a cotangent with the row stride ncols + 3 (the padding NaN: it must not be read), writes G followed by 64 sentinels and the
value with the row stride ncols + 3 followed by 64 sentinels, and gets a workspace filled with NaN, announced with exactly cp_mlp_vjp_workspace_doubles
and followed by 64 sentinels; all sentinels must survive, the value must equal cp_mlp_predict_columns bit for bit, a second call (without the value)
must give the same bits, and the inputs must be unchanged afterwards.

Cases, one dimension at a time from B = 65, ndim = 3, widths (5, 17), M = 257, silu, no y function: B in {1, 63, 64, 129} (the ends of a row tile),
ndim in {1, 2, 8, 32}, last width in {1, 16, 33, 49, 64} (the four instantiations of mlp_dh_kernel), first width in {33, 64} (more than 64 KB of LDS in
the forward kernel), M in {1, 8, 9, 65, 1025} (with 257: slices of 8, 40, 56 and 64 columns, the last slice partial), depth 1 and 8, every
activation, every y function, and the column ranges (1, 2), (3, 200), (256, 257)."""
import ctypes

import numpy as np
import pytest

import mlp_reference as mr
import vjp_reference as vr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def run(cfg, cot=None, columns=None):
    """(value (B, ncols), G (B, ndim)) of cp_mlp_vjp for the cotangent ``cot`` (B, ncols; default: cfg['cot'] on the range), with everything the module
    docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    dims, (B, ndim) = cfg['dims'], cfg['X'].shape
    L, M = len(dims) - 2, dims[-1]
    col0, stop = columns or (0, M)
    ncols = stop - col0
    cot = cfg['cot'][:, col0:stop] if cot is None else cot
    widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']])
    yfunction = _lib.MLP_YFUNCTIONS[cfg['yfunction'] or None]
    ld = ncols + PAD
    padded = np.full((B, ld), np.nan)
    padded[:, :ncols] = cot
    names = ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale', 'cot')
    host = [np.ascontiguousarray(cfg[name], dtype='f8') for name in names[:-1]] + [padded]
    X, packed, xoffset, xscale, yoffset, yscale, cotd = t = [torch.as_tensor(a, device=device) for a in host]
    net = (B, ndim, L, widths, acts, M, packed.data_ptr(), xoffset.data_ptr(), xscale.data_ptr(), yoffset.data_ptr(), yscale.data_ptr(), yfunction, col0, ncols)
    need = int(lib.cp_mlp_vjp_workspace_doubles(B, ndim, L, widths, M, ncols))
    assert need > 0
    results = []
    for with_value in (True, False):
        value = torch.full((B * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        grad = torch.full((B * ndim + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        work = torch.full((need + TAIL,), np.nan, dtype=torch.float64, device=device)
        work[need:] = SENTINEL
        _lib.check(lib.cp_mlp_vjp(X.data_ptr(), *net, cotd.data_ptr(), ld, value.data_ptr() if with_value else None, ld, grad.data_ptr(), work.data_ptr(), need, 0,
                                  dv.stream_of(device)))
        torch.cuda.synchronize(device)
        value, grad, work = value.cpu().numpy(), grad.cpu().numpy(), work.cpu().numpy()
        assert (value[B * ld:] == SENTINEL).all() and (grad[B * ndim:] == SENTINEL).all() and (work[need:] == SENTINEL).all(), 'written past the end'
        value = value[:B * ld].reshape(B, ld)
        assert (value[:, ncols:] == SENTINEL).all(), 'padding overwritten'
        assert with_value or (value == SENTINEL).all(), 'value written though not asked for'
        results.append((value[:, :ncols].copy(), grad[:B * ndim].reshape(B, ndim).copy()))
    assert same_bits(results[0][1], results[1][1]), 'two calls differ'
    for name, before, after in zip(names, host, t):
        assert same_bits(before, after.cpu().numpy()), name      # the inputs are read only
    want = torch.empty((B, ncols), dtype=torch.float64, device=device)
    _lib.check(lib.cp_mlp_predict_columns(X.data_ptr(), *net, want.data_ptr(), ncols, 0, dv.stream_of(device)))
    assert same_bits(results[0][0], want.cpu().numpy()), 'value is not cp_mlp_predict_columns'
    return results[0]


@pytest.mark.parametrize('options', vr.MLP_CASES, ids=[vr.case_id(case) for case in vr.MLP_CASES])
def test_against_truth(options):
    cfg = vr.mlp_config(**options)
    G_ld, A, level = vr.mlp_case(cfg, cfg['cot'])
    value, G = run(cfg)
    vr.assert_within(G, G_ld, A, level, str(options))


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_column_ranges(yfunction):
    """A range is within the rule of the full call with zeros outside the range (whose truth it shares)."""
    cfg = vr.mlp_config(yfunction=yfunction, activations='tanh')
    for a, b in vr.MLP_RANGES:
        cot = cfg['cot'][:, a:b]
        G_ld, A, level = vr.mlp_case(cfg, cot, columns=(a, b))
        value, G = run(cfg, columns=(a, b))
        vr.assert_within(G, G_ld, A, level, 'columns [%d, %d)' % (a, b))
        full = np.zeros_like(cfg['cot'])
        full[:, a:b] = cot
        value, G_full = run(cfg, cot=full)
        vr.assert_within(G_full, G_ld, A, level, 'the full call, zero outside [%d, %d)' % (a, b))


@pytest.mark.parametrize('yfunction', ['', 'log10'])
def test_one_hot_cotangent_against_the_jacobian(yfunction):
    """cot = e_c gives column c of the device's own cp_mlp_jacobian, within the sum of both allowances."""
    import jacobian_reference as jr
    from test_mlp_jacobian_gpu import run as run_jacobian
    cfg = vr.mlp_config(yfunction=yfunction)
    args = (cfg['packed'], cfg['dims'], cfg['activations'], cfg['X'], cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])
    J_ld, J_64 = jr.mlp_jacobian(*args, dtype=jr.LD)[1], jr.mlp_jacobian(*args, dtype='f8')[1]
    top, block_level = jr.levels(J_ld, J_64)
    value, J = run_jacobian(cfg)
    for c in (0, 100, 256):
        cot = np.zeros_like(cfg['cot'])
        cot[:, c] = 1.
        G_ld, A, level = vr.mlp_case(cfg, cot)
        value, G = run(cfg, cot=cot)
        vr.assert_within(G, G_ld, A, level, 'one-hot %d' % c)
        allowed = vr.ALLOW * level * vr.EPS * A + jr.ALLOW * (block_level * top)[:, c]
        assert (np.abs(G - J[:, :, c]) <= allowed).all(), c


def test_nan_contract():
    """A NaN in row b of X makes exactly row b of G NaN (for every activation, relu with its comparison included, and without a y function, where the
    weighted cotangent of that row stays finite), and the other rows keep their bits; the same for a NaN in row b of the cotangent."""
    for activation in mr.ACTIVATIONS:
        for yfunction in ('', 'arcsinh'):
            cfg = vr.mlp_config(B=66, activations=activation, yfunction=yfunction)
            value, G = run(cfg)
            assert np.isfinite(G).all()
            hit = np.zeros(66, dtype=bool)
            hit[[7, 64]] = True
            X = cfg['X'].copy()
            X[7, 1] = X[64, 2] = np.nan
            v, g = run(dict(cfg, X=X))
            assert np.isnan(g[hit]).all() and np.isnan(v[hit]).all(), (activation, yfunction)
            assert same_bits(g[~hit], G[~hit]) and same_bits(v[~hit], value[~hit]), (activation, yfunction)
            cot = cfg['cot'].copy()
            cot[7, 100] = cot[64, 0] = np.nan
            v, g = run(cfg, cot=cot)
            assert np.isnan(g[hit]).all() and same_bits(g[~hit], G[~hit]) and same_bits(v, value), (activation, yfunction)


def test_relu_at_zero():
    """A pre-activation exactly 0 passes nothing back: one input x = 1 (offset 0, scale 1), neuron 0 with z = 0.5 x - 0.5 = 0, neuron 1 with
    z = 0.25 x + 0.125 > 0; G = 0.25 sum_c cot_c W_out[1, c] with nothing of neuron 0 (its output weights are 1e300: any share would show)."""
    dims = (1, 2, 5)
    packed = np.zeros(mr.nparams(dims))
    sl = mr.blocks(dims)
    packed[sl['kernel0']], packed[sl['bias0']] = [0.5, 0.25], [-0.5, 0.125]
    wout = np.random.default_rng(5).normal(0., 1., (2, 5))
    wout[0] = 1e300
    packed[sl['kernel1']], packed[sl['bias1']] = wout.ravel(), np.arange(5.)
    cot = np.array([[1., -2., 0.5, 4., 0.25]])
    cfg = dict(dims=dims, activations=['relu'], packed=packed, yfunction='', xoffset=np.zeros(1), xscale=np.ones(1), yoffset=np.zeros(5), yscale=np.ones(5), X=np.ones((1, 1)),
               cot=cot)
    value, G = run(cfg)
    want = 0.25 * np.sum(cot[0].astype(vr.LD) * wout[1].astype(vr.LD))
    assert abs(G[0, 0] - want) <= 16 * vr.EPS * 0.25 * np.sum(np.abs(cot[0] * wout[1]))


def test_engine(golden):
    """MLPEmulatorEngine.vjp: shapes, ``columns``, ``return_value`` equal to ``predict`` bit for bit, a strided cotangent, the truth of a golden (trained)
    configuration."""
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    for i in range(2):
        cfg = mr.golden_config(golden('mlp'), i)
        engine = MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')
        X, (ndim, M) = cfg['Xq'], (cfg['dims'][0], cfg['dims'][-1])
        cot = np.random.default_rng(i).normal(0., 1., (len(X), M))
        G = engine.vjp(X, cot)
        assert isinstance(G, torch.Tensor) and G.is_cuda and tuple(G.shape) == (len(X), ndim) and G.is_contiguous()
        value, G2 = engine.vjp(X, torch.as_tensor(cot, device='cuda:0'), return_value=True)
        assert torch.equal(G2, G) and torch.equal(value, engine.predict(X))
        a, b = M // 3, M - 1
        cotd = torch.as_tensor(cot, device='cuda:0')
        value, Gc = engine.vjp(torch.as_tensor(X, device='cuda:0'), cotd[:, a:b], columns=(a, b), return_value=True)      # (a view with the row stride M)
        assert torch.equal(value, engine.predict(X, columns=(a, b))) and torch.equal(Gc, engine.vjp(X, cot[:, a:b].copy(), columns=(a, b)))
        ref = dict(cfg, X=X)
        G_ld, A, level = vr.mlp_case(ref, cot)
        vr.assert_within(G.cpu().numpy(), G_ld, A, level, 'golden configuration %d' % i)
        G_ld, A, level = vr.mlp_case(ref, cot[:, a:b], columns=(a, b))
        vr.assert_within(Gc.cpu().numpy(), G_ld, A, level, 'golden configuration %d, columns' % i)
        with pytest.raises(ValueError):
            engine.vjp(X, cot[:, :0], columns=(3, 3))
        with pytest.raises(ValueError):
            engine.vjp(X, cot[:, :-1])
        with pytest.raises(ValueError):
            engine.vjp(X[:, :-1], cot)
