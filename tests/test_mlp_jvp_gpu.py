"""GPU: cp_mlp_jvp (csrc/cp_mlp.hip, mlp_jvp_kernel) against the longdouble tangents contracted with the longdouble forward-mode Jacobian
(tests/jvp_reference.py).

Tolerance (jacobian_reference.assert_within): per block -- one (direction k, output column) pair over the batch -- the rounding level
is the float64 restatement's largest distance from the truth relative to the block's largest entry, floored at 1.1e-16 (held to at most 32 x that floor for
every case here by tests/test_jvp_host.py); the device is allowed 16 x that level.  Tangents are xscale x N(0, 1).

Every call here (``run``) goes into buffers with row strides ldv, ldo = ncols + 3 followed by 64 doubles, all holding a sentinel that must survive;
d_value must equal cp_mlp_predict_columns bit for bit, a second call must give the same bits, and the inputs must be unchanged afterwards.

Cases (jvp_reference.MLP_CASES), one dimension at a time from B = 65, ndim = 3, K = 2, widths (5, 17), M = 257, silu, no y function: (B, K) in (63, 1),
(64, 1), (22, 3), (43, 3) (63, 64, 66 and 129 rows: the last row of a tile, a point split across two tiles), K in {1, 5, 7, 64, 65}, ndim in {1, 2, 5, 32}, last
width in {3, 8, 9, 33, 64}, first width in {1, 64}, M in {1, 16, 255, 256}, depth in {1, 8}, every activation, every y function, and the column ranges (0, 1),
(255, 257), (16, 17), which must give the bits of the same columns of the full call.  Then: identity tangents against cp_mlp_jacobian bit for bit, the
duality with cp_mlp_vjp, the zero tangent, NaN in a point and in a tangent, relu at a pre-activation of exactly 0."""
import ctypes

import numpy as np
import pytest

import jacobian_reference as jr
import jvp_reference as pr
import mlp_reference as mr
import vjp_reference as vr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def device_arguments(cfg, columns):
    """(tensors by name, host copies, the arguments of the C entry points between d_x and the outputs, ncols)"""
    import torch
    from cosmoprimo_amd import _lib
    device = torch.device('cuda', 0)
    dims, (B, ndim) = cfg['dims'], cfg['X'].shape
    L, M = len(dims) - 2, dims[-1]
    col0, stop = columns or (0, M)
    widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']])
    names = [name for name in ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale', 'tan', 'cot') if name in cfg]
    host = {name: np.ascontiguousarray(cfg[name], dtype='f8') for name in names}
    t = {name: torch.as_tensor(a, device=device) for name, a in host.items()}
    net = (B, ndim, L, widths, acts, M) + tuple(t[name].data_ptr() for name in ('packed', 'xoffset', 'xscale', 'yoffset', 'yscale')) \
        + (_lib.MLP_YFUNCTIONS[cfg['yfunction'] or None], col0, stop - col0)
    return t, host, net, stop - col0


def run(cfg, columns=None):
    """(value (B, ncols), out (B, K, ncols)) of one call of cp_mlp_jvp, with everything the module docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    t, host, net, ncols = device_arguments(cfg, columns)
    B, K = cfg['tan'].shape[:2]
    ld = ncols + PAD
    results = []
    for _ in range(2):
        value = torch.full((B * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        out = torch.full((B * K * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        _lib.check(lib.cp_mlp_jvp(t['X'].data_ptr(), *net, t['tan'].data_ptr(), K, value.data_ptr(), ld, out.data_ptr(), ld, 0, dv.stream_of(device)))
        torch.cuda.synchronize(device)
        value, out = value.cpu().numpy(), out.cpu().numpy()
        assert (value[B * ld:] == SENTINEL).all() and (out[B * K * ld:] == SENTINEL).all(), 'written past the end'
        value, out = value[:B * ld].reshape(B, ld), out[:B * K * ld].reshape(B, K, ld)
        assert (value[:, ncols:] == SENTINEL).all() and (out[:, :, ncols:] == SENTINEL).all(), 'padding overwritten'
        results.append((value[:, :ncols].copy(), out[:, :, :ncols].copy()))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1]), 'two calls differ'
    for name, before in host.items():
        assert same_bits(before, t[name].cpu().numpy()), name      # the inputs are read only
    want = torch.empty((B, ncols), dtype=torch.float64, device=device)
    _lib.check(lib.cp_mlp_predict_columns(t['X'].data_ptr(), *net, want.data_ptr(), ncols, 0, dv.stream_of(device)))
    assert same_bits(results[0][0], want.cpu().numpy()), 'value is not cp_mlp_predict_columns'
    return results[0]


def jacobian(cfg):
    """J (B, ndim, M) of cp_mlp_jacobian"""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    device = torch.device('cuda', 0)
    t, host, net, ncols = device_arguments(cfg, None)
    B, ndim = cfg['X'].shape
    value, jac = torch.empty((B, ncols), dtype=torch.float64, device=device), torch.empty((B, ndim, ncols), dtype=torch.float64, device=device)
    _lib.check(_lib.load().cp_mlp_jacobian(t['X'].data_ptr(), *net, value.data_ptr(), ncols, jac.data_ptr(), ncols, 0, dv.stream_of(device)))
    return jac.cpu().numpy()


def vjp(cfg):
    """G (B, ndim) of cp_mlp_vjp with the cotangent cfg['cot'] (B, M)"""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    t, host, net, ncols = device_arguments(cfg, None)
    B, ndim = cfg['X'].shape
    need = int(lib.cp_mlp_vjp_workspace_doubles(B, ndim, net[2], net[3], net[5], ncols))
    work, grad = torch.empty(need, dtype=torch.float64, device=device), torch.empty((B, ndim), dtype=torch.float64, device=device)
    _lib.check(lib.cp_mlp_vjp(t['X'].data_ptr(), *net, t['cot'].data_ptr(), ncols, None, ncols, grad.data_ptr(), work.data_ptr(), need, 0, dv.stream_of(device)))
    return grad.cpu().numpy()


@pytest.mark.parametrize('options', pr.MLP_CASES, ids=[pr.case_id(case) for case in pr.MLP_CASES])
def test_against_truth(options):
    cfg = pr.mlp_config(**options)
    out_ld, out_64 = pr.mlp_truth(cfg)
    value, out = run(cfg)
    jr.assert_within(out, out_ld, out_64, str(options))


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_column_ranges(yfunction):
    cfg = pr.mlp_config(yfunction=yfunction, activations='tanh')
    out_ld, out_64 = pr.mlp_truth(cfg)
    value, out = run(cfg)
    for a, b in pr.MLP_RANGES:
        v, o = run(cfg, columns=(a, b))
        assert same_bits(v, value[:, a:b]) and same_bits(o, out[:, :, a:b]), (a, b)
        jr.assert_within(o, out_ld[:, :, a:b], out_64[:, :, a:b], 'columns [%d, %d)' % (a, b))


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_identity_tangents_are_the_jacobian(yfunction):
    """K = ndim identity tangents: the bits of cp_mlp_jacobian (the rows are wired to the right points and directions)."""
    for options in (dict(K=3), dict(B=22, K=3), dict(ndim=5, K=5, widths=(33, 64), activations='identity-silu')):
        cfg = pr.mlp_config(yfunction=yfunction, **options)
        B, ndim = cfg['X'].shape
        cfg['tan'] = np.broadcast_to(np.eye(ndim), (B, ndim, ndim)).copy()
        value, out = run(cfg)
        assert same_bits(out, jacobian(cfg)), options


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_duality_with_vjp(yfunction):
    """sum_c cot jvp(t) = sum_i vjp(cot) t per point and direction.  Either side is a float64 sum of products of quantities that each lie within their own
    allowance: jvp within 16 level_c top_c per column (the rule above), vjp within 16 level 2^-53 A_i (the rule of tests/vjp_reference.py, A its magnitude
    pass).  The difference is allowed the sum of both, sum_c |cot_c| 16 level_c top_c + sum_i 16 level 2^-53 A_i |t_i|, plus the rounding of the two float64
    sums themselves, (M + ndim) 2^-53 times their magnitude sum |terms|."""
    cfg = pr.mlp_config(yfunction=yfunction, K=3)
    B, K, ndim = cfg['tan'].shape
    M = cfg['dims'][-1]
    cfg['cot'] = np.random.default_rng(7).normal(0., 1., (B, M))
    value, out = run(cfg)
    G = vjp(cfg)
    G_ld, A, vjp_level = vr.mlp_case(cfg, cfg['cot'])
    top, level = jr.levels(*pr.mlp_truth(cfg))      # (K, M)
    cot, tan = np.abs(cfg['cot']).astype(jr.LD), np.abs(cfg['tan']).astype(jr.LD)
    left, right = np.einsum('bc,bkc->bk', cfg['cot'], out), np.einsum('bi,bki->bk', G, cfg['tan'])
    allowed = np.einsum('bc,kc->bk', cot, jr.ALLOW * level * top) + jr.ALLOW * vjp_level * 2.**-53 * np.einsum('bi,bki->bk', A, tan)
    allowed = allowed + (M + ndim) * 2.**-53 * (np.einsum('bc,bkc->bk', cot, np.abs(out)) + np.einsum('bi,bki->bk', np.abs(G), tan))
    fraction = np.abs(left.astype(jr.LD) - right) / allowed
    print('duality, %s: largest fraction of the allowance %.3g' % (yfunction or 'no y function', float(fraction.max())))
    assert float(fraction.max()) <= 1.


def test_zero_tangent_and_nan_contract():
    """A zero tangent gives zeros where the point is finite.  A NaN in row b of X makes the K rows of point b NaN (for every activation, relu with its comparison
    included) and no other; a NaN in tangent (b, k) makes exactly row (b, k) NaN, and the others keep their bits."""
    for activation in mr.ACTIVATIONS:
        cfg = pr.mlp_config(B=22, K=3, activations=activation, yfunction='arcsinh')
        cfg['tan'][5] = 0.
        cfg['tan'][9, 1] = 0.
        value, out = run(cfg)
        assert np.isfinite(out).all() and not out[5].any() and not out[9, 1].any() and out[9, 0].any()
        X = cfg['X'].copy()
        X[7, 1] = X[21, 2] = np.nan      # (point 21: rows 63 .. 65, in two tiles)
        v, o = run(dict(cfg, X=X))
        hit = np.zeros(22, dtype=bool)
        hit[[7, 21]] = True
        assert np.isnan(o[hit]).all() and np.isnan(v[hit]).all(), activation
        assert same_bits(o[~hit], out[~hit]) and same_bits(v[~hit], value[~hit]), activation
        tan = cfg['tan'].copy()
        tan[7, 1, 0] = tan[21, 0, 2] = tan[21, 1, 1] = np.nan      # (rows 22, 63 and 64: the last row of a tile and the first of the next)
        v, o = run(dict(cfg, tan=tan))
        hit = np.zeros((22, 3), dtype=bool)
        hit[7, 1] = hit[21, 0] = hit[21, 1] = True
        assert np.isnan(o[hit]).all() and same_bits(o[~hit], out[~hit]) and same_bits(v, value), activation


def test_relu_at_zero():
    """A pre-activation exactly 0 gives the tangent 0: one input x = 1 (offset 0, scale 1), neuron 0 with z = 0.5 x - 0.5 = 0, neuron 1 with
    z = 0.25 x + 0.125 > 0; the derivative of output c along t is t 0.25 W_out[1, c], exactly (t a power of two), with nothing of 0.5 W_out[0, c]."""
    dims = (1, 2, 5)
    packed = np.zeros(mr.nparams(dims))
    sl = mr.blocks(dims)
    packed[sl['kernel0']], packed[sl['bias0']] = [0.5, 0.25], [-0.5, 0.125]
    wout = np.random.default_rng(5).normal(0., 1., (2, 5))
    packed[sl['kernel1']], packed[sl['bias1']] = wout.ravel(), np.arange(5.)
    cfg = dict(dims=dims, activations=['relu'], packed=packed, yfunction='', xoffset=np.zeros(1), xscale=np.ones(1), yoffset=np.zeros(5), yscale=np.ones(5), X=np.ones((1, 1)),
               tan=np.array([[[1.], [-4.]]]))
    value, out = run(cfg)
    assert np.array_equal(out[0, 0], 0.25 * wout[1]) and np.array_equal(out[0, 1], -wout[1]) and np.array_equal(value[0], 0.375 * wout[1] + np.arange(5.))


def test_engine(golden):
    """MLPEmulatorEngine.jvp: shapes, ``columns``, ``return_value`` equal to ``predict`` bit for bit, host and device tangents, the truth of a golden
    (trained) configuration."""
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    for i in range(2):
        cfg = mr.golden_config(golden('mlp'), i)
        engine = MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')
        X, (ndim, M) = cfg['Xq'], (cfg['dims'][0], cfg['dims'][-1])
        tan = np.asarray(cfg['xscale']) * np.random.default_rng(i).normal(0., 1., (len(X), 4, ndim))
        out = engine.jvp(X, tan)
        assert isinstance(out, torch.Tensor) and out.is_cuda and tuple(out.shape) == (len(X), 4, M) and out.is_contiguous()
        value, out2 = engine.jvp(X, torch.as_tensor(tan, device='cuda:0'), return_value=True)
        assert torch.equal(out2, out) and torch.equal(value, engine.predict(X))
        single = engine.jvp(X, tan[:, 2])
        assert tuple(single.shape) == (len(X), M) and torch.equal(single, out[:, 2])
        a, b = M // 3, M - 1
        value, outc = engine.jvp(torch.as_tensor(X, device='cuda:0'), tan, columns=(a, b), return_value=True)
        assert torch.equal(outc, out[:, :, a:b]) and torch.equal(value, engine.predict(X, columns=(a, b)))
        assert torch.equal(engine.jvp(X, np.broadcast_to(np.eye(ndim), (len(X), ndim, ndim))), engine.jacobian(X))
        c = dict(cfg, X=X, tan=tan)
        out_ld, out_64 = pr.mlp_truth(c)
        jr.assert_within(out.cpu().numpy(), out_ld, out_64, 'golden configuration %d' % i)
        with pytest.raises(ValueError):
            engine.jvp(X, tan, columns=(3, 3))
        with pytest.raises(ValueError):
            engine.jvp(X, tan[:, :, :-1])
        with pytest.raises(ValueError):
            engine.jvp(X, tan[:-1])
