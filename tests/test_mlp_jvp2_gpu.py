"""GPU: cp_mlp_jvp2 (csrc/cp_mlp.hip, csrc/cp_mlp_tangent2.h: mlp_tangent2_kernel) against the longdouble second-order forward pass of tests/jvp2_reference.py.

Tolerance (jacobian_reference.assert_within, unchanged): per block -- one (pair of directions k, output column) over the batch -- the
rounding level is the float64 restatement's largest distance from the truth relative to the block's largest entry, floored at 1.1e-16 (held to at most
32 x that floor for every case here by tests/test_jvp2_host.py); the device is allowed 16 x that level.

Every call here (``run``) goes into buffers with row strides ldv, ldf, ldo = ncols + 3 followed by 64 doubles, all holding a sentinel that must survive;
d_value and d_first_u / d_first_v must equal what cp_mlp_jvp writes bit for bit, a second call must give the same bits, exchanging the two tangent sets
must give the same bits, and the inputs must be unchanged afterwards.

Cases (jvp2_reference.MLP_CASES: the shapes of jvp_reference.MLP_CASES, each with v = u and with a second tangent set), one dimension at a time from
B = 65, ndim = 3, K = 2, widths (5, 17), M = 257, silu, no y function; the widths (5, 64), (64, 17) and (33, 64) launch with 139 KB of LDS (104 KB with
v = u).  The column ranges (0, 1), (255, 257), (16, 17) must give the bits of the same columns of the full call.  Then: a relu network without y function
returns exactly 0, NaN in a point and in a tangent of either set stay in their rows, and the first-order products are optional without a y function."""
import numpy as np
import pytest

import jacobian_reference as jr
import jvp2_reference as sr
import mlp_reference as mr
from mlp_device import same_bits
from test_mlp_jvp_gpu import device_arguments

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64


def call(cfg, columns, tan_u, tan_v, first=True):
    """(value (B, ncols), first_u, first_v (B, K, ncols) or None, out (B, K, ncols)) of one call of cp_mlp_jvp2 with the sentinels checked."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    t, host, net, ncols = device_arguments(cfg, columns)
    B, K = tan_u.shape[:2]
    tans = [torch.as_tensor(np.ascontiguousarray(a), device=device) if a is not None else None for a in (tan_u, tan_v)]
    ld = ncols + PAD
    full = lambda rows: torch.full((rows * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)      # noqa: E731
    value, out = full(B), full(B * K)
    firsts = [full(B * K) if first and a is not None else None for a in tans]
    ptr = lambda a: a.data_ptr() if a is not None else None      # noqa: E731
    _lib.check(lib.cp_mlp_jvp2(t['X'].data_ptr(), *net, ptr(tans[0]), ptr(tans[1]), K, value.data_ptr(), ld, ptr(firsts[0]), ptr(firsts[1]), ld, out.data_ptr(), ld, 0,
                               dv.stream_of(device)))
    torch.cuda.synchronize(device)
    for name, before in host.items():
        assert same_bits(before, t[name].cpu().numpy()), name      # the inputs are read only
    for before, after in zip((tan_u, tan_v), tans):
        assert after is None or same_bits(np.ascontiguousarray(before), after.cpu().numpy())

    def unpad(a, shape):
        if a is None:
            return None
        a, rows = a.cpu().numpy(), int(np.prod(shape))
        assert (a[rows * ld:] == SENTINEL).all(), 'written past the end'
        a = a[:rows * ld].reshape(shape + (ld,))
        assert (a[..., ncols:] == SENTINEL).all(), 'padding overwritten'
        return a[..., :ncols].copy()

    return unpad(value, (B,)), unpad(firsts[0], (B, K)), unpad(firsts[1], (B, K)), unpad(out, (B, K))


def jvp(cfg, columns, tan):
    """(value, out) of cp_mlp_jvp along ``tan``"""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    device = torch.device('cuda', 0)
    t, host, net, ncols = device_arguments(cfg, columns)
    B, K = tan.shape[:2]
    tan = torch.as_tensor(np.ascontiguousarray(tan), device=device)
    value, out = torch.empty((B, ncols), dtype=torch.float64, device=device), torch.empty((B, K, ncols), dtype=torch.float64, device=device)
    _lib.check(_lib.load().cp_mlp_jvp(t['X'].data_ptr(), *net, tan.data_ptr(), K, value.data_ptr(), ncols, out.data_ptr(), ncols, 0, dv.stream_of(device)))
    return value.cpu().numpy(), out.cpu().numpy()


def run(cfg, mixed, columns=None):
    """(value, out) of cp_mlp_jvp2 along (tan, tan2) (``mixed``) or (tan, tan), with everything the module docstring says asserted."""
    u, v = cfg['tan'], cfg['tan2'] if mixed else None
    results = [call(cfg, columns, u, v) for _ in range(2)]
    for a, b in zip(*results):
        assert (a is None and b is None) or same_bits(a, b), 'two calls differ'
    value, first_u, first_v, out = results[0]
    want_value, want_u = jvp(cfg, columns, u)
    assert same_bits(value, want_value) and same_bits(first_u, want_u), 'value or first_u is not what cp_mlp_jvp writes'
    if mixed:
        assert same_bits(first_v, jvp(cfg, columns, v)[1]), 'first_v is not what cp_mlp_jvp writes'
        swapped = call(cfg, columns, v, u)
        assert same_bits(swapped[3], out) and same_bits(swapped[1], first_v) and same_bits(swapped[2], first_u), 'exchanging u and v changes bits'
    else:
        assert first_v is None
        assert same_bits(call(cfg, columns, u, u)[3], out), 'v = u given twice differs from v absent'
    if not cfg['yfunction']:      # the first-order products are optional
        assert same_bits(call(cfg, columns, u, v, first=False)[3], out), 'the result depends on d_first being given'
    return value, out


@pytest.mark.parametrize('mixed', [False, True], ids=['v=u', 'mixed'])
@pytest.mark.parametrize('options', sr.MLP_CASES, ids=[sr.case_id(case) for case in sr.MLP_CASES])
def test_against_truth(options, mixed):
    cfg = sr.mlp_config(**options)
    out_ld, out_64 = sr.mlp_truth(cfg, mixed)
    value, out = run(cfg, mixed)
    jr.assert_within(out, out_ld, out_64, '%s, %s' % (options, 'mixed' if mixed else 'v = u'))


@pytest.mark.parametrize('options', sr.MLP_RANGE_CASES, ids=[sr.case_id(case) for case in sr.MLP_RANGE_CASES])
def test_column_ranges(options):
    cfg = sr.mlp_config(**options)
    for mixed in (False, True):
        out_ld, out_64 = sr.mlp_truth(cfg, mixed)
        value, out = run(cfg, mixed)
        jr.assert_within(out, out_ld, out_64, '%s, every column' % (options,))
        for a, b in sr.MLP_RANGES:
            v, o = run(cfg, mixed, columns=(a, b))
            assert same_bits(v, value[:, a:b]) and same_bits(o, out[:, :, a:b]), (a, b)
            jr.assert_within(o, out_ld[:, :, a:b], out_64[:, :, a:b], 'columns [%d, %d)' % (a, b))


def test_relu_is_exactly_zero():
    """relu'' = 0: a network of relu layers alone, without y function, is piecewise linear, and every second derivative is exactly 0."""
    for options in (dict(activations='relu'), dict(activations='relu', widths=(33, 64), B=22, K=3)):
        cfg = sr.mlp_config(**options)
        for mixed in (False, True):
            value, out = run(cfg, mixed)
            assert not out.any(), options
        out_ld = sr.mlp_truth(cfg, True)[0]
        assert not out_ld.any()


def test_nan_contract():
    """A NaN in row b of X makes the K rows of point b NaN (for every activation, relu with its comparison included) and no other; a NaN in tangent (b, k) of
    either set makes exactly row (b, k) NaN, and the others keep their bits."""
    for activation in mr.ACTIVATIONS:
        cfg = sr.mlp_config(B=22, K=3, activations=activation, yfunction='arcsinh')
        value, out = run(cfg, True)
        assert np.isfinite(out).all()
        X = cfg['X'].copy()
        X[7, 1] = X[21, 2] = np.nan      # (point 21: rows 63 .. 65, in two tiles)
        v, o = run(dict(cfg, X=X), True)
        hit = np.zeros(22, dtype=bool)
        hit[[7, 21]] = True
        assert np.isnan(o[hit]).all() and np.isnan(v[hit]).all(), activation
        assert same_bits(o[~hit], out[~hit]) and same_bits(v[~hit], value[~hit]), activation
        tan, tan2 = cfg['tan'].copy(), cfg['tan2'].copy()
        tan[7, 1, 0] = tan2[21, 0, 2] = tan2[21, 1, 1] = np.nan      # (rows 22, 63 and 64: the last row of a tile and the first of the next)
        v, o = run(dict(cfg, tan=tan, tan2=tan2), True)
        hit = np.zeros((22, 3), dtype=bool)
        hit[7, 1] = hit[21, 0] = hit[21, 1] = True
        assert np.isnan(o[hit]).all() and same_bits(o[~hit], out[~hit]) and same_bits(v, value), activation


def test_engine(golden):
    """MLPEmulatorEngine.jvp2: shapes, ``columns``, ``return_value`` and ``return_first`` equal to ``predict`` and ``jvp`` bit for bit, host and device tangents,
    the truth of a golden (trained) configuration."""
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    for i in range(2):
        cfg = mr.golden_config(golden('mlp'), i)
        engine = MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')
        X, (ndim, M) = cfg['Xq'], (cfg['dims'][0], cfg['dims'][-1])
        rng = np.random.default_rng(i)
        tan, tan2 = (np.asarray(cfg['xscale']) * rng.normal(0., 1., (len(X), 4, ndim)) for _ in range(2))
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
        a, b = M // 3, M - 1
        value, outc = engine.jvp2(torch.as_tensor(X, device='cuda:0'), tan, tan2, columns=(a, b), return_value=True)
        assert torch.equal(outc, out[:, :, a:b]) and torch.equal(value, engine.predict(X, columns=(a, b)))
        c = dict(cfg, X=X, tan=tan, tan2=tan2)
        for mixed, got in ((True, out), (False, same)):
            out_ld, out_64 = sr.mlp_truth(c, mixed)
            jr.assert_within(got.cpu().numpy(), out_ld, out_64, 'golden configuration %d, %s' % (i, 'mixed' if mixed else 'v = u'))
        with pytest.raises(ValueError):
            engine.jvp2(X, tan, columns=(3, 3))
        with pytest.raises(ValueError):
            engine.jvp2(X, tan, tan2[:, :2])
        with pytest.raises(ValueError):
            engine.jvp2(X, tan[:-1])
