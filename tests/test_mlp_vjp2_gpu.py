"""GPU: cp_mlp_vjp2 (csrc/cp_mlp.hip: mlp_forward_kernel in its vjp modes, mlp_dh_kernel, with a y function mlp_omega_kernel and the Gauss-Newton launches,
mlp_curvature_kernel of cp_mlp_curvature.h) against the longdouble contraction of tests/vjp2_reference.py: C[b, i, j] = sum_c q d^2 value / d x_i d x_j with
the signed cotangent q = w (data - value).

Tolerance (vjp2_reference.assert_within): the project's rule, per pair (i, j) over the batch 16 x the rounding level of the float64 restatement, floored at
1.1e-16; tests/test_vjp2_host.py holds every case to a level of at most 32 floors.

Every call (``run``) gets a copy of the network whose columns outside the range would show if read (1e300 in the output kernel, NaN in the y operations),
reads a cotangent with the row stride ncols + 3 (the padding NaN), writes the matrices followed by 64 sentinels and the value with the row stride ncols + 3,
and gets a workspace filled with NaN, announced with exactly cp_mlp_vjp2_workspace_doubles and followed by 64 sentinels.  Asserted there: all sentinels
survive, the value has the bits of cp_mlp_predict_columns, a second call (without the value) gives the same bits, every matrix is symmetric bit for bit.

Cases (vjp2_reference.mlp_cases), one thing at a time from B = 9, ndim = 3, widths (5, 17), columns [3, 20) of 25: the rows B ndim (ndim + 1) / 2 against the
tiles of 64 (one tile, one more row, three tiles, B = 1, a point across two workgroups), the columns against the slices of mlp_dh_kernel and the tiles of the
Gauss-Newton variant, the widths (more than 64 KB of LDS from width 33 on), every activation, every y function."""
import ctypes

import numpy as np
import pytest

import gauss_newton_reference as gn
import mlp_reference as mr
import vjp2_reference as cr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64
CASES = cr.mlp_cases()


def run(cfg, q, poisoned=True):
    """(value (B, ncols), C (B, ndim, ndim)) of cp_mlp_vjp2 on the columns of cfg for the cotangent ``q`` (B, ncols), with everything the module docstring
    says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    given = gn.mlp_poisoned(cfg) if poisoned else cfg
    dims, (B, ndim) = cfg['dims'], cfg['X'].shape
    L, M = len(dims) - 2, dims[-1]
    col0, stop = cfg['columns']
    ncols = stop - col0
    widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']])
    yfunction = _lib.MLP_YFUNCTIONS[cfg['yfunction'] or None]
    ld = ncols + PAD
    padded = np.full((B, ld), np.nan)
    padded[:, :ncols] = q
    names = ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale', 'cot')
    host = [np.ascontiguousarray(given[name], dtype='f8') for name in names[:-1]] + [padded]
    X, packed, xoffset, xscale, yoffset, yscale, cotd = t = [torch.as_tensor(a, device=device) for a in host]
    net = (B, ndim, L, widths, acts, M, packed.data_ptr(), xoffset.data_ptr(), xscale.data_ptr(), yoffset.data_ptr(), yscale.data_ptr(), yfunction, col0, ncols)
    need = int(lib.cp_mlp_vjp2_workspace_doubles(B, ndim, L, widths, M, ncols, yfunction))
    assert need > 0
    results = []
    for with_value in (True, False):
        value = torch.full((B * ld + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        hess = torch.full((B * ndim * ndim + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        work = torch.full((need + TAIL,), np.nan, dtype=torch.float64, device=device)
        work[need:] = SENTINEL
        _lib.check(lib.cp_mlp_vjp2(X.data_ptr(), *net, cotd.data_ptr(), ld, value.data_ptr() if with_value else None, ld, hess.data_ptr(), work.data_ptr(), need, 0,
                                   dv.stream_of(device)))
        torch.cuda.synchronize(device)
        value, hess, work = value.cpu().numpy(), hess.cpu().numpy(), work.cpu().numpy()
        assert (value[B * ld:] == SENTINEL).all() and (hess[B * ndim * ndim:] == SENTINEL).all() and (work[need:] == SENTINEL).all(), 'written past the end'
        value = value[:B * ld].reshape(B, ld)
        assert (value[:, ncols:] == SENTINEL).all(), 'padding overwritten'
        assert with_value or (value == SENTINEL).all(), 'value written though not asked for'
        results.append((value[:, :ncols].copy(), hess[:B * ndim * ndim].reshape(B, ndim, ndim).copy()))
    assert same_bits(results[0][1], results[1][1]), 'two calls differ'
    assert same_bits(results[0][1], np.ascontiguousarray(results[0][1].transpose(0, 2, 1))), 'not symmetric bit for bit'
    for name, before, after in zip(names, host, t):
        assert same_bits(before, after.cpu().numpy()), name      # the inputs are read only
    want = torch.empty((B, ncols), dtype=torch.float64, device=device)
    _lib.check(lib.cp_mlp_predict_columns(X.data_ptr(), *net, want.data_ptr(), ncols, 0, dv.stream_of(device)))
    assert same_bits(results[0][0], want.cpu().numpy()), 'value is not cp_mlp_predict_columns'
    return results[0]


@pytest.mark.parametrize('options', CASES, ids=[cr.case_id(case) for case in CASES])
def test_against_truth(options):
    cfg, case = cr.mlp_case(**options)
    value, C = run(cfg, case['q'])
    cr.assert_within(C, case, str(options))
    if options.get('activations') == 'relu':
        assert not C.any(), 'relu without a y function is exactly 0'
    twice = run(cfg, 2. * case['q'])[1]
    assert same_bits(twice, 2. * C), 'twice the cotangent is not exactly twice the result'


def cut(cfg):
    """the network of cfg cut to its columns: M = ncols outputs"""
    a, b = cfg['columns']
    dims = cfg['dims']
    L, M = len(dims) - 2, dims[-1]
    sl = mr.blocks(dims)
    small = dims[:-1] + (b - a,)
    packed, to = np.zeros(mr.nparams(small)), mr.blocks(small)
    for name in sl:
        if name == 'kernel%d' % L:
            packed[to[name]] = cfg['packed'][sl[name]].reshape(dims[-2], M)[:, a:b].ravel()
        elif name == 'bias%d' % L:
            packed[to[name]] = cfg['packed'][sl[name]][a:b]
        else:
            packed[to[name]] = cfg['packed'][sl[name]]
    return dict(cfg, dims=small, packed=packed, yoffset=cfg['yoffset'][a:b], yscale=cfg['yscale'][a:b], columns=(0, b - a))


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_a_range_is_the_network_cut_to_it(yfunction):
    for options in (dict(), dict(ncols=65), dict(ncols=257, widths=(33, 64))):
        cfg, case = cr.mlp_case(yfunction=yfunction, **options)
        value, C = run(cfg, case['q'])
        value_cut, C_cut = run(cut(cfg), case['q'], poisoned=False)
        assert same_bits(C, C_cut) and same_bits(value, value_cut), (yfunction, options)


@pytest.mark.parametrize('yfunction', ['', 'log10', 'arcsinh'])
def test_a_point_keeps_its_bits(yfunction):
    """the points 2 .. 6 of B = 9 alone (other tiles, other lanes, other workgroups at ndim = 7) have the bits they have among the nine"""
    for options in (dict(), dict(ndim=7, B=10)):
        cfg, case = cr.mlp_case(yfunction=yfunction, **options)
        value, C = run(cfg, case['q'])
        for keep in (slice(2, 7), slice(3, 4)):
            v, c = run(dict(cfg, X=cfg['X'][keep]), case['q'][keep])
            assert same_bits(c, C[keep]) and same_bits(v, value[keep]), (yfunction, options, keep)


def test_nan_contract():
    """A NaN in row b of X makes exactly point b's matrix NaN, for every activation (relu with its comparisons included) and y function, and the other points
    keep their bits; the same for a NaN in row b of the cotangent."""
    for activation in mr.ACTIVATIONS:
        for yfunction in ('', 'log10', 'arcsinh'):
            cfg, case = cr.mlp_case(B=23, activations=activation, yfunction=yfunction)      # 138 rows: three tiles, point 10 across two of them
            value, C = run(cfg, case['q'])
            assert np.isfinite(C).all()
            hit = np.zeros(23, dtype=bool)
            hit[[7, 10, 22]] = True
            X = cfg['X'].copy()
            X[7, 1] = X[10, 0] = X[22, 2] = np.nan
            v, c = run(dict(cfg, X=X), case['q'])
            assert np.isnan(c[hit]).all() and np.isnan(v[hit]).all(), (activation, yfunction)
            assert same_bits(c[~hit], C[~hit]) and same_bits(v[~hit], value[~hit]), (activation, yfunction)
            q = case['q'].copy()
            q[7, 16] = q[10, 0] = q[22, 5] = np.nan
            v, c = run(cfg, q)
            assert np.isnan(c[hit]).all() and same_bits(c[~hit], C[~hit]) and same_bits(v, value), (activation, yfunction)


def test_engine():
    """MLPEmulatorEngine.vjp2: the bits of the C entry point, shapes, ``columns``, ``return_value`` equal to ``predict`` bit for bit, a strided cotangent."""
    import torch
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    for yfunction in ('', 'log10'):
        cfg, case = cr.mlp_case(yfunction=yfunction, ndim=7, B=10)
        engine = MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')
        X, (a, b), (ndim, M) = cfg['X'], cfg['columns'], (cfg['dims'][0], cfg['dims'][-1])
        value, C = run(cfg, case['q'], poisoned=False)
        got = engine.vjp2(X, case['q'], columns=(a, b))
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (len(X), ndim, ndim) and got.is_contiguous()
        assert same_bits(got.cpu().numpy(), C)
        wide = torch.zeros((len(X), M), dtype=torch.float64, device='cuda:0')
        wide[:, a:b] = torch.as_tensor(case['q'], device='cuda:0')
        v, strided = engine.vjp2(torch.as_tensor(X, device='cuda:0'), wide[:, a:b], columns=(a, b), return_value=True)      # (a view with the row stride M)
        assert torch.equal(strided, got) and torch.equal(v, engine.predict(X, columns=(a, b)))
        every = engine.vjp2(X, wide)      # every column, zero outside the range: the same truth
        cr.assert_within(every.cpu().numpy(), case, 'every column')
        assert torch.equal(every, every.transpose(1, 2))
        with pytest.raises(ValueError):
            engine.vjp2(X, case['q'][:, :0], columns=(3, 3))
        with pytest.raises(ValueError):
            engine.vjp2(X, case['q'][:, :-1], columns=(a, b))
        with pytest.raises(ValueError):
            engine.vjp2(X[:, :-1], case['q'], columns=(a, b))
