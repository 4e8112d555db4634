"""Truth and cases of the emulators' Jacobian-vector products for the tests (tests/test_jvp_host.py, test_mlp_jvp_gpu.py, test_taylor_jvp_gpu.py,
test_emulator_jvp_gpu.py), on top of the forward-mode passes of tests/jacobian_reference.py: ``out[b, k, c] = sum_i tan[b, k, i] J[b, i, c]`` in any
floating-point type.  ``np.longdouble`` is the truth, float64 the restatement that gives the rounding level.

Tolerance: the rule of tests/jacobian_reference.py (``levels``, ``assert_within``) with a block being one (direction k, output column) pair over the batch:
the level is the float64 restatement's largest distance from the truth relative to the block's largest entry, floored at 1.1e-16, and the device is
allowed 16 x that level.  Tangents are drawn as xscale x N(0, 1) (Taylor: no x operation, N(0, 1)).

The cases are kept here so that tests/test_jvp_host.py can hold the level of every shape the device tests use to at most 32.  A case with ``seed=`` was
redrawn because its first draw lay above that (the float64 restatement's own error, not the device's: with a first hidden layer of ONE neuron, through
whose pre-activation every derivative passes, the Jacobian's level itself is mostly above 32, and seed 20 was the first of 20 draws below)."""
import numpy as np

import jacobian_reference as jr
from mlp_device import draw_network

LD = jr.LD


def jvp(J, tan, dtype):
    """(B, K, M) = sum_i tan[b, k, i] J[b, i, c] in ``dtype``, summed over i in parameter order."""
    tan = np.asarray(tan).astype(dtype)
    out = np.zeros(tan.shape[:2] + J.shape[2:], dtype=dtype)
    for i in range(tan.shape[2]):
        out = out + tan[:, :, i, None] * J[:, None, i, :]
    return out


def mlp_args(cfg):
    return (cfg['packed'], cfg['dims'], cfg['activations'], cfg['X'], cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])


def mlp_config(B=65, ndim=3, K=2, widths=(5, 17), M=257, activations='silu', yfunction='', seed=0):
    rng = np.random.default_rng(100000 * K + 1000 * B + 100 * ndim + 10 * sum(widths) + M + seed)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = [activations] * len(widths) if isinstance(activations, str) else list(activations)
    lo, xscale = rng.uniform(-1., 1., ndim), rng.uniform(0.5, 2., ndim)
    cfg = dict(dims=dims, activations=activations, packed=draw_network(rng, dims), yfunction=yfunction, xoffset=lo, xscale=xscale,
               yoffset=rng.normal(0., 1., M), yscale=rng.uniform(0.5, 2., M))
    cfg['X'] = lo + xscale * rng.uniform(0., 1., (B, ndim))
    cfg['tan'] = xscale * rng.normal(0., 1., (B, K, ndim))
    return cfg


def mlp_truth(cfg):
    """(out_ld, out_64), each (B, K, M)"""
    return tuple(jvp(jr.mlp_jacobian(*mlp_args(cfg), dtype=dtype)[1], cfg['tan'], dtype) for dtype in (LD, 'f8'))


def taylor_config(B=65, ndim=3, K=2, T=65, M=257, seed=0):
    rng = np.random.default_rng(100000 * K + 1000 * B + 100 * ndim + 10 * T + M + seed)
    powers = rng.integers(0, 4, (T, ndim)).astype('i4')
    powers[0] = 0
    if T > 1:
        powers[T // 2, rng.integers(ndim)] = 15
    return dict(center=rng.uniform(-0.5, 0.5, ndim), powers=powers, derivatives=rng.normal(0., 1., (T, M)), X=rng.uniform(-1., 1., (B, ndim)),
                tan=rng.normal(0., 1., (B, K, ndim)))


def taylor_truth(cfg):
    """(out_ld, out_64), each (B, K, M)"""
    args = (cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'])
    return tuple(jvp(jr.taylor_jacobian(*args, dtype=dtype), cfg['tan'], dtype) for dtype in (LD, 'f8'))


def case_id(case):
    return '-'.join('%s=%s' % item for item in case.items()).replace(' ', '') or 'base'


BK = [dict(B=63, K=1), dict(B=64, K=1), dict(B=22, K=3), dict(B=43, K=3)]      # B K = 63, 64, 66, 129 rows: the last row of a tile, a point in two tiles
KS = [dict(K=K) for K in (1, 5, 7, 64, 65)]
TAYLOR_KS = [dict(K=1), dict(K=5), dict(K=7, seed=2), dict(K=64), dict(K=65, seed=1)]
MLP_CASES = ([dict()] + BK + KS + [dict(ndim=1, seed=4)] + [dict(ndim=n) for n in (2, 5, 32)] + [dict(widths=(5, w)) for w in (3, 8, 9, 33, 64)]
             + [dict(widths=(1, 17), seed=20), dict(widths=(64, 17))] + [dict(M=1), dict(M=16), dict(M=255, seed=1), dict(M=256)]
             + [dict(widths=(17,)), dict(widths=(5, 9, 17, 6, 33, 12, 7, 17), seed=2)]
             + [dict(activations=a) for a in ('relu', 'tanh', 'identity-silu')] + [dict(activations=['identity-silu', 'relu', 'tanh', 'silu'], widths=(9, 12, 7, 17))]
             + [dict(yfunction=y) for y in ('log10', 'arcsinh')] + [dict(yfunction='log10', activations='identity-silu', widths=(33, 64))])
MLP_RANGES = [(0, 1), (255, 257), (16, 17)]
TAYLOR_CASES = [dict()] + BK + TAYLOR_KS + [dict(ndim=n) for n in (1, 2, 32)] + [dict(T=1), dict(T=31), dict(T=32, seed=1), dict(T=33)] + [dict(M=M) for M in (1, 255, 256)]
