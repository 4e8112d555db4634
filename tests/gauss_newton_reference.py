"""Truth and cases of the emulators' Fisher matrices and Gauss-Newton normal equations for the tests (tests/test_gauss_newton_host.py,
test_mlp_gauss_newton_gpu.py, test_taylor_gauss_newton_gpu.py, test_emulator_gauss_newton_gpu.py), on top of the forward-mode passes of
tests/jacobian_reference.py: per point b over the columns c of a range

    fisher[b, i, j] = sum_c w[b, c] J[b, i, c] J[b, j, c],  grad[b, i] = sum_c w[b, c] (data[b, c] - value[b, c]) J[b, i, c],
    chi2[b] = sum_c w[b, c] (data[b, c] - value[b, c])^2

in any floating-point type (:func:`contract`); a column whose weight is exactly 0 is dropped, whatever it holds.  ``np.longdouble`` (the longdouble Jacobian
and value contracted in longdouble) is the truth, float64 (the float64 restatement contracted in float64) the yardstick that is not the code under test.

Tolerance: the rule of tests/jacobian_reference.py (``levels``, ``assert_within``: FLOOR = 1.1e-16, ALLOW = 16).  A block is one (i, j) entry of fisher, one i
of grad, or chi2, taken over the batch; its level is the restatement's largest distance from the truth relative to the block's largest magnitude, floored
at FLOOR; the device gets ALLOW levels.  A case whose level exceeds 32 x FLOOR is not used: tests/test_gauss_newton_host.py holds every case listed here
to that, and a case above it has its inputs redrawn (``seed=``), never the cap moved.

Scales.  A residual of 5 % of the value magnifies the value's own rounding twentyfold in grad and chi2, so the cap asks for a value good to about one
rounding.  MLP: the part of an output that varies with the parameters is SIGNAL = 2^-8 of its offset (yscale; the offset itself an eighth under a y
function, whose argument's rounding the function magnifies), so the value is its last rounding.  Taylor: every input is dyadic (:func:`taylor_config`)
and the value exact.

Operands: data = value_truth x (1 + 0.05 xi), xi standard normal, so that residuals stay far above rounding; weights 10^U(-2, 1), positive, three decades.
A case is drawn on M = col0 + ncols + 5 columns and evaluated on [col0, col0 + ncols); :func:`poisoned` gives the device a copy whose other columns would
show if read (1e300 in the output kernel or the derivatives, NaN in the y operations)."""
import numpy as np

import jacobian_reference as jr
import mlp_reference as mr
from mlp_device import draw_network

LD = jr.LD
SIGNAL = 2.**-8      # MLP: the part of an output that varies with the parameters, relative to its offset (module docstring)


def contract(J, value, weights, data, dtype):
    """(fisher (B, n, n), grad (B, n), chi2 (B,)) in ``dtype`` from J (B, n, ncols), value (B, ncols), weights and data (ncols,) or (B, ncols); columns of
    weight exactly 0 dropped.  ``data`` None: (fisher, None, None)."""
    J, value = np.asarray(J).astype(dtype), np.asarray(value).astype(dtype)
    B, n, ncols = J.shape
    w = np.broadcast_to(np.asarray(weights).astype(dtype), (B, ncols))
    keep = w != 0
    w = np.where(keep, w, 0)
    J = np.where(keep[:, None, :], J, 0)
    fisher = np.einsum('bc,bic,bjc->bij', w, J, J)
    if data is None:
        return fisher, None, None
    resid = np.where(keep, np.broadcast_to(np.asarray(data).astype(dtype), (B, ncols)) - value, 0)
    return fisher, np.einsum('bc,bc,bic->bi', w, resid, J), np.einsum('bc,bc,bc->b', w, resid, resid)


def operands(rng, value_ld, shared_weights=False, shared_data=False):
    """(weights, data) for a value (B, ncols): per point, or one row shared by all points (the data then scattered around the first point's value)."""
    B, ncols = value_ld.shape
    weights = 10.**rng.uniform(-2., 1., (ncols,) if shared_weights else (B, ncols))
    around = np.asarray(value_ld[0] if shared_data else value_ld, dtype='f8')
    return weights, around * (1. + 0.05 * rng.standard_normal(around.shape))


def mlp_config(B=9, ndim=3, widths=(5, 17), col0=3, ncols=17, activations='silu', yfunction='', shared_weights=False, shared_data=False, seed=0):
    M = col0 + ncols + 5
    rng = np.random.default_rng(1000000 * seed + 1000 * B + 100 * ndim + 10 * sum(widths) + M)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = [activations] * len(widths) if isinstance(activations, str) else list(activations)
    lo, xscale = rng.uniform(-1., 1., ndim), rng.uniform(0.5, 2., ndim)
    cfg = dict(dims=dims, activations=activations, packed=draw_network(rng, dims), yfunction=yfunction, xoffset=lo, xscale=xscale,
               yoffset=rng.normal(0., 1., M) * (0.125 if yfunction else 1.), yscale=rng.uniform(0.5, 2., M) * SIGNAL, columns=(col0, col0 + ncols))
    cfg['X'] = lo + xscale * rng.uniform(0., 1., (B, ndim))
    cfg['rng'] = rng
    cfg['shared'] = (shared_weights, shared_data)
    return cfg


def mlp_args(cfg):
    return (cfg['packed'], cfg['dims'], cfg['activations'], cfg['X'], cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])


def mlp_truth(cfg):
    """Adds ``weights`` and ``data`` to cfg (drawn once, around the longdouble value) and returns ((fisher, grad, chi2) in longdouble, the same in float64,
    value in longdouble), on the columns of the case."""
    a, b = cfg['columns']
    value_ld, J_ld = jr.mlp_jacobian(*mlp_args(cfg), dtype=LD)
    value_64, J_64 = jr.mlp_jacobian(*mlp_args(cfg), dtype='f8')
    if 'weights' not in cfg:
        cfg['weights'], cfg['data'] = operands(cfg['rng'], value_ld[:, a:b], *cfg['shared'])
    return (contract(J_ld[:, :, a:b], value_ld[:, a:b], cfg['weights'], cfg['data'], LD),
            contract(J_64[:, :, a:b], value_64[:, a:b], cfg['weights'], cfg['data'], 'f8'), value_ld[:, a:b])


def mlp_poisoned(cfg):
    """cfg with everything outside its columns made to show if read: 1e300 in the output kernel and bias, NaN in yoffset and yscale."""
    a, b = cfg['columns']
    dims = cfg['dims']
    L, M = len(dims) - 2, dims[-1]
    packed, sl = cfg['packed'].copy(), mr.blocks(dims)
    outside = np.ones(M, dtype=bool)
    outside[a:b] = False
    kernel = packed[sl['kernel%d' % L]].reshape(dims[-2], M)
    kernel[:, outside] = 1e300
    packed[sl['kernel%d' % L]] = kernel.ravel()
    bias = packed[sl['bias%d' % L]]
    bias[outside] = 1e300
    packed[sl['bias%d' % L]] = bias
    yoffset, yscale = cfg['yoffset'].copy(), cfg['yscale'].copy()
    yoffset[outside] = yscale[outside] = np.nan
    return dict(cfg, packed=packed, yoffset=yoffset, yscale=yscale)


def taylor_config(B=9, ndim=3, T=20, order=3, col0=3, ncols=17, shared_weights=False, shared_data=False, seed=0):
    """T terms of total degree 1 .. ``order`` spread over random parameters, the first one the constant.  Everything is dyadic with few bits -- the centre in
    eighths, the points in sixteenths, the derivatives in 1024ths of at most 4 -- so that the polynomial and its Jacobian are EXACT in float64 in any order
    of summation (at most 18 + 2 + 13 + 7 bits): the value's rounding, which a residual of 5 % magnifies twentyfold, is not in the way of the cap."""
    M = col0 + ncols + 5
    rng = np.random.default_rng(1000000 * seed + 1000 * B + 100 * ndim + 10 * T + M + 7 * order)
    powers = np.zeros((T, ndim), dtype='i4')
    for t in range(1, T):
        for i in rng.integers(0, ndim, rng.integers(1, order + 1)):
            powers[t, i] += 1
    return dict(center=rng.integers(-4, 5, ndim) / 8., powers=powers, derivatives=rng.integers(-4096, 4097, (T, M)) / 1024., X=rng.integers(-16, 17, (B, ndim)) / 16.,
                columns=(col0, col0 + ncols), rng=rng, shared=(shared_weights, shared_data))


def taylor_truth(cfg):
    a, b = cfg['columns']
    args = (cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'])
    value_ld, J_ld = jr.taylor_predict(*args, dtype=LD), jr.taylor_jacobian(*args, dtype=LD)
    value_64, J_64 = jr.taylor_predict(*args, dtype='f8'), jr.taylor_jacobian(*args, dtype='f8')
    if 'weights' not in cfg:
        cfg['weights'], cfg['data'] = operands(cfg['rng'], value_ld[:, a:b], *cfg['shared'])
    return (contract(J_ld[:, :, a:b], value_ld[:, a:b], cfg['weights'], cfg['data'], LD),
            contract(J_64[:, :, a:b], value_64[:, a:b], cfg['weights'], cfg['data'], 'f8'), value_ld[:, a:b])


def taylor_poisoned(cfg):
    a, b = cfg['columns']
    derivatives = cfg['derivatives'].copy()
    derivatives[:, :a] = derivatives[:, b:] = 1e300
    return dict(cfg, derivatives=derivatives)


def blocks(result):
    """The three results with the batch leading and a block per remaining index: fisher (B, n, n), grad (B, n), chi2 (B, 1)."""
    fisher, grad, chi2 = result
    return fisher, grad, np.asarray(chi2)[:, None]


def worst_level(truth, restated):
    """The largest level over the blocks of the three results, in units of FLOOR."""
    return max(float(jr.levels(t, r)[1].max()) for t, r in zip(blocks(truth), blocks(restated))) / jr.FLOOR


def assert_within(device, truth, restated, what=''):
    for name, d, t, r in zip(('fisher', 'grad', 'chi2'), blocks(device), blocks(truth), blocks(restated)):
        jr.assert_within(d, t, r, '%s %s' % (what, name))


def case_id(case):
    return '-'.join('%s=%s' % item for item in case.items()).replace(' ', '') or 'base'


# ladders that vary one thing at a time from the small base case (B = 9, ndim = 3, widths (5, 17) or T = 20 of order 3, columns [3, 20) of 25, silu, no y
# function).  A case with ``seed=`` was redrawn because its first draw lay above the cap (the restatement's own error: at ndim = 32 a block of fisher is a
# maximum over two or three points only, and seeds 43 and 24 were the first of their draws below 26).
POINTS = [dict(ndim=1, B=1), dict(ndim=1, B=64), dict(ndim=1, B=65), dict(ndim=3, B=21), dict(ndim=3, B=22), dict(ndim=7, B=9), dict(ndim=7, B=10), dict(ndim=7, B=19),
          dict(ndim=8, B=17), dict(ndim=32, B=2), dict(ndim=32, B=3)]      # P = 64, 21, 9, 8, 2 points per tile: one tile, one tile + 1, three tiles
COLUMNS = [dict(ncols=n) for n in (1, 15, 16, 63, 64, 65, 255, 256, 257, 520)] + [dict(col0=0), dict(col0=0, ncols=257)]      # (the base: col0 = 3, ncols = 17)
STRIDES = [dict(shared_weights=True), dict(shared_data=True), dict(shared_weights=True, shared_data=True, B=22)]
MLP_SEEDS = {'ndim=1-B=1': 1, 'ndim=32-B=2': 43, 'ndim=32-B=3': 24, 'ncols=15': 1, 'ncols=64': 1, 'shared_data=True': 1, 'shared_weights=True-shared_data=True-B=22': 5,
             'activations=tanh': 1}
TAYLOR_SEEDS = {'ndim=32-B=2': 1, 'ndim=32-B=3': 1}


def _seeded(cases, seeds):
    return [dict(case, seed=seeds[case_id(case)]) if case_id(case) in seeds else case for case in cases]


MLP_CASES = _seeded([dict()] + POINTS + COLUMNS + STRIDES + [dict(widths=w) for w in ((5,), (33, 64), (64, 64, 64))] + [dict(activations=a) for a in ('relu', 'tanh', 'identity-silu')]
                    + [dict(yfunction=y) for y in ('log10', 'arcsinh')] + [dict(yfunction='log10', ncols=257, widths=(33, 64), activations='identity-silu')], MLP_SEEDS)
TAYLOR_CASES = _seeded([dict()] + POINTS + COLUMNS + STRIDES + [dict(order=o) for o in (1, 2)] + [dict(T=T) for T in (1, 31, 32, 33, 70)], TAYLOR_SEEDS)
