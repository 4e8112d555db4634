"""Truth and cases of the emulators' second directional derivatives for the tests (tests/test_jvp2_host.py, test_mlp_jvp2_gpu.py, test_taylor_jvp2_gpu.py,
test_emulator_jvp2_gpu.py), on top of tests/jacobian_reference.py and tests/mlp_reference.py:
``out[b, k, c] = sum_ij u[b, k, i] v[b, k, j] d^2 y[b, c] / d x[b, i] d x[b, j]`` by second-order forward mode in any floating-point type.  ``np.longdouble`` is
the truth, float64 the restatement that gives the rounding level; neither is the code under test.

Tolerance: the rule of tests/jacobian_reference.py (``levels``, ``assert_within``), unchanged, with a block being one (pair of directions k, output column)
over the batch: the level is the float64 restatement's largest distance from the truth relative to the block's largest entry, floored at 1.1e-16, and the
device is allowed 16 x that level.  tests/test_jvp2_host.py holds the level of every case below to at most 32 floors, with ``v = u`` and with the second
tangent set; second order roughly doubles the levels of the Jacobian-vector product, so more cases than there needed another draw: a case's ``seed`` is
the first one, counted from 0, at which both runs lie below the cap (the cap is never moved).

The cases are the shapes of tests/jvp_reference.py (``MLP_CASES``, ``MLP_RANGES``, ``TAYLOR_CASES``) with the seeds of this file in the place of theirs.  The
first tangent set is that of ``jvp_reference.mlp_config`` / ``taylor_config``; the second is drawn here in the same way, xscale x N(0, 1) (Taylor: N(0, 1))."""
import numpy as np

import jacobian_reference as jr
import jvp_reference as pr
import mlp_reference as mr

LD = jr.LD


def activate_second(name, v, alpha, beta):
    """act''(v) in the type of v; relu: exactly 0, and a NaN stays one."""
    if name == 'silu':
        s = mr.sigmoid(v)
        return s * (1 - s) * (2 + v * (1 - 2 * s))
    if name == 'relu':
        return np.where(v != v, v, np.zeros_like(v))
    if name == 'tanh':
        t = np.tanh(v)
        return -2 * t * (1 - t * t)
    s = mr.sigmoid(alpha * v)
    return beta * alpha * s * (1 - s) * (2 + alpha * v * (1 - 2 * s))


def mlp_jvp2(packed, dims, activations, X, xoffset, xscale, yoffset, yscale, yfunction, tan_u, tan_v=None, dtype='f8'):
    """(B, K, M) second directional derivatives of the engine's prediction along the pairs (tan_u[b, k], tan_v[b, k]) in ``dtype``; ``tan_v=None``: tan_u."""
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    layers = mr.unpack(packed, dims, dtype)
    ndim = dims[0]
    xs = t(np.broadcast_to(xscale, (ndim,)))
    h = (t(X) - t(xoffset)) / xs
    du = t(tan_u) / xs      # (B, K, neuron)
    dv = du if tan_v is None else t(tan_v) / xs
    d2 = np.zeros_like(du)
    for (kernel, bias, alpha, beta), name in zip(layers[:-1], activations):
        z = h @ kernel + bias
        zu, zv, z2 = du @ kernel, dv @ kernel, d2 @ kernel
        h = mr.activate(name, z, alpha, beta)
        first = jr.activate_derivative(name, z, alpha, beta)[:, None, :]
        second = activate_second(name, z, alpha, beta)[:, None, :]
        du, dv, d2 = first * zu, first * zv, second * (zu * zv) + first * z2
    kernel = layers[-1][0]
    v = ((h @ kernel + layers[-1][1]) * t(yscale) + t(yoffset))[:, None, :]
    vu, vv, a = (du @ kernel) * t(yscale), (dv @ kernel) * t(yscale), (d2 @ kernel) * t(yscale)
    if yfunction == 'log10':      # f = 10^v: f' = ln 10 f, f'' = ln 10^2 f
        ln10 = np.log(np.asarray(10, dtype=dtype))
        value = 10**v
        return ln10 * value * a + ln10 * ln10 * value * (vu * vv)
    if yfunction == 'arcsinh':      # f = sinh v
        return np.cosh(v) * a + np.sinh(v) * (vu * vv)
    return a


def taylor_left2(center, powers, X, tan_u, tan_v=None, dtype='f8'):
    """(B, K, T): entry (b, k, t) = sum over the parameters i <= j with p_ti, p_tj > 0 of c_ij d^2 mono_t / d x_i d x_j, c_ii = u_i v_i, c_ij = u_i v_j + u_j v_i.
    Factors of power 0 are skipped (neither x nor the tangents of such a parameter are read), the diagonal of a parameter with p_ti < 2 as well."""
    powers = np.asarray(powers)
    d = np.asarray(X).astype(dtype) - np.asarray(center).astype(dtype)
    u = np.asarray(tan_u).astype(dtype)
    v = u if tan_v is None else np.asarray(tan_v).astype(dtype)
    B, K, ndim = u.shape
    left = np.zeros((B, K, len(powers)), dtype=dtype)
    for t, power in enumerate(powers):
        marked = [q for q, p in enumerate(power) if p > 0]
        table = {(q, r): (d[:, q]**int(power[q] - r) if power[q] > r else np.ones(B, dtype=dtype)) for q in marked for r in range(3) if power[q] >= r}
        for a, i in enumerate(marked):
            for j in marked[a:]:
                if i == j and power[i] < 2:
                    continue
                m = np.ones(B, dtype=dtype)
                for q in marked:
                    r = (q == i) + (q == j)
                    p = int(power[q])
                    m = m * table[q, r] * (1 if r == 0 else p if r == 1 else p * (p - 1))
                c = u[:, :, i] * v[:, :, i] if i == j else u[:, :, i] * v[:, :, j] + u[:, :, j] * v[:, :, i]
                left[:, :, t] = left[:, :, t] + c * m[:, None]
    return left


def taylor_jvp2(center, powers, derivatives, X, tan_u, tan_v=None, dtype='f8'):
    """(B, K, M) second directional derivatives of the polynomial in ``dtype``."""
    return taylor_left2(center, powers, X, tan_u, tan_v, dtype) @ np.asarray(derivatives).astype(dtype)


def second_tangents(cfg, seed):
    """The second tangent set of a configuration of tests/jvp_reference.py: independent of the first, drawn like it."""
    rng = np.random.default_rng(7000003 + 101 * seed + cfg['tan'].size)
    return np.asarray(cfg.get('xscale', 1.)) * rng.normal(0., 1., cfg['tan'].shape)


def mlp_config(**options):
    cfg = pr.mlp_config(**options)
    cfg['tan2'] = second_tangents(cfg, options.get('seed', 0))
    return cfg


def taylor_config(**options):
    cfg = pr.taylor_config(**options)
    cfg['tan2'] = second_tangents(cfg, options.get('seed', 0))
    return cfg


def mlp_truth(cfg, mixed):
    """(out_ld, out_64), each (B, K, M); ``mixed``: along (tan, tan2), else along (tan, tan)"""
    return tuple(mlp_jvp2(*pr.mlp_args(cfg), cfg['tan'], cfg['tan2'] if mixed else None, dtype=dtype) for dtype in (LD, 'f8'))


def taylor_truth(cfg, mixed):
    args = (cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'])
    return tuple(taylor_jvp2(*args, cfg['tan'], cfg['tan2'] if mixed else None, dtype=dtype) for dtype in (LD, 'f8'))


case_id = pr.case_id
# the seed of a case: the first, from 0, at which the level is at most 32 floors with v = u AND with the second set (tools/search_jvp2_seeds.py; none: 0)
MLP_SEEDS = {'K=5': 2, 'K=7': 1, 'K=64': 2, 'K=65': 1, 'ndim=1': 9, 'widths=(5,33)': 1, 'widths=(1,17)': 5, 'widths=(5,9,17,6,33,12,7,17)': 12,
             "activations=['identity-silu','relu','tanh','silu']-widths=(9,12,7,17)": 2, 'yfunction=log10-activations=identity-silu-widths=(33,64)': 7}
TAYLOR_SEEDS = {'B=63-K=1': 1, 'B=43-K=3': 1, 'K=7': 2, 'ndim=32': 2, 'T=32': 1}


def _seeded(cases, seeds):
    toret = []
    for case in cases:
        case = {name: value for name, value in case.items() if name != 'seed'}
        seed = seeds.get(case_id(case), 0)
        toret.append(dict(case, seed=seed) if seed else case)
    return toret


MLP_CASES = _seeded(pr.MLP_CASES, MLP_SEEDS)
TAYLOR_CASES = _seeded(pr.TAYLOR_CASES, TAYLOR_SEEDS)
MLP_RANGES = pr.MLP_RANGES
# the configurations of the column ranges of tests/test_mlp_jvp2_gpu.py, one per y function
MLP_RANGE_CASES = _seeded([dict(yfunction=y, activations='tanh') for y in ('', 'log10', 'arcsinh')], MLP_SEEDS)
