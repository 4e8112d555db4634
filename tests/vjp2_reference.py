"""Truth and cases of the emulators' contracted second derivatives for the tests (tests/test_vjp2_host.py, test_mlp_vjp2_gpu.py, test_taylor_vjp2_gpu.py,
test_emulator_vjp2_gpu.py), on top of the second-order passes of tests/jvp2_reference.py and the configurations of tests/gauss_newton_reference.py: per
point b over the columns c of a range

    C[b, i, j] = sum_c q[b, c] d^2 value[b, c] / d x[b, i] d x[b, j]

as ``einsum('bc,bpc->bp', q, jvp2 on the unit pairs i <= j)`` in any floating-point type (:func:`contract`), p running over the pairs in the order
(0, 0), (0, 1), ..., (1, 1), ...  ``np.longdouble`` is the truth, float64 the yardstick that is not the code under test.

Tolerance: the rule of tests/jacobian_reference.py (``levels``, ``assert_within``: FLOOR = 1.1e-16, ALLOW = 16).  A block is one pair (i, j) taken over the
batch; its level is the restatement's largest distance from the truth relative to the block's largest magnitude, floored at FLOOR; the device gets ALLOW
levels.  A case whose level exceeds 32 x FLOOR is not used: tests/test_vjp2_host.py holds every case listed here to that, and a case above it has its
inputs redrawn (``seed=``; tools/search_vjp2_seeds.py prints the table), never the cap moved.

Configurations: those of gauss_newton_reference (MLP: SIGNAL scaling; Taylor: dyadic inputs), and the cotangent is the realistic, signed one,
q = w (data - value) from its ``operands`` (the value the longdouble one rounded to float64: the cotangent is an INPUT, the same for truth, yardstick and
device).

The sign and convention of ``Emulator.chi2_hessian`` (hessian = fisher - C = -d gradient / d theta) are pinned on the restatement by
:func:`gradient_difference`: the central difference of the restated Gauss-Newton gradient in longdouble."""
import numpy as np

import gauss_newton_reference as gn
import jacobian_reference as jr
import jvp2_reference as j2

LD = jr.LD
CAP = 32.      # floors: a case whose level lies above is redrawn


def pairs(ndim):
    return [(i, j) for i in range(ndim) for j in range(i, ndim)]


def unit_tangents(B, ndim):
    """(U, V), each (B, npairs, ndim): the unit pairs (e_i, e_j), i <= j"""
    index = pairs(ndim)
    U, V = np.zeros((B, len(index), ndim)), np.zeros((B, len(index), ndim))
    for p, (i, j) in enumerate(index):
        U[:, p, i] = V[:, p, j] = 1.
    return U, V


def full(C, ndim):
    """(B, ndim, ndim) of the triangle (B, npairs), mirrored"""
    out = np.zeros((len(C), ndim, ndim), dtype=np.asarray(C).dtype)
    for p, (i, j) in enumerate(pairs(ndim)):
        out[:, i, j] = out[:, j, i] = C[:, p]
    return out


def triangle(H):
    """(B, npairs) of a matrix (B, ndim, ndim): its entries i <= j"""
    ndim = H.shape[-1]
    return np.stack([H[:, i, j] for i, j in pairs(ndim)], axis=1)


def contract(second, q, dtype):
    """C (B, npairs) in ``dtype`` from the second derivatives (B, npairs, ncols) and the cotangent (B, ncols)"""
    return np.einsum('bc,bpc->bp', np.asarray(q).astype(dtype), np.asarray(second).astype(dtype))


def mlp_second(cfg, dtype):
    a, b = cfg['columns']
    U, V = unit_tangents(len(cfg['X']), cfg['dims'][0])
    return j2.mlp_jvp2(*gn.mlp_args(cfg), U, V, dtype=dtype)[:, :, a:b]


def taylor_second(cfg, dtype):
    a, b = cfg['columns']
    U, V = unit_tangents(*cfg['X'].shape)
    return j2.taylor_jvp2(cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'], U, V, dtype=dtype)[:, :, a:b]


def _case(cfg, truth_of, second_of):
    normal, restated, value = truth_of(cfg)      # (adds the weights and the data to cfg)
    w, data = (np.broadcast_to(cfg[name], value.shape) for name in ('weights', 'data'))
    q = np.asarray(w * (data - np.asarray(value, dtype='f8')), dtype='f8')
    return dict(q=q, value=value, normal=normal, truth=contract(second_of(cfg, LD), q, LD), restated=contract(second_of(cfg, 'f8'), q, 'f8'))


def mlp_case(**options):
    """(cfg, case) of a configuration of gauss_newton_reference.mlp_config: case holds the cotangent ``q`` (B, ncols) float64, ``truth`` and ``restated``
    (B, npairs) in longdouble and float64, the longdouble ``value`` on the range and ``normal`` = (fisher, grad, chi2) in longdouble"""
    cfg = gn.mlp_config(**options)
    return cfg, _case(cfg, gn.mlp_truth, mlp_second)


def taylor_case(**options):
    cfg = gn.taylor_config(**options)
    return cfg, _case(cfg, gn.taylor_truth, taylor_second)


def level(case):
    """the largest level over the blocks, in floors"""
    return float(jr.levels(case['truth'], case['restated'])[1].max()) / jr.FLOOR


def assert_within(device, case, what=''):
    """``device`` (B, ndim, ndim): its triangle against the truth under the rule (the mirror is checked bit for bit by the callers)"""
    jr.assert_within(triangle(np.asarray(device)), case['truth'], case['restated'], what)


def gradient_difference(cfg, kind, step=1e-6):
    """(-(F - C) (B, ndim, ndim), d gradient / d theta by central differences (B, ndim, ndim), |hessian| top (B,)) of the restated chi2 in longdouble, with the
    weights and the data of cfg fixed: column j of the second is (g(x + h_j e_j) - g(x - h_j e_j)) / (2 h_j), h_j = step x xscale_j (1 for Taylor)."""
    a, b = cfg['columns']
    B, ndim = cfg['X'].shape
    w, data = cfg['weights'], cfg['data']

    def gradient(X):
        c = dict(cfg, X=X)
        if kind == 'mlp':
            value, J = jr.mlp_jacobian(*gn.mlp_args(c), dtype=LD)
        else:
            args = (c['center'], c['powers'], c['derivatives'], X)
            value, J = jr.taylor_predict(*args, dtype=LD), jr.taylor_jacobian(*args, dtype=LD)
        return gn.contract(J[:, :, a:b], value[:, a:b], w, data, LD)

    fisher, grad, chi2 = gradient(cfg['X'].astype(LD))
    second = (mlp_second if kind == 'mlp' else taylor_second)(cfg, LD)
    value = jr.mlp_jacobian(*gn.mlp_args(cfg), dtype=LD)[0] if kind == 'mlp' else jr.taylor_predict(cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'], dtype=LD)
    q = np.broadcast_to(w, (B, b - a)).astype(LD) * (np.broadcast_to(data, (B, b - a)).astype(LD) - value[:, a:b])
    hessian = fisher - full(contract(second, q, LD), ndim)
    scale = np.broadcast_to(np.asarray(cfg.get('xscale', 1.)), (ndim,))
    derivative = np.zeros((B, ndim, ndim), dtype=LD)
    for j in range(ndim):
        h = LD(step) * LD(scale[j])
        shift = np.zeros(ndim, dtype=LD)
        shift[j] = h
        derivative[:, :, j] = (gradient(cfg['X'].astype(LD) + shift)[1] - gradient(cfg['X'].astype(LD) - shift)[1]) / (2 * h)
    return -hessian, derivative, np.abs(hessian).max(axis=(1, 2))


case_id = gn.case_id

# ladders that vary one thing at a time from the small base case (B = 9, ndim = 3, widths (5, 17) or T = 20 of order 3, columns [3, 20) of 25, silu, no y
# function).  Rows: npairs = 1, 3, 6, 28, 36, 66, 528 rows per point against tiles of 64 rows -- one tile (or the most whole points under it), one tile and
# more, three tiles (or the first count past them); with npairs = 66 every point spans two workgroups.  A case with ``seed=`` was redrawn because its first
# draw lay above the cap (the restatement's own error: with B = 1 a block is ONE entry, a signed sum that may cancel; at ndim = 32 and B = 1 no draw of 64 lay
# below the cap for the MLP -- 528 single entries, one of which always cancels -- so ndim = 32 is run with two points)
ROWS = [dict(ndim=1, B=1), dict(ndim=1, B=64), dict(ndim=1, B=65), dict(ndim=1, B=192), dict(ndim=2, B=21), dict(ndim=2, B=22), dict(ndim=2, B=64), dict(ndim=3, B=11),
        dict(ndim=3, B=32), dict(ndim=7, B=2), dict(ndim=7, B=3), dict(ndim=7, B=7), dict(ndim=8, B=1), dict(ndim=8, B=2), dict(ndim=8, B=16), dict(ndim=11, B=1),
        dict(ndim=11, B=3), dict(ndim=32, B=2)]
COLUMNS = [dict(ncols=n) for n in (1, 63, 64, 65, 256, 257, 520)] + [dict(col0=0)]
NETWORKS = [dict(widths=w) for w in ((5,), (33, 64), (64, 64, 64), (5, 9, 17, 6, 33, 12, 7, 17))] + [dict(activations=a) for a in ('relu', 'tanh', 'identity-silu')] \
    + [dict(activations=['identity-silu', 'relu', 'tanh', 'silu'], widths=(9, 12, 7, 17))] + [dict(yfunction=y) for y in ('log10', 'arcsinh')] \
    + [dict(yfunction='log10', ncols=257, widths=(33, 64), activations='identity-silu'), dict(yfunction='arcsinh', ndim=8, B=2, ncols=257)]
# the cases of the issue's CPU check that the ladders do not hold already
CHECKED = [dict(ndim=7, B=10), dict(ndim=8, B=17)]
MLP_SEEDS = {'ndim=8-B=1': 3, 'ndim=32-B=2': 17}
TAYLOR_SEEDS = {'ndim=8-B=1': 1}


def _seeded(cases, seeds):
    return [dict(case, seed=seeds[case_id(case)]) if case_id(case) in seeds else case for case in cases]


def mlp_cases():
    return _seeded([dict()] + ROWS + COLUMNS + NETWORKS + CHECKED, MLP_SEEDS)


def taylor_cases():
    return _seeded([dict()] + ROWS + COLUMNS + [dict(order=o) for o in (1, 2)] + [dict(T=T) for T in (1, 31, 32, 33, 70)], TAYLOR_SEEDS)
