"""Truth and cases of the Fisher matrices and Gauss-Newton normal equations under a dense precision matrix (cp_gauss_newton_dense) for the tests
(tests/test_gauss_newton_dense_host.py, test_gauss_newton_dense_gpu.py, test_emulator_dense_precision_gpu.py).  Per point b, with J_b (ndim, N),
r_b = data_b - value_b, A_b = [J_b ; r_b] and P (N, N) symmetric, shared by all points:

    G_b = A_b P A_b^T,  fisher[b] = G_b[:ndim, :ndim],  grad[b] = G_b[:ndim, ndim],  chi2[b] = G_b[ndim, ndim]

in any floating-point type (:func:`contract`); a column c with P[c, c] exactly 0 is dropped, whatever the operands hold there: its column of A is selected
to 0, and so are row and column c of P.  ``np.longdouble`` is the truth, float64 the yardstick that is not the code under test.

Tolerance: the rule of tests/jacobian_reference.py as tests/gauss_newton_reference.py uses it (``worst_level``, ``assert_within``: a block is one (i, j) entry of
fisher, one i of grad, or chi2, over the batch; its level is the restatement's distance from the truth, floored at FLOOR = 1.1e-16; the device gets
ALLOW = 16 levels).  A case whose level exceeds CAP = 32 floors is not used: tests/test_gauss_newton_dense_host.py holds every case listed here to that, and a
case above it has its inputs redrawn (``seed``), never the cap moved.

Operands (:func:`draw`): the kernel does not know the engine, so they are drawn directly, and so that the dense products do not cancel -- every entry of A P
A^T is a sum of terms of one sign but for the residual's: J ~ U(0.5, 1.5), value ~ U(1, 2), data = value (1 + 0.05 xi), xi standard normal,
P[c, d] = 0.6^|c - d| sqrt(w_c w_d) with w = 10^U(-2, 1): positive definite, every entry positive, three decades."""
import numpy as np

import gauss_newton_reference as gr
import jacobian_reference as jr

LD = jr.LD
CAP = 32.


def contract(J, value, precision, data, dtype):
    """(fisher (B, n, n), grad (B, n), chi2 (B,)) in ``dtype`` from J (B, n, N), value (B, N), precision (N, N) and data (N,) or (B, N); columns whose
    diagonal entry of the precision is exactly 0 dropped.  ``data`` None: (fisher, None, None)."""
    J, P = np.asarray(J).astype(dtype), np.asarray(precision).astype(dtype)
    B, n, N = J.shape
    keep = np.diagonal(P) != 0
    P = np.where(keep[:, None] & keep[None, :], P, 0)
    if data is None:
        resid = np.zeros((B, 1, N), dtype=dtype)
    else:
        resid = (np.broadcast_to(np.asarray(data).astype(dtype), (B, N)) - np.asarray(value).astype(dtype))[:, None, :]
    A = np.where(keep, np.concatenate([J, resid], axis=1), 0)
    G = np.matmul(np.matmul(A, P), A.transpose(0, 2, 1))
    if data is None:
        return G[:, :n, :n], None, None
    return G[:, :n, :n], G[:, :n, n], G[:, n, n]


def draw(B, ndim, ncols, seed=0, shared_data=False):
    """The operands of a case: dict of J (B, ndim, ncols), value (B, ncols), data (B, ncols) or (ncols,), precision (ncols, ncols), float64."""
    rng = np.random.default_rng(1000000 * seed + 10000 * B + 100 * ndim + ncols)
    J, value = rng.uniform(0.5, 1.5, (B, ndim, ncols)), rng.uniform(1., 2., (B, ncols))
    around = value[0] if shared_data else value
    data = around * (1. + 0.05 * rng.standard_normal(around.shape))
    w = 10.**rng.uniform(-2., 1., ncols)
    c = np.arange(ncols)
    precision = 0.6**np.abs(c[:, None] - c[None, :]) * np.sqrt(w[:, None] * w[None, :])
    return dict(J=J, value=value, data=data, precision=precision)


def truth(ops, with_data=True):
    """((fisher, grad, chi2) in longdouble, the same in float64)"""
    data = ops['data'] if with_data else None
    return contract(ops['J'], ops['value'], ops['precision'], data, LD), contract(ops['J'], ops['value'], ops['precision'], data, 'f8')


def worst_level(ops):
    return gr.worst_level(*truth(ops))


assert_within = gr.assert_within


def case_id(case):
    return 'B=%d-ndim=%d-ncols=%d' % case[:3] + ('-seed=%d' % case[3] if len(case) > 3 and case[3] else '')


# (B, ndim, ncols[, seed]).  The kernel's rows: a row tile holds floor(64 / (ndim + 1)) whole points (32, 16, 8, 4, 3, 2, 1 points at ndim = 1, 3, 7, 15,
# 20, 31, 32): one tile, one tile plus one point, three tiles.  Its columns: the MFMA step of 4, the half slab of 8 and the accumulator tile of 16, the wave's
# 64, the workgroup's 256 with up to three column tiles; the K loop's chunk of 32 lies among them.
BASE = (9, 7, 17)
ROW_TILES = [(B, ndim, 17) for ndim, B in ((1, 32), (1, 33), (3, 16), (3, 17), (7, 8), (7, 9), (7, 17), (15, 4), (15, 5), (20, 3), (20, 4), (31, 2), (31, 3), (32, 1), (32, 2),
                                          (32, 3))]
COLUMNS = [(9, 7, n) for n in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 520)]
# the tiles of the diagonal path (P = floor(64 / ndim) points), which a user may move from
DIAGONAL_TILES = [(B, ndim, 17) for B, ndim in ((1, 1), (64, 1), (65, 1), (21, 3), (22, 3), (10, 7), (19, 7), (17, 8), (2, 32), (3, 32), (12, 5), (13, 5), (4, 15), (5, 15), (4, 16))]
SEEDS = {}      # case -> the seed of its redraw, where the first draw lay above the cap


def _seeded(cases):
    return [case + (SEEDS[case],) if case in SEEDS else case for case in cases]


ROW_TILES, COLUMNS, DIAGONAL_TILES = _seeded(ROW_TILES), _seeded(COLUMNS), _seeded(DIAGONAL_TILES)
CASES = list(dict.fromkeys([BASE] + ROW_TILES + COLUMNS + DIAGONAL_TILES))
