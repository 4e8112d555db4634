"""GPU: the results of the forward-mode derivative entry points of both emulator engines -- cp_mlp_jacobian, cp_mlp_jvp, cp_mlp_gauss_newton and their
cp_taylor_* counterparts -- bit for bit, against tests/golden/derivative_kernel_bits.npz: what the library gave while the jvp and the Gauss-Newton kernels
were still copies of the tangent kernel and of the Taylor GEMM (recorded on an MI355X by tools/gen_derivative_kernel_bits.py, every call run twice there
and refused if its two runs differed).  The kernels use no atomics and sum in a fixed order, and a change of their source that keeps their instructions
keeps every output, so every output must be EQUAL: a tolerance would not see a row wired to the wrong point, or the seed of one variant in another.

The inputs come from seeded numpy (tests/jvp_reference.py and below), so the file holds outputs only: one flat float64 array per test and the names and
shapes of the entries in it.  The shapes are the smallest that cross every edge the kernels steer by their variant:
  common: ndim = 5 (64 is no multiple of it: a point's rows lie in two row tiles, a Gauss-Newton tile holds 12 points and 4 idle rows); M = 260 and the
    column range (250, 260), which crosses the edge of the 256-column tile; every result goes into rows 3 doubles longer than the range, padding checked
    (the ``run`` of the jacobian and jvp tests, ``call`` of tests/gauss_newton_device.py);
  jacobian and jvp: B = 22 points, ndim = 5 parameters or K = 3 general directions: 110 or 66 rows, two row tiles;
  Gauss-Newton: B = 13 (two tiles, one point in the second), two calls: weights per point with data and the value returned; one shared weight row
    (ldw = 0) without data and with a null d_value;
  MLP: last hidden widths 17 (the masked last MFMA step), 33 and 64 (72 KB of LDS: above 64 KB, every kernel symbol must have been allowed it) with the
    y functions none, log10, arcsinh: every instantiation of every variant;
  Taylor: all 56 terms of order 3 in 5 parameters: two chunks of 32 terms, the second partial, powers 1, 2 and 3 present."""
import os

import numpy as np
import pytest

import gauss_newton_device as gd
import jvp_reference as pr
import test_mlp_jacobian_gpu as mlp_jacobian
import test_mlp_jvp_gpu as mlp_jvp
import test_taylor_jacobian_gpu as taylor_jacobian
import test_taylor_jvp_gpu as taylor_jvp
from test_emulator_front_bits_gpu import assert_equal_bits

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'derivative_kernel_bits.npz')
NDIM, M, RANGE = 5, 260, (250, 260)
B, K, B_GN = 22, 3, 13
MLP_CASES = [(17, ''), (33, 'log10'), (64, 'arcsinh')]      # last hidden width, y function


def _gauss_newton_entries(kind, cfg, seed):
    """The two calls of the module docstring on ``cfg`` (B_GN points), weights and data drawn here."""
    rng = np.random.default_rng(seed)
    ncols = RANGE[1] - RANGE[0]
    cfg = dict(cfg, columns=RANGE, weights=10.**rng.uniform(-2., 1., (B_GN, ncols)), data=rng.normal(0., 1., (B_GN, ncols)))
    out = {}
    out['gn.fisher'], out['gn.grad'], out['gn.chi2'], out['gn.value'] = gd.call(kind, cfg)
    shared = dict(cfg, weights=10.**rng.uniform(-2., 1., ncols))
    out['gn_shared.fisher'] = gd.call(kind, shared, with_data=False, with_value=False)[0]
    return out


def mlp_entries(H, yfunction):
    cfg = pr.mlp_config(B=B, ndim=NDIM, K=K, widths=(9, H), M=M, activations=['tanh', 'silu'], yfunction=yfunction, seed=H)
    out = {}
    out['jacobian.value'], out['jacobian'] = mlp_jacobian.run(cfg, RANGE)
    out['jvp.value'], out['jvp'] = mlp_jvp.run(cfg, RANGE)
    small = pr.mlp_config(B=B_GN, ndim=NDIM, K=1, widths=(9, H), M=M, activations=['identity-silu', 'relu'], yfunction=yfunction, seed=H)
    out.update(_gauss_newton_entries('mlp', small, H))
    return out


def taylor_config(points, seed):
    rng = np.random.default_rng(seed)
    powers = np.array([p for p in np.ndindex(*(4,) * NDIM) if sum(p) <= 3], dtype='i4')      # all 56 terms of order 3
    assert powers.shape == (56, NDIM)
    return dict(center=rng.uniform(-0.5, 0.5, NDIM), powers=powers, derivatives=rng.normal(0., 1., (len(powers), M)), X=rng.uniform(-1., 1., (points, NDIM)),
                tan=rng.normal(0., 1., (points, K, NDIM)))


def taylor_entries():
    cfg = taylor_config(B, 560)
    out = {'jacobian': taylor_jacobian.run(cfg, RANGE), 'jvp': taylor_jvp.run(cfg, RANGE)}
    out.update(_gauss_newton_entries('taylor', taylor_config(B_GN, 561), 562))
    return out


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize('H,yfunction', MLP_CASES)
def test_mlp(recorded, H, yfunction):
    assert_equal_bits(mlp_entries(H, yfunction), recorded, 'mlp%d' % H)


def test_taylor(recorded):
    assert_equal_bits(taylor_entries(), recorded, 'taylor')
