"""GPU: cp_mlp_loss_grad and cp_mlp_adam (csrc/cp_mlp.hip) at the edges of their tiles, slices and phases, on synthetic weights, all distinct, one
dimension at a time from a small base (b = 65, ndim = 3, widths (5, 17), M = 257), as tests/test_mlp_edges_gpu.py does for predict.

Truth and tolerance are those of tests/test_mlp_gpu.py::test_loss_grad (tests/mlp_reference.py): the longdouble backward pass; per block of the packed
layout 16 x the float64 numpy pass's rounding level (floored at eps) x the block's largest gradient; a block whose true gradient is 0 must be exactly 0;
the loss within 16 x 2 sqrt(b M) eps.  Every call goes through tests/mlp_device.py ``device_loss_grad``: workspace filled with NaN and announced exactly,
sentinels after the workspace and after the gradient, inputs bit for bit untouched.

Which shape reaches which path (``mlp_work``'s slice rule: nsl0 = min(ceil(1024 / row tiles), ceil(M / 64)) slices wanted, each ks = ceil(M / nsl0) rounded up
to a multiple of 8, so nsl = ceil(M / ks) slices, the last one shorter):

* ``mlp_gw_out_kernel<NI>`` / ``mlp_dh_kernel<NJ>``, NI = NJ = ceil(H / 16) for the last hidden width H: H = 1, 4, 15, 16 -> <1>; 17, 32 -> <2>; 33, 47, 48 -> <3>
  (never run before, nor was <1>); 49, 63, 64 -> <4>.  H = 1 also clamps every row index of the left operand to 0.
* the 4-sample MFMA step of ``mlp_gw_out_kernel`` (``inside`` masks a[] and bb[] of samples past b): b = 1, 3, 5, 15, 17, 63, 65 (the base), 129, 193 leave 1, 3, 1, 3,
  1, 3, 1, 1, 1 valid samples in the last step; b = 4, 16, 64 none to mask.
* the 16 phases of ``mlp_gw_hidden_kernel``: b = 1, 3, 4, 5, 15 leave phases without a sample, b = 16 one each, b = 17 two in phase 0; its workgroups of 64 entries:
  first width w with (w + 1) x 17 entries: w = 1 -> 34 (one, ragged), w = 63 -> 1088 (17, full), w = 64 -> 1105 (18, the last holds 17); (ndim + 1) x 5 entries at ndim = 1, 32.
* row tiles of the training forward pass and of ``mlp_dh_kernel``: b = 1 .. 64 -> 1, 65, 129 -> 2, 3, b = 193 -> 4, b = 4033 -> 64; column tiles (``losspart`` is
  indexed [column tile][row tile]): M = 1 .. 256 -> 1, 257, 259 -> 2, 513 -> 3, 1025 -> 5.
* slices of ``mlp_dh_kernel`` at b = 65 (M: ks, nsl, length of the last slice): 1: 8, 1, 1; 3: 8, 1, 3; 63: 64, 1, 63; 64: 64, 1, 64; 65: 40, 2, 25; 255: 64, 4, 63;
  256: 64, 4, 64; 257: 56, 5, 33; 259: 56, 5, 35; 513: 64, 9, 1; 1025: 64, 17, 1.  The last MFMA step of a slice holds 1 (M = 1, 65, 257, 513, 1025) or 3 (M = 3,
  63, 255, 259) valid inner indices: the ``inside`` / ``kk`` path; slices start off a multiple of 64 at ks = 40 and 56; 1 (nsl <= 4), 2 (5), 3 (9) and 5 (17)
  y-blocks of four slices; ``mlp_dz_kernel`` sums 1 .. 17 partial products.
* the row tiles, not M, limiting the slices (ceil(1024 / nrt) < ceil(M / 64)): b = 4033, widths (5,), M = 1025: 64 row tiles, 16 < 17, ks = 72, 15 slices, the last 17 long.
* ndim = 1 and 32 (the input staging of the forward pass, a wave taking inputs i = wave mod 4; the first layer's (ndim + 1, 5) gradient).
* depth: one hidden layer (``mlp_dz_kernel`` only in its ``part`` form, X the left operand of the only hidden gradient); eight layers of widths (7, 17, 33, 4, 64, 1, 9,
  12) with every activation twice, and with eight identity-silu: ``dz[l & 1]`` ping-pong over 8 layers, ``ca`` / ``cb`` rewritten and summed 8 times, every
  ``alphabeta`` block trained.

cp_mlp_adam: against ``mlp_reference.adam`` with the tolerances of test_mlp_gpu.py::test_adam at the ends of its workgroups of 256, and its special values."""
import ctypes

import numpy as np
import pytest

import mlp_reference as mr
from mlp_device import SENTINEL, device_loss_grad, draw_network, same_bits

pytestmark = pytest.mark.gpu
BASE = dict(b=65, ndim=3, widths=(5, 17), M=257)
DEEP = (7, 17, 33, 4, 64, 1, 9, 12)


def case(b, ndim, widths, M, seed, activations=None):
    rng = np.random.default_rng(seed)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = list(activations or [mr.ACTIVATIONS[(seed + l) % 4] for l in range(len(widths))])
    packed = draw_network(rng, dims)
    X, Y = rng.uniform(0., 1., (b, ndim)), rng.uniform(0., 1., (b, M))
    return packed, dims, activations, X, Y


def check_against_truth(label, args, truth):
    """The checks of test_loss_grad on one case; the largest fraction of the allowance used by any block."""
    packed, dims, activations, X, Y = args
    levels, (loss_ld, grad_ld), _ = truth
    b, M = len(X), dims[-1]
    loss, grad = device_loss_grad(*args)
    again = device_loss_grad(*args)
    only = device_loss_grad(*args, with_grad=False)
    assert again[0] == loss and same_bits(again[1], grad)               # two calls, bit for bit
    assert only[0] == loss and (only[1] == SENTINEL).all()              # loss only: the same bits, the gradient untouched
    assert np.isfinite(grad).all()                                      # (no slot of the NaN workspace read before it was written)
    used = abs(loss - float(loss_ld)) / (16 * 2 * np.sqrt(b * M) * mr.EPS * float(loss_ld))
    print('%s: the loss uses %.3g of its allowance' % (label, used))
    assert used <= 1.
    worst = 0.
    for name, sl in mr.blocks(dims).items():
        top, level = levels[name]
        if top == 0.:
            assert not grad[sl].any(), name
            continue
        fraction = float(np.abs(grad[sl] - np.asarray(grad_ld[sl], dtype='f8')).max()) / (16 * level * top)
        print('%s, %s: level %.3g, the device uses %.3g of 16 x' % (label, name, level, fraction))
        assert fraction <= 1., name
        worst = max(worst, fraction)
    print('%s: largest fraction %.3g' % (label, worst))
    return worst


SWEEP = ([('b', v) for v in (1, 3, 4, 5, 15, 16, 17, 63, 64, 129, 193)] + [('M', v) for v in (1, 3, 63, 64, 65, 255, 256, 259, 513, 1025)]
         + [('H', v) for v in (1, 4, 15, 16, 17, 32, 33, 47, 48, 49, 63, 64)] + [('w', v) for v in (1, 63, 64)] + [('ndim', v) for v in (1, 32)])


def sweep_case(name, value):
    """The seed is the case's place in SWEEP, so that neighbouring cases start the cycle of activations at different places: each of (silu, relu), (relu, tanh),
    (tanh, identity-silu), (identity-silu, silu) comes up in every group, identity-silu both as the last hidden layer (``mlp_dz_kernel`` on partial sums)
    and before it."""
    shape = dict(BASE)
    if name == 'H':
        shape['widths'] = (5, value)
    elif name == 'w':
        shape['widths'] = (value, 17)
    else:
        shape[name] = value
    return case(seed=1000 + SWEEP.index((name, value)), **shape)


@pytest.mark.parametrize('name,value', SWEEP, ids=['%s%d' % item for item in SWEEP])
def test_loss_grad_one_dimension_at_a_time(name, value):
    """Around b = 65, ndim = 3, widths (5, 17), M = 257 (two row tiles, two column tiles, <2> of both matrix-core kernels, five slices of 56 in two y-blocks, the
    last 33 long, one valid index in its last MFMA step and one valid sample in ``mlp_gw_out_kernel``'s last step): ``b`` the MFMA step of
    ``mlp_gw_out_kernel``, the phases of ``mlp_gw_hidden_kernel`` and 1 to 4 row tiles; ``M`` the slices of ``mlp_dh_kernel`` (length, count, y-blocks, the partial
    last step) and 1 to 5 column tiles; ``H`` (the last hidden width) the four instantiations of ``mlp_gw_out_kernel<NI>`` and ``mlp_dh_kernel<NJ>`` at both ends
    of their range; ``w`` (the first hidden width) the workgroups of ``mlp_gw_hidden_kernel``; ``ndim`` 1 and 32.  The module docstring has the table."""
    args = sweep_case(name, value)
    check_against_truth('%s = %d' % (name, value), args, mr.gradient_levels(*args))


DEPTHS = [('one', (7,), None, 701), ('eight', DEEP, None, 709), ('eight-identity-silu', DEEP, ['identity-silu'] * 8, 710)]      # (seed 709: the layer of width 1 gets tanh; with relu it can die)


@pytest.mark.parametrize('label,widths,activations,seed', DEPTHS, ids=[d[0] for d in DEPTHS])
def test_loss_grad_depth(label, widths, activations, seed):
    """One hidden layer: ``mlp_dz_kernel`` runs in its ``part`` form only and the one hidden gradient reads X.  Eight, widths (7, 17, 33, 4, 64, 1, 9, 12): the
    ``dz[l & 1]`` ping-pong and the workspace's z / h offsets over eight layers, once with every activation twice (two ``alphabeta`` blocks trained, six
    cleared by ``mlp_gw_hidden_kernel``), once with eight identity-silu (every ``alphabeta`` block trained, ``ca`` / ``cb`` reused eight times).  The last width
    12 runs <1> of both matrix-core kernels, the width 1 in the middle a (b, 1) dz."""
    args = case(BASE['b'], BASE['ndim'], widths, BASE['M'], seed=seed, activations=activations)
    truth = mr.gradient_levels(*args)
    trained = [name for name, (top, level) in truth[0].items() if top > 0.]
    wanted = [name for l, a in enumerate(args[2]) for name in ('kernel%d' % l, 'bias%d' % l) + (('alphabeta%d' % l,) if a == 'identity-silu' else ())]
    assert set(wanted) <= set(trained)      # (the case is not degenerate: no layer's gradient died on the way down)
    check_against_truth(label, args, truth)


@pytest.fixture(scope='module')
def many_row_tiles():
    args = case(4033, 3, (5,), 1025, seed=4033, activations=['identity-silu'])
    return args, mr.gradient_levels(*args)


def test_loss_grad_row_tiles_limit_the_slices(many_row_tiles):
    """b = 4033, widths (5,), M = 1025: 64 row tiles and 5 column tiles (320 entries of ``losspart``); ceil(1024 / 64) = 16 slices wanted where M alone would give
    17, so ks = ceil(1025 / 16) = 65 -> 72 and 15 slices, the last 17 long (one valid index in its last step), four y-blocks the last with three waves at
    work; ``mlp_gw_out_kernel<1>`` runs 1009 steps over the batch, ``mlp_gw_hidden_kernel`` 252 or 253 samples per phase, ``mlp_sum_kernel`` 20165 entries.
    The level is the numpy pass's alone, as everywhere: the output kernel's block, where each lane group adds its 1009 samples in order and numpy's matrix
    product does not, takes 0.76 of 16 x 5.1e-16 on an MI355X, every other block under 0.02."""
    args, truth = many_row_tiles
    check_against_truth('b = 4033', args, truth)


def raw_call(b, work_short=0):
    """One call on the base network with every buffer holding a sentinel; (status, loss, gradient, workspace) afterwards."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    packed, dims, activations, X, Y = case(seed=11, **BASE)
    lib, device = _lib.load(), torch.device('cuda', 0)
    widths, acts = (ctypes.c_int * 2)(*dims[1:-1]), (ctypes.c_int * 2)(*[_lib.MLP_ACTIVATIONS[a] for a in activations])
    Xd, Yd, pd = (torch.as_tensor(a, device=device) for a in (X, Y, packed))
    need = int(lib.cp_mlp_workspace_doubles(len(X), dims[0], 2, widths, dims[-1]))
    work, loss, grad = (torch.full((n,), SENTINEL, dtype=torch.float64, device=device) for n in (need, 1, packed.size))
    status = lib.cp_mlp_loss_grad(Xd.data_ptr(), Yd.data_ptr(), b, dims[0], 2, widths, acts, dims[-1], pd.data_ptr(), work.data_ptr(), need - work_short,
                                  loss.data_ptr(), grad.data_ptr(), 0, dv.stream_of(device))
    torch.cuda.synchronize(device)
    return status, lib.cp_last_error(), tuple(t.cpu().numpy() for t in (loss, grad, work))


def test_an_empty_batch_writes_nothing():
    from cosmoprimo_amd import _lib
    status, _, buffers = raw_call(0)
    assert status == _lib.CP_OK and all((a == SENTINEL).all() for a in buffers)


def test_a_short_workspace_is_refused_before_any_launch():
    from cosmoprimo_amd import _lib
    status, message, buffers = raw_call(BASE['b'], work_short=1)
    assert status == _lib.CP_EINVAL and b'cp_mlp_loss_grad' in message and b'workspace' in message
    assert all((a == SENTINEL).all() for a in buffers)
    status, _, (loss, grad, work) = raw_call(BASE['b'])      # the same buffers at their full length: the call goes through
    assert status == _lib.CP_OK and np.isfinite(loss).all() and np.isfinite(grad).all() and not (grad == SENTINEL).any()


LR, B1, B2, ADAM_EPS = 1e-2, 0.9, 0.999, 1e-8


def device_adam(p, m, v, g, lr=LR, step=3):
    """One call on copies with a sentinel element after each of p, m, v (asserted intact, g unchanged): the new (p, m, v)."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    device, n = torch.device('cuda', 0), len(p)
    pd, md, vd = (torch.as_tensor(np.append(a, SENTINEL), device=device) for a in (p, m, v))
    gd = torch.as_tensor(np.append(g, 1e30), device=device)      # (an entry past the end that would show if it were used)
    _lib.check(_lib.load().cp_mlp_adam(pd.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), n, lr, B1, B2, ADAM_EPS, 1. - B1**step, 1. - B2**step, 0,
                                       dv.stream_of(device)))
    torch.cuda.synchronize(device)
    out = [t.cpu().numpy() for t in (pd, md, vd)]
    assert all(a[-1] == SENTINEL for a in out) and same_bits(gd.cpu().numpy(), np.append(g, 1e30))
    return [a[:-1] for a in out]


def adam_inputs(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0., 1., n), rng.normal(0., 1e-2, n), rng.uniform(0., 1e-4, n), rng.normal(0., 1e-2, n)


def assert_adam(got, p, m, v, g, lr, step):
    """The tolerances of test_adam: 4 eps of the two terms' magnitudes for m and v, 4 eps of |p| + the update for p."""
    p1, m1, v1 = mr.adam(p, m, v, g, lr, step)
    c1, c2 = 1. - B1**step, 1. - B2**step
    assert (np.abs(got[1] - m1) <= 4 * mr.EPS * (B1 * np.abs(m) + (1. - B1) * np.abs(g))).all()
    assert (np.abs(got[2] - v1) <= 4 * mr.EPS * (B2 * v + (1. - B2) * g * g)).all()
    update = lr * np.abs(m1 / c1) / (np.sqrt(v1 / c2) + ADAM_EPS)
    excess = np.abs(got[0] - p1) / (4 * mr.EPS * (np.abs(p) + update))
    print('adam, n = %d: p uses %.3g of 4 eps' % (len(p), excess.max()))
    assert (excess <= 1.).all() and np.isfinite(got[0]).all()


@pytest.mark.parametrize('n', [1, 255, 256, 257, 513])
def test_adam_at_the_ends_of_its_workgroups(n):
    """Workgroups of 256 entries: one thread at work, one short of a workgroup, exactly one, one entry in the second, one in the third."""
    p, m, v, g = adam_inputs(n, seed=n)
    assert_adam(device_adam(p, m, v, g), p, m, v, g, LR, 3)


def test_adam_without_a_learning_rate():
    p, m, v, g = adam_inputs(300, seed=21)
    got = device_adam(p, m, v, g, lr=0.)
    assert same_bits(got[0], p) and (got[1] != m).all() and (got[2] != v).all()
    assert_adam(got, p, m, v, g, 0., 3)


def test_adam_first_step():
    """Step 1 from zero moments: c1 = 1 - 0.9 = 0.1 and c2 = 1 - 0.999 = 0.001 (as float64 forms them, what ``fit`` passes), m_hat = g, v_hat = g^2 up to rounding:
    every entry moves by lr g / (|g| + 1e-8), lr against the sign of its gradient."""
    rng = np.random.default_rng(22)
    n = 300
    p, g = rng.normal(0., 1., n), rng.uniform(1e-3, 1., n) * rng.choice([-1., 1.], n)
    zero = np.zeros(n)
    got = device_adam(p, zero, zero, g, step=1)
    assert_adam(got, p, zero, zero, g, LR, 1)
    assert np.allclose(got[0] - p, -LR * np.sign(g), rtol=2e-5, atol=0.)      # (1e-8 / |g| <= 1e-5)


def test_adam_keeps_nan_and_infinity_in_their_entries():
    p, m, v, g = adam_inputs(600, seed=23)
    clean = device_adam(p, m, v, g)
    bad = g.copy()
    nans, infs = [0, 255, 256, 599], [7, 300, 511, 512]
    bad[nans], bad[infs] = np.nan, [np.inf, -np.inf, np.inf, -np.inf]
    got = device_adam(p, m, v, bad)
    others = np.ones(600, dtype=bool)
    others[nans + infs] = False
    assert all(same_bits(a[others], c[others]) for a, c in zip(got, clean))
    assert all(np.isnan(a[nans]).all() for a in got)
    assert np.array_equal(got[1][infs], bad[infs]) and (got[2][infs] == np.inf).all() and np.isnan(got[0][infs]).all()      # inf / (sqrt(inf) + eps)


def test_adam_where_the_square_of_the_gradient_leaves_the_range():
    """g^2 overflows (|g| = 1e200: v infinite, the update lr m_hat / inf = 0), underflows to 0 (1e-200) or to a subnormal (1e-160), with zero and non-zero moments:
    what numpy gives, every operation rounded once on both sides."""
    values = np.array([1e200, -1e200, 1e-200, -1e-200, 1e-160, -3e-160, 1.3e154, 1.4e154, 1.5e-162, 1e-2])
    n = 2 * len(values)
    p, m, v, _ = adam_inputs(n, seed=24)
    g = np.concatenate([values, values])
    m[:len(values)], v[:len(values)] = 0., 0.
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        want = mr.adam(p, m, v, g, LR, 3)
    got = device_adam(p, m, v, g)
    assert np.isinf(want[2]).any() and (want[2] == 0.).any() and ((want[2] > 0.) & (want[2] < 2.3e-308)).any()      # the case holds what it is named after
    for name, a, w in zip('pmv', got, want):
        assert np.array_equal(np.isnan(a), np.isnan(w)), name
        assert np.array_equal(a[~np.isnan(w)], w[~np.isnan(w)]), name
