"""GPU: cp_gauss_newton_dense against the longdouble truth of tests/gauss_newton_dense_reference.py by the project's rule (a block is one (i, j) entry of
fisher, one i of grad, or chi2, over the batch; its level the float64 restatement's distance from the truth, floored at 1.1e-16; 16 levels allowed), at the
edges of the kernel's tiling (csrc/cp_gauss_newton_dense.hip, the tiling the issue suggests but for the epilogue's slab):

    rows     a row tile holds floor(64 / (ndim + 1)) whole points: one tile, one tile plus one point, three tiles at ndim = 1, 3, 7, 15, 20, 31, 32
             (``ROW_TILES``); from ndim = 14 on the launch asks for more than 64 KB of LDS (101 KB at ndim = 32), so those cases launch it there
    columns  the MFMA step of 4, the epilogue's half slab of 8 (where the suggested tiling has a slab of 16: 7, 8, 9 are added), the accumulator tile of 16, the
             K loop's chunk of 32 (31, 32, 33 are added), the wave's 64 and the workgroup's 256 with up to three column tiles (``COLUMNS``)

Every call (:func:`call`) reads the Jacobian, the value, the data and the precision through row strides of ncols + 3 whose padding holds NaN (a read of it
would show), or one shared data row with stride 0; announces exactly the workspace the library asks for, filled with NaN and followed by 64 sentinels;
and has 64 sentinels behind fisher, grad and chi2.  :func:`run` asserts of every case: the sentinels intact, a second call gives the same bits, fisher[b]
symmetric bit for bit, a call without data gives the same fisher bits.  Then: contiguous and strided operands through the Python front, masked columns,
a diagonal precision against cp_mlp_gauss_newton, no columns at all."""
import numpy as np
import pytest

import gauss_newton_dense_reference as gd
import gauss_newton_reference as gr
import jacobian_reference as jr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL, PAD, TAIL = -7.25, 3, 64


def padded(a, torch, device, pad=PAD):
    """(tensor, ld): the last axis of ``a`` widened by ``pad`` entries of NaN"""
    wide = np.full(a.shape[:-1] + (a.shape[-1] + pad,), np.nan)
    wide[..., :a.shape[-1]] = a
    return torch.as_tensor(wide, device=device), a.shape[-1] + pad


def call(ops, with_data=True, pad=PAD):
    """One call of the C entry point: (fisher (B, n, n), grad (B, n) or None, chi2 (B,) or None), sentinels and inputs checked."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    B, ndim, ncols = ops['J'].shape
    jac, ldj = padded(ops['J'], torch, device, pad)
    value, ldv = padded(ops['value'], torch, device, pad)
    precision, ldp = padded(ops['precision'], torch, device, pad)
    data, ldd = (None, 0) if not with_data else (torch.as_tensor(ops['data'], device=device), 0) if ops['data'].ndim == 1 else padded(ops['data'], torch, device, pad)
    inputs = [t for t in (jac, value, precision, data) if t is not None]
    before = [t.cpu().numpy() for t in inputs]
    need = int(lib.cp_gauss_newton_dense_workspace_doubles(B, ndim, ncols))
    assert need >= ncols
    full = lambda n: torch.full((n + TAIL,), SENTINEL, dtype=torch.float64, device=device)      # noqa: E731
    fisher, grad, chi2 = full(B * ndim * ndim), full(B * ndim), full(B)
    work = torch.full((need + TAIL,), np.nan, dtype=torch.float64, device=device)
    work[need:] = SENTINEL
    _lib.check(lib.cp_gauss_newton_dense(jac.data_ptr(), ldj, B, ndim, ncols, value.data_ptr(), ldv, data.data_ptr() if with_data else None, ldd, precision.data_ptr(), ldp,
                                         fisher.data_ptr(), grad.data_ptr() if with_data else None, chi2.data_ptr() if with_data else None, work.data_ptr(), need, 0,
                                         dv.stream_of(device)))
    torch.cuda.synchronize(device)
    fisher, grad, chi2, tail = fisher.cpu().numpy(), grad.cpu().numpy(), chi2.cpu().numpy(), work[need:].cpu().numpy()
    assert (tail == SENTINEL).all(), 'written past the workspace'
    for name, a, n in (('fisher', fisher, B * ndim * ndim), ('grad', grad, B * ndim), ('chi2', chi2, B)):
        assert (a[n:] == SENTINEL).all(), 'written past the end of ' + name
    if not with_data:
        assert (grad == SENTINEL).all() and (chi2 == SENTINEL).all()
    assert all(same_bits(a, t.cpu().numpy()) for a, t in zip(before, inputs)), 'an input was written'
    return fisher[:B * ndim * ndim].reshape(B, ndim, ndim), grad[:B * ndim].reshape(B, ndim) if with_data else None, chi2[:B] if with_data else None


def run(ops):
    """(fisher, grad, chi2) of the full call, with everything the module docstring says asserted."""
    first, second = call(ops), call(ops)
    assert all(same_bits(a, b) for a, b in zip(first, second)), 'two calls differ'
    fisher = first[0]
    assert same_bits(fisher, np.ascontiguousarray(fisher.transpose(0, 2, 1))), 'fisher is not symmetric bit for bit'
    assert same_bits(call(ops, with_data=False)[0], fisher), 'fisher without data differs'
    return first


@pytest.mark.parametrize('case', list(dict.fromkeys(gd.ROW_TILES + gd.COLUMNS)), ids=gd.case_id)
def test_against_truth_at_the_tile_edges(case):
    ops = gd.draw(*case)
    gd.assert_within(run(ops), *gd.truth(ops), what=gd.case_id(case))


@pytest.mark.parametrize('case', [(9, 7, 17), (5, 15, 257)], ids=gd.case_id)
def test_shared_data_row(case):
    ops = gd.draw(*case, shared_data=True)
    assert ops['data'].ndim == 1
    device = run(ops)
    gd.assert_within(device, *gd.truth(ops), what='shared data row')
    assert all(same_bits(a, b) for a, b in zip(device, call(dict(ops, data=np.tile(ops['data'], (case[0], 1))))))      # the same numbers, row by row


def test_python_front_strides_and_uploads():
    """gauss_newton_dense on host arrays, on contiguous device tensors and on views with rows of other strides (taken as they are: the padding holds NaN):
    the bits of the C call"""
    import torch
    from cosmoprimo_amd.emulators.tools import gauss_newton_dense
    ops = gd.draw(9, 7, 65)
    want = call(ops)
    B, ndim, ncols = ops['J'].shape
    names = ('J', 'value', 'precision', 'data')
    host = gauss_newton_dense(*[ops[name] for name in names])
    contiguous = gauss_newton_dense(*[torch.as_tensor(ops[name], device='cuda:0') for name in names])
    wide = [padded(ops[name], torch, 'cuda:0', pad=5)[0] for name in names]
    views = [t[..., :ncols] for t in wide]
    assert all(not v.is_contiguous() for v in views)
    strided = gauss_newton_dense(*views)
    for got in (host, contiguous, strided):
        assert all(torch.is_tensor(t) and t.is_cuda for t in got) and tuple(got[0].shape) == (B, ndim, ndim) and tuple(got[1].shape) == (B, ndim) and tuple(got[2].shape) == (B,)
        assert all(same_bits(t.cpu().numpy(), w) for t, w in zip(got, want))
    only = gauss_newton_dense(views[0], None, views[2])
    assert torch.is_tensor(only) and same_bits(only.cpu().numpy(), want[0])
    shared = gauss_newton_dense(ops['J'], ops['value'], ops['precision'], ops['data'][0])
    assert same_bits(shared[0].cpu().numpy(), want[0]) and same_bits(shared[2][:1].cpu().numpy(), want[2][:1])
    with pytest.raises(ValueError):
        gauss_newton_dense(ops['J'], ops['value'], ops['precision'][:-1], ops['data'])
    with pytest.raises(ValueError):
        gauss_newton_dense(ops['J'], ops['value'][:, :-1], ops['precision'], ops['data'])
    with pytest.raises(ValueError):
        gauss_newton_dense(ops['J'][0], ops['value'], ops['precision'], ops['data'])
    with pytest.raises(NotImplementedError):
        gauss_newton_dense(np.ones((2, 33, 4)), np.ones((2, 4)), np.eye(4))


@pytest.mark.parametrize('case', [(9, 7, 65), (3, 32, 17), (17, 3, 270)], ids=gd.case_id)
def test_masked_columns(case):
    """Columns with a zero on the diagonal of the precision -- the diagonal alone, or the whole row and column -- hold NaN, Inf and 1e300 in the Jacobian, the
    value and the data.  The sums run over tiles of columns in place, so the bits are not those of the call with the columns removed (its tiles hold other
    columns): the masked call agrees with the truth of the removed operands by the rule, and is finite."""
    ops = gd.draw(*case)
    B, ndim, ncols = case
    gone = np.unique(np.array([0, 3, 8, 15, 16, 31, 32, 63, 64, 255, 256, ncols - 1]) % ncols)
    gone = gone[:max(1, min(len(gone), ncols - 4))]
    kept = np.setdiff1d(np.arange(ncols), gone)
    masked = {name: ops[name].copy() for name in ops}
    masked['precision'][gone, gone] = 0.
    whole = gone[::2]      # every other one: its row and column as well
    masked['precision'][whole, :] = masked['precision'][:, whole] = 0.
    poison = np.array([np.nan, np.inf, -np.inf, 1e300])
    masked['J'][:, :, gone] = poison[np.arange(len(gone)) % 4]
    masked['value'][:, gone] = poison[(np.arange(len(gone)) + 1) % 4]
    masked['data'][:, gone] = poison[(np.arange(len(gone)) + 2) % 4]
    removed = dict(J=ops['J'][:, :, kept], value=ops['value'][:, kept], data=ops['data'][:, kept], precision=ops['precision'][np.ix_(kept, kept)])
    device = run(masked)
    assert all(np.isfinite(a).all() for a in device)
    truth, restated = gd.truth(removed)
    gd.assert_within(device, truth, restated, what='masked columns')
    gd.assert_within(run(removed), truth, restated, what='the same columns removed')
    # a precision that masks everything: zeros
    nothing = run(dict(masked, precision=np.zeros((ncols, ncols))))
    assert all(not a.any() for a in nothing)


def test_diagonal_precision_against_cp_mlp_gauss_newton():
    """P = diag(w) on the Jacobian and the value that cp_mlp_jacobian writes, against cp_mlp_gauss_newton on the same network (a case of
    tests/gauss_newton_reference.py, weights shared by all points, some of them exactly 0): both within the rule of the truth, and of each other (other
    summation orders: bit equality is not expected)."""
    import torch
    import gauss_newton_device as gnd
    from cosmoprimo_amd import _device as dv, _lib
    from cosmoprimo_amd.emulators.tools import gauss_newton_dense
    cfg = gr.mlp_config(B=19, ndim=7, ncols=65, shared_weights=True)
    gr.mlp_truth(cfg)      # draws the operands
    cfg['weights'][::6] = 0.
    truth, restated, _ = gr.mlp_truth(cfg)
    assert gr.worst_level(truth, restated) <= gd.CAP
    diagonal = gnd.call('mlp', cfg)[:3]
    device = torch.device('cuda', 0)
    head, keep, host, (B, ndim, ncols), need = gnd._head('mlp', cfg, torch, device)
    value, jac = torch.empty((B, ncols), dtype=torch.float64, device=device), torch.empty((B, ndim, ncols), dtype=torch.float64, device=device)
    _lib.check(_lib.load().cp_mlp_jacobian(*head, value.data_ptr(), ncols, jac.data_ptr(), ncols, 0, dv.stream_of(device)))
    dense = tuple(t.cpu().numpy() for t in gauss_newton_dense(jac, value, np.diag(cfg['weights']), cfg['data']))
    gr.assert_within(dense, truth, restated, 'dense with a diagonal precision')
    gr.assert_within(diagonal, truth, restated, 'cp_mlp_gauss_newton')
    for name, a, b, t, r in zip(('fisher', 'grad', 'chi2'), gr.blocks(dense), gr.blocks(diagonal), gr.blocks(truth), gr.blocks(restated)):
        top, level = jr.levels(t, r)
        assert (np.abs(a - b).max(axis=0) <= jr.ALLOW * level * top).all(), name


def test_no_columns_gives_zeros():
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    from cosmoprimo_amd.emulators.tools import gauss_newton_dense
    lib, device = _lib.load(), torch.device('cuda', 0)
    B, ndim = 5, 3
    fisher, grad, chi2 = (torch.full((n,), SENTINEL, dtype=torch.float64, device=device) for n in (B * ndim * ndim + 8, B * ndim + 8, B + 8))
    one = torch.zeros(1, dtype=torch.float64, device=device)
    _lib.check(lib.cp_gauss_newton_dense(None, 0, B, ndim, 0, None, 0, one.data_ptr(), 0, None, 0, fisher.data_ptr(), grad.data_ptr(), chi2.data_ptr(), None, 0, 0,
                                         dv.stream_of(device)))
    for a, n in ((fisher, B * ndim * ndim), (grad, B * ndim), (chi2, B)):
        a = a.cpu().numpy()
        assert not a[:n].any() and (a[n:] == SENTINEL).all()
    f, g, c = gauss_newton_dense(np.zeros((B, ndim, 0)), np.zeros((B, 0)), np.zeros((0, 0)), np.zeros((B, 0)))
    assert tuple(f.shape) == (B, ndim, ndim) and not f.any() and not g.any() and not c.any()
