"""What the device tests of the MLP emulator share (tests/test_mlp_gpu.py, tests/test_mlp_train_edges_gpu.py): synthetic networks with all-distinct weights
and one guarded call of ``cp_mlp_loss_grad``."""
import ctypes

import numpy as np

import mlp_reference as mr

SENTINEL = -7.25
WORK_PAD = 64      # doubles after the workspace the library asks for


def draw_network(rng, dims):
    """Packed weights as tests/test_mlp_edges_gpu.py ``config`` draws them: kernels N(0, 1 / n_in), biases N(0, 0.3^2), alpha and beta in (0.3, 1.2), all distinct."""
    packed = np.zeros(mr.nparams(dims))
    for name, sl in mr.blocks(dims).items():
        l = int(name[-1])
        packed[sl] = rng.uniform(0.3, 1.2, 2) if name.startswith('alphabeta') else rng.normal(0., 1. / np.sqrt(dims[l]) if name.startswith('kernel') else 0.3, sl.stop - sl.start)
    assert np.unique(packed).size == packed.size
    return packed


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view('u8'), np.ascontiguousarray(b).view('u8'))


def device_loss_grad(packed, dims, activations, X, Y, with_grad=True):
    """(loss, gradient) of one call of ``cp_mlp_loss_grad``.  The workspace is filled with NaN (a read of a slot nobody wrote shows in the result), is followed
    by WORK_PAD doubles holding a sentinel and is announced with exactly ``cp_mlp_workspace_doubles``; the gradient buffer has one sentinel after it.  Asserted
    here: both sentinels intact, and the device copies of X, Y and the parameters bit for bit what was uploaded."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    L = len(dims) - 2
    widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in activations])
    host = [np.ascontiguousarray(a, dtype='f8') for a in (X, Y, packed)]
    Xd, Yd, pd = (torch.as_tensor(a, device=device) for a in host)
    need = int(lib.cp_mlp_workspace_doubles(len(X), dims[0], L, widths, dims[-1]))
    assert need > 0
    work = torch.full((need + WORK_PAD,), np.nan, dtype=torch.float64, device=device)
    work[need:] = SENTINEL
    loss = torch.full((1,), np.nan, dtype=torch.float64, device=device)
    grad = torch.full((pd.numel() + 1,), SENTINEL, dtype=torch.float64, device=device)
    _lib.check(lib.cp_mlp_loss_grad(Xd.data_ptr(), Yd.data_ptr(), len(X), dims[0], L, widths, acts, dims[-1], pd.data_ptr(), work.data_ptr(), need,
                                    loss.data_ptr(), grad.data_ptr() if with_grad else None, 0, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    grad = grad.cpu().numpy()
    assert grad[-1] == SENTINEL      # nothing past the packed layout
    assert (work[need:].cpu().numpy() == SENTINEL).all()      # nothing past the workspace
    for name, before, after in zip(('X', 'Y', 'parameters'), host, (Xd, Yd, pd)):
        assert same_bits(before, after.cpu().numpy()), name      # the inputs are read only
    return float(loss.item()), grad[:-1]
