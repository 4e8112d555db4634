"""What the device tests of cp_mlp_gauss_newton and cp_taylor_gauss_newton share (tests/test_mlp_gauss_newton_gpu.py, tests/test_taylor_gauss_newton_gpu.py): one
guarded call of either entry point on a configuration of tests/gauss_newton_reference.py.

Every call (:func:`run`) reads per-point weights and data through row strides of ncols + 3 whose padding holds NaN (a read of it would show), or one shared
row with stride 0; writes the value through a row stride of ncols + 3 whose padding holds a sentinel; announces exactly the workspace the library asks
for, filled with NaN and followed by 64 sentinels; and has 64 sentinels behind fisher, grad and chi2.  Asserted here: every sentinel intact, the inputs
unchanged, a second call gives the same bits, fisher[b] is symmetric bit for bit, a call without data gives the same fisher bits, and the value is what
cp_*_predict_columns writes (bit for bit: either engine launches that kernel)."""
import ctypes

import numpy as np

from mlp_device import same_bits

SENTINEL = -7.25
PAD, TAIL = 3, 64


def _head(kind, cfg, torch, device):
    """(the arguments of the entry points up to ncols, tensors kept alive, host copies, (B, ndim, ncols), the workspace in doubles)"""
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    col0, stop = cfg['columns']
    ncols = stop - col0
    B, ndim = cfg['X'].shape
    if kind == 'mlp':
        dims = cfg['dims']
        L, M = len(dims) - 2, dims[-1]
        widths, acts = (ctypes.c_int * L)(*dims[1:-1]), (ctypes.c_int * L)(*[_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']])
        host = {name: np.ascontiguousarray(cfg[name], dtype='f8') for name in ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale')}
        t = {name: torch.as_tensor(a, device=device) for name, a in host.items()}
        head = (t['X'].data_ptr(), B, ndim, L, widths, acts, M) + tuple(t[name].data_ptr() for name in ('packed', 'xoffset', 'xscale', 'yoffset', 'yscale')) \
            + (_lib.MLP_YFUNCTIONS[cfg['yfunction'] or None], col0, ncols)
        need = int(lib.cp_mlp_gauss_newton_workspace_doubles(B, ndim, L, widths, M, ncols))
    else:
        T, M = cfg['derivatives'].shape
        host = {name: np.ascontiguousarray(cfg[name], dtype='f8') for name in ('X', 'center', 'derivatives')}
        host['powers'] = np.ascontiguousarray(cfg['powers'], dtype='i4')
        t = {name: torch.as_tensor(a, device=device) for name, a in host.items()}
        head = (t['X'].data_ptr(), B, t['center'].data_ptr(), t['powers'].data_ptr(), ndim, T, int(host['powers'].max(initial=0)), t['derivatives'].data_ptr(), M, col0, ncols)
        need = int(lib.cp_taylor_gauss_newton_workspace_doubles(B, ndim, T, M, ncols))
    assert need > 0
    return head, t, host, (B, ndim, ncols), need


def _rows(a, B, ncols, torch, device):
    """(tensor, ld) of weights or data: one shared row (ld = 0), or rows ncols + PAD apart with NaN between them"""
    a = np.asarray(a, dtype='f8')
    if a.ndim == 1:
        return torch.as_tensor(np.ascontiguousarray(a), device=device), 0
    padded = np.full((B, ncols + PAD), np.nan)
    padded[:, :ncols] = a
    return torch.as_tensor(padded, device=device), ncols + PAD


def predict_columns(kind, cfg):
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    device = torch.device('cuda', 0)
    head, t, host, (B, ndim, ncols), need = _head(kind, cfg, torch, device)
    want = torch.empty((B, ncols), dtype=torch.float64, device=device)
    entry = _lib.load().cp_mlp_predict_columns if kind == 'mlp' else _lib.load().cp_taylor_predict_columns
    _lib.check(entry(*head, want.data_ptr(), ncols, 0, dv.stream_of(device)))
    return want.cpu().numpy()


def call(kind, cfg, with_data=True, with_value=True):
    """One call: (fisher (B, n, n), grad (B, n) or None, chi2 (B,) or None, value (B, ncols) or None), sentinels and inputs checked."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    head, t, host, (B, ndim, ncols), need = _head(kind, cfg, torch, device)
    weights, ldw = _rows(cfg['weights'], B, ncols, torch, device)
    data, ldd = _rows(cfg['data'], B, ncols, torch, device) if with_data else (None, 0)
    before = [weights.cpu().numpy()] + ([data.cpu().numpy()] if with_data else [])
    ldv = ncols + PAD
    full = lambda n: torch.full((n + TAIL,), SENTINEL, dtype=torch.float64, device=device)      # noqa: E731
    value, fisher, grad, chi2 = full(B * ldv), full(B * ndim * ndim), full(B * ndim), full(B)
    work = torch.full((need + TAIL,), np.nan, dtype=torch.float64, device=device)
    work[need:] = SENTINEL
    entry = lib.cp_mlp_gauss_newton if kind == 'mlp' else lib.cp_taylor_gauss_newton
    _lib.check(entry(*head, weights.data_ptr(), ldw, data.data_ptr() if with_data else None, ldd, value.data_ptr() if with_value else None, ldv, fisher.data_ptr(),
                     grad.data_ptr() if with_data else None, chi2.data_ptr() if with_data else None, work.data_ptr(), need, 0, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    value, fisher, grad, chi2, tail = value.cpu().numpy(), fisher.cpu().numpy(), grad.cpu().numpy(), chi2.cpu().numpy(), work[need:].cpu().numpy()
    assert (tail == SENTINEL).all(), 'written past the workspace'
    for name, a, n in (('value', value, B * ldv), ('fisher', fisher, B * ndim * ndim), ('grad', grad, B * ndim), ('chi2', chi2, B)):
        assert (a[n:] == SENTINEL).all(), 'written past the end of ' + name
    value = value[:B * ldv].reshape(B, ldv)
    assert (value[:, ncols:] == SENTINEL).all(), 'padding of the value overwritten'
    if not with_value:
        assert (value == SENTINEL).all()
    if not with_data:
        assert (grad == SENTINEL).all() and (chi2 == SENTINEL).all()
    for name, a in host.items():
        assert np.array_equal(a.view('u1'), t[name].cpu().numpy().view('u1')), name      # the inputs are read only, bit for bit
    after = [weights.cpu().numpy()] + ([data.cpu().numpy()] if with_data else [])
    assert all(same_bits(a, b) for a, b in zip(before, after))
    return (fisher[:B * ndim * ndim].reshape(B, ndim, ndim), grad[:B * ndim].reshape(B, ndim) if with_data else None, chi2[:B] if with_data else None,
            value[:, :ncols].copy() if with_value else None)


def run(kind, cfg):
    """(fisher, grad, chi2, value) of the full call, with everything the module docstring says asserted."""
    first, second = call(kind, cfg), call(kind, cfg)
    assert all(same_bits(a, b) for a, b in zip(first, second)), 'two calls differ'
    fisher = first[0]
    assert same_bits(fisher, np.ascontiguousarray(fisher.transpose(0, 2, 1))), 'fisher is not symmetric bit for bit'
    assert same_bits(call(kind, cfg, with_data=False, with_value=False)[0], fisher), 'fisher without data differs'
    assert same_bits(call(kind, cfg, with_value=False)[1], first[1]), 'grad without the value differs'
    assert same_bits(first[3], predict_columns(kind, cfg)), 'value is not predict_columns'
    return first
