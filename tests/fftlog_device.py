"""What the truth tests of the FFTLog kernels share on the device side (tests/test_fftlog_large_truth_gpu.py, tests/test_fftlog_fused_truth_gpu.py):
a cp_fftlog_plan of the synthetic tables of tests/fftlog_taps_truth.py, driven through the C ABI, every output into a buffer full of canaries."""
import ctypes

import numpy as np
import pytest

import fftlog_taps_truth as tt

CANARY = -1.2345678912345e+77      # no transform of these rows gives this number


@pytest.fixture(scope='module')
def lib():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib
    return _lib.load()


class Plan(object):
    """A cp_fftlog_plan of the synthetic tables, destroyed on the way out."""

    def __init__(self, lib, n, syn):
        import torch
        self.lib, self.n, self.syn = lib, n, syn
        self.dev = torch.device('cuda', torch.cuda.current_device())
        self.handle = ctypes.c_void_p()

    def __enter__(self):
        from cosmoprimo_amd import _lib
        syn = self.syn
        pre, post, u = np.ascontiguousarray(syn.pre), np.ascontiguousarray(syn.post), np.ascontiguousarray(syn.u)
        assert pre.shape == post.shape == (syn.nker, syn.npad) and u.shape == (syn.nker, syn.npad // 2 + 1) and u.dtype == np.complex128
        _lib.check(self.lib.cp_fftlog_plan_create(ctypes.byref(self.handle), self.n, syn.npad, syn.nker, _lib.as_double_p(pre), _lib.as_double_p(post),
                                                  _lib.as_double_p(u.view('f8')), self.dev.index))
        return self

    def __exit__(self, *exc):
        handle, self.handle = self.handle, ctypes.c_void_p()
        self.lib.cp_fftlog_plan_destroy(handle)
        return False

    def grid(self, nbatch):
        """Workgroups cp_fftlog_plan_info reports for a batch of ``nbatch`` items."""
        from cosmoprimo_amd import _lib
        grid = ctypes.c_int()
        _lib.check(self.lib.cp_fftlog_plan_info(self.handle, nbatch, ctypes.byref(grid), None, None))
        return grid.value

    def enqueue(self, tin, tout, extrap, keep, stream, window=None):
        """cp_fftlog_execute, or cp_fftlog_execute_window for ``window`` = (out_first, out_count)."""
        from cosmoprimo_amd import _lib
        codes = tt.extrap_codes(extrap)
        if window is None:
            _lib.check(self.lib.cp_fftlog_execute(self.handle, tin.data_ptr(), tout.data_ptr(), tin.shape[0], codes[0], codes[1], codes[2], codes[3], int(keep), stream))
        else:
            _lib.check(self.lib.cp_fftlog_execute_window(self.handle, tin.data_ptr(), tout.data_ptr(), tin.shape[0], codes[0], codes[1], codes[2], codes[3], int(keep),
                                                         int(window[0]), int(window[1]), stream))

    def run(self, rows, extrap, keep, window=None):
        """rows (nbatch, nker, n) -> (nbatch, nker, m) as the device left it in a buffer full of canaries; the element behind it must still be one."""
        import torch
        nbatch, nker, n = rows.shape
        assert (nker, n) == (self.syn.nker, self.n)
        m = self.syn.npad if keep else n
        tin = torch.as_tensor(np.ascontiguousarray(rows, dtype='f8'), device=self.dev)
        tout = torch.full((nbatch * nker * m + 1,), CANARY, dtype=torch.float64, device=self.dev)
        self.enqueue(tin, tout, extrap, keep, torch.cuda.current_stream(self.dev).cuda_stream, window)
        torch.cuda.synchronize()
        out = tout.cpu().numpy()
        assert out[-1] == CANARY, 'the element behind the output was written'
        return out[:-1].reshape(nbatch, nker, m)

    def __call__(self, rows, extrap, keep):
        """rows (nbatch, nker, n) -> (nbatch, nker, m): into a buffer full of canaries with one more behind it, every element written."""
        got = self.run(rows, extrap, keep)
        assert not (got == CANARY).any(), '{:d} output elements were not written'.format(int((got == CANARY).sum()))
        return got
