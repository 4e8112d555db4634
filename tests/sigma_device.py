"""What the device tests of the fused sigma kernels share (tests/test_sigma_tail_edges_gpu.py, tests/test_sigma_rz_edges_gpu.py): plans of synthetic tables through
the C ABI, destroyed on the way out, and the read-back that ends the session on a device error."""
import ctypes

import numpy as np
import pytest

import sigma_truth as sg

CANARY = -1.2345678912345e+77      # no result of these tests is this number
LDS_FFT = 34960      # Fftlog<2048, 16>::LDS_BYTES (tests/test_full_lds_launches_gpu.py); a workgroup has 160 KiB


def synchronized(torch, tensor):
    """The tensor on the host behind a synchronisation; an error of the device ends the session (nothing more is started on a device that has faulted)."""
    try:
        torch.cuda.synchronize()
        return tensor.cpu().numpy()
    except RuntimeError as exc:
        pytest.exit('the device reported an error: {}'.format(exc), returncode=3)


class FftPlan(object):
    """A cp_fftlog_plan of synthetic tables (n = 1024, npad = 2048, one kernel index), destroyed on the way out."""

    def __init__(self, env, syn):
        self.env, self.syn, self.handle = env, syn, ctypes.c_void_p()

    def __enter__(self):
        torch, _lib, lib, dev, stream = self.env
        pre, post, u = (np.ascontiguousarray(a) for a in (self.syn.pre, self.syn.post, self.syn.u))
        _lib.check(lib.cp_fftlog_plan_create(ctypes.byref(self.handle), sg.N, sg.NPAD, 1, _lib.as_double_p(pre), _lib.as_double_p(post), _lib.as_double_p(u.view('f8')),
                                             dev.index))
        return self

    def __exit__(self, *exc):
        handle, self.handle = self.handle, ctypes.c_void_p()
        self.env[2].cp_fftlog_plan_destroy(handle)
        return False


class GeoPlan(object):
    """A cp_geospline_plan on S_GRID: the CU solve, or -- syn given -- the prefiltered form, which owns its transform."""

    def __init__(self, env, r, syn=None):
        self.env, self.r, self.syn, self.handle = env, np.ascontiguousarray(r, dtype='f8'), syn, ctypes.c_void_p()

    def __enter__(self):
        torch, _lib, lib, dev, stream = self.env
        s, r = np.ascontiguousarray(sg.S_GRID), self.r
        if self.syn is None:
            _lib.check(lib.cp_geospline_plan_create(ctypes.byref(self.handle), _lib.as_double_p(s), s.size, _lib.as_double_p(r), r.size, dev.index))
        else:
            pre, post, u = (np.ascontiguousarray(a[0]) for a in (self.syn.pre, self.syn.post, self.syn.u))
            _lib.check(lib.cp_geospline_plan_create_prefiltered(ctypes.byref(self.handle), sg.N, sg.NPAD, _lib.as_double_p(pre), _lib.as_double_p(post),
                                                                _lib.as_double_p(u.view('f8')), _lib.as_double_p(s), _lib.as_double_p(r), r.size, dev.index))
        return self

    def __exit__(self, *exc):
        handle, self.handle = self.handle, ctypes.c_void_p()
        self.env[2].cp_geospline_plan_destroy(handle)
        return False

    def info(self):
        torch, _lib, lib, dev, stream = self.env
        first, count, nq = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.check(lib.cp_geospline_plan_info(self.handle, ctypes.byref(first), ctypes.byref(count), ctypes.byref(nq)))
        return first.value, count.value, nq.value
