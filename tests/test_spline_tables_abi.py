"""CPU: the argument checks of cp_spline_tables_build / cp_spline_tables_apply(_f32) come before any device call (this test runs without a device) and
name their entry point; nothing to do is CP_OK."""
import ctypes

import pytest

from cosmoprimo_amd import _lib

P = ctypes.c_void_p(64)      # a non-null pointer that is never dereferenced


def build(xk=P, y=P, nrows=4, n=16, order=3, coef=P, ok=P):
    return _lib.load().cp_spline_tables_build(xk, y, nrows, n, order, coef, ok, 0, None)


def apply(name, xk=P, coef=P, ok=P, nrows=4, n=16, xq=P, per_row=0, nq=8, out=P, flag=P, outside=None):
    return getattr(_lib.load(), name)(xk, coef, ok, nrows, n, xq, per_row, nq, out, flag, outside, 0, None)


def refused(status, name):
    assert status == _lib.CP_EINVAL, status
    assert _lib.load().cp_last_error().decode().startswith(name + ':'), _lib.load().cp_last_error()
    with pytest.raises(ValueError):
        _lib.check(status)


def test_build_refuses_bad_arguments():
    name = 'cp_spline_tables_build'
    for bad in (dict(xk=None), dict(y=None), dict(coef=None), dict(ok=None), dict(n=1), dict(n=0), dict(n=-3), dict(order=2), dict(order=0), dict(order=4),
                dict(nrows=-1)):
        refused(build(**bad), name)
    assert build(nrows=0) == _lib.CP_OK and build(nrows=0, xk=None, y=None, coef=None, ok=None) == _lib.CP_OK
    assert build(n=4097) == _lib.CP_EUNSUPPORTED and b'cp_spline_tables_build' in _lib.load().cp_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(build(n=1 << 20))


@pytest.mark.parametrize('name', ['cp_spline_tables_apply', 'cp_spline_tables_apply_f32'])
def test_apply_refuses_bad_arguments(name):
    outside = ctypes.c_int(7)
    for bad in (dict(xk=None), dict(coef=None), dict(ok=None), dict(xq=None), dict(out=None), dict(n=1), dict(n=-1), dict(nrows=-1), dict(nq=-1),
                dict(flag=None, outside=ctypes.byref(outside))):
        refused(apply(name, **bad), name)
    assert apply(name, nrows=0) == _lib.CP_OK and apply(name, nq=0) == _lib.CP_OK
    assert apply(name, nq=0, xq=None, out=None, per_row=1, outside=ctypes.byref(outside)) == _lib.CP_OK and outside.value == 0      # nothing outside nothing
    assert apply(name, nrows=0, xk=None, coef=None, ok=None, xq=None, out=None) == _lib.CP_OK
