"""CPU: the short transcendental forms of csrc/cp_math.h as g++ compiles the header, unchanged, over tests/host_emu/stub (tests/host_emu/emu_math.cpp,
-ffp-contract=off), on the structured sets of tests/math_truth.py against their ``np.longdouble`` truths, and the header's two tables against longdouble.
exp_mid, exp_tab, exp10_mid, exp10_tab, sin_bounded and log_tab are built of rint / fma / ldexp / frexp and table lookups: the emulation gives the
device's bits (tests/test_math_edges_gpu.py runs the same sets through cp_math_eval).  recip, rsqrt_pos and log_pos start from a hardware estimate the
stub replaces by the exact value rounded to 24 bits: their error is emulated, their bits are not."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import math_truth as mt

LD = mt.LD
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def emu():
    emu_dir = os.path.join(HERE, 'host_emu')
    src, out = os.path.join(emu_dir, 'emu_math.cpp'), os.path.join(emu_dir, 'libemu_math.so')
    deps = [src, os.path.join(emu_dir, 'stub', 'hip', 'hip_runtime.h'), os.path.join(os.path.dirname(HERE), 'cosmoprimo_amd', 'csrc', 'cp_math.h')]
    if not os.path.isfile(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):      # (as the other harnesses of tests/host_emu: built where build() has not left it)
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', '-I' + os.path.join(emu_dir, 'stub'), '-o', out, src])
    lib = ctypes.CDLL(out)
    lib.emu_math.restype = ctypes.c_int
    lib.emu_math.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    lib.emu_math_exp2_table.restype = ctypes.POINTER(ctypes.c_double * 64)
    lib.emu_math_log_table.restype = ctypes.POINTER(ctypes.c_double * 128)
    return lib


@pytest.fixture(scope='module')
def ev(emu):
    def evaluate(name, x):
        x = np.ascontiguousarray(x, dtype='f8')
        y = np.empty_like(x)
        assert emu.emu_math(mt.KINDS[name], x.ctypes.data, y.ctypes.data, x.size) == 0
        return y
    return evaluate


def test_unknown_kind(emu):
    assert emu.emu_math(9, None, None, 0) == 1 and emu.emu_math(-1, None, None, 0) == 1


def test_tables(emu):
    """Every entry correctly rounded: 2^(j / 64); 1 / c_j; and -log of the ROUNDED reciprocal beside it (log m = log(m inv) - log inv holds for the inv in use)."""
    exp2 = np.array(emu.emu_math_exp2_table().contents)
    logt = np.array(emu.emu_math_log_table().contents)
    off = mt.half_ulp_off(exp2, mt.exp2_table_truth())
    inv, lc = mt.log_table_truth(logt)
    off_inv, off_lc = mt.half_ulp_off(logt[0::2], inv), mt.half_ulp_off(logt[1::2], lc)
    print('tables: largest distance from the truth in ulps: exp2 %.4f, 1 / c %.4f, -log(1 / c) %.4f' % (off.max(), off_inv.max(), off_lc.max()))
    assert off.max() <= 0.5 + 2.0 ** -10 and off_inv.max() <= 0.5 + 2.0 ** -10 and off_lc.max() <= 0.5 + 2.0 ** -10
    assert exp2[0] == 1. and (np.diff(exp2) > 0).all() and (np.diff(logt[0::2]) < 0).all() and (np.diff(logt[1::2]) > 0).all()


@pytest.mark.parametrize('name', ['exp_mid', 'exp_tab', 'exp10_mid', 'exp10_tab'])
def test_exponentials(ev, name):
    mt.check_exponential(name, ev, 'emulation')


def test_logarithms(ev):
    mt.check_logarithms(ev, 'emulation')


def test_sine(ev):
    """Every |n| <= 636 000 here (1.3e7 arguments, 4 s); the device runs the thinned set."""
    mt.check_sine(ev, 'emulation', thin=False)


def test_reciprocal_root(ev):
    mt.check_reciprocal_root(ev, 'emulation')


def test_sets_lie_where_they_claim():
    """The ties are ties (the two sides of each round to different n), the subnormal sets give subnormal truths, the results beyond leave the doubles."""
    for name, step in (('exp_mid', mt.LN2), ('exp_tab', mt.LN2 / 64), ('exp10_mid', mt.LOG10_2 / 64), ('exp10_tab', mt.LOG10_2 / 64)):
        x = mt.exp_normal(name)
        n = np.rint(x.astype(LD) / step)
        assert (np.diff(n[:20000]) != 0).sum() >= 1500, name      # nine doubles per tie: every ninth step crosses one
        t = mt.TRUTH[name](x)
        assert (t >= LD(mt.DBL_MIN)).all() and (t < LD(mt.DBL_MAX)).all()
    assert (np.abs(mt.exp_normal('exp10_tab')) < 300.).all() and np.abs(mt.exp_normal('exp10_tab')).max() == np.nextafter(300., 0.)
    wraps = np.rint(mt.exp_normal('exp_tab').astype(LD) / (mt.LN2 / 64)).astype(np.int64) & 63
    assert set(np.unique(wraps)) == set(range(64))
    for name in ('exp_mid', 'exp_tab', 'exp10_mid'):
        t = mt.TRUTH[name](mt.exp_subnormal(name))
        assert (t < LD(mt.DBL_MIN)).all() and (t > 0).all() and (t < mt.TINY).any() and (t > LD(2) ** -1023).any()
    x = mt.sin_arguments()
    assert (np.abs(x) < 1e6).all() and (np.abs(mt.sin_handoff()) >= 1e6).all() and np.abs(x).max() == np.nextafter(1e6, 0.)
    lx = mt.log_arguments()
    hi = (np.frexp(lx)[0].view(np.int64) >> 46) & 63      # the piece log_tab picks
    assert set(np.unique(hi)) == set(range(64)) and lx.min() == mt.DBL_MIN and lx.max() == mt.DBL_MAX


def test_truths_against_mpmath():
    """The longdouble sine next to the multiples of pi / 2 (where its argument reduction has to hold 1e6 to 1e-19), pow(10, x) and exp on thinned sets
    against 200-bit arithmetic: below 2e-19 absolute (sine) and relative.  e^(x ln 10) in longdouble is NOT a truth: 3.7e-17 at |x| = 300."""
    mpmath = pytest.importorskip('mpmath')
    mpmath.mp.prec = 200

    def mp_of(v):      # a longdouble, exactly: its mantissa as the sum of two doubles
        m, e = np.frexp(v)
        hi = np.float64(m)
        return mpmath.ldexp(mpmath.mpf(float(hi)) + mpmath.mpf(float(m - LD(hi))), int(e))

    x = mt.sin_arguments()[::211]
    err = max(abs(mp_of(t) - mpmath.sin(mpmath.mpf(float(v)))) for v, t in zip(x, mt.sin_truth(x)))
    x10 = mt.exp_normal('exp10_tab')[::1999]
    err10 = max(abs(mp_of(t) / mpmath.power(10, mpmath.mpf(float(v))) - 1) for v, t in zip(x10, mt.exp10_truth(x10)))
    naive = max(abs(mp_of(t) / mpmath.power(10, mpmath.mpf(float(v))) - 1) for v, t in zip(x10, np.exp(x10.astype(LD) * mt.LN10)))
    xe = mt.exp_normal('exp_mid')[::37]
    erre = max(abs(mp_of(t) / mpmath.exp(mpmath.mpf(float(v))) - 1) for v, t in zip(xe, mt.exp_truth(xe)))
    print('longdouble truths against 200 bits: sin %.3g, 10^x %.3g (e^(x ln 10): %.3g), exp %.3g' % (float(err), float(err10), float(naive), float(erre)))
    assert err < 2e-19 and err10 < 2e-19 and erre < 2e-19 and naive > 1e-17
