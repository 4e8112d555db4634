"""CPU: ``cpur::recursions`` and ``cpur::add_carries`` (csrc/cp_uniform_recursions.h) as g++ compiles them, run for the 64 lanes of a wave by
tests/host_emu/emu_uniform_recursions.cpp -- the harness does the shift between the lanes: lane l receives the total of lane l -+ 1, the end lanes zero --
against a ``np.longdouble`` restatement of the SAME truncated sums: per knot its own segment, the segment before it (through the causal carry, over the
first NF knots of the segment only) and the segment behind it, weights p^|i - j| with the header's p.  The truncation is part of the truth, not of the
tolerance.  Sizes: S = 32 (second_derivatives_and_box_recursive), 33 and 57 with NF = S, and 57 with NF = 36, the cut of ``splice_uniform_kernel``
(NF = min(S, 36): at S = 33 that is S itself).
Inputs: seeded second differences, over h^2, of the smooth rows of tests/splice_truth.py with its relative noise of 0 .. 1e-3, 7 rows.
Tolerance: the rule of tests/spline_truth.py per row, ALLOW = 16 levels of a float64 restatement of the same sums (numpy, no fma), floored at FLOOR; that
restatement's own level is held below ``spline_truth.CAP`` x FLOOR.  A mistake must fail: the two carries handed over in the other order.  (The cut at
NF = 36 against NF = S moves a result by p^37 = 7e-22 of a neighbour's total, below the last bit of a longdouble: no tolerance tells the two apart; the
instance is run here for its bounds and pinned bit for bit by tests/test_uniform_recursion_bits_gpu.py.)"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import splice_truth as sp
import spline_truth as st

LD = st.LD
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(32, 32), (33, 33), (57, 57), (57, 36)]


@pytest.fixture(scope='module')
def emu():
    src = os.path.join(HERE, 'host_emu', 'emu_uniform_recursions.cpp')
    out = os.path.join(HERE, 'host_emu', 'libemu_uniform_recursions.so')
    dep = os.path.join(os.path.dirname(HERE), 'cosmoprimo_amd', 'csrc', 'cp_uniform_recursions.h')
    if not os.path.isfile(out) or os.path.getmtime(out) < max(os.path.getmtime(src), os.path.getmtime(dep)):      # (as the other harnesses of tests/host_emu: built where build() has not left it)
        subprocess.check_call(['g++', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', out, src])
    lib = ctypes.CDLL(out)
    lib.emu_uniform_recursions.restype = ctypes.c_int
    lib.emu_uniform_recursions.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    lib.emu_uniform_recursions_p.restype = ctypes.c_double
    return lib


def second_differences(S, seed=0):
    """(7, 64 S): (y_{i+1} - 2 y_i + y_{i-1}) / h^2 of the smooth row of splice_truth on 64 S + 2 knots, noise of EPS relative size per row."""
    n = 64 * S + 2
    rng = np.random.default_rng(1000 * S + seed)
    y = sp.smooth(sp.U0 + sp.H * np.arange(n), n) * (1. + np.array(sp.EPS)[:, None] * rng.uniform(-1., 1., (st.NBASE, n)))
    return np.ascontiguousarray((y[:, 2:] - 2. * y[:, 1:-1] + y[:, :-2]) / sp.H**2)


def restate(r, S, NF, p, dtype):
    """sum_j p^|i-j| r_j over the lane's own segment, the one behind it and -- for the first NF knots of the segment -- the one before it."""
    r = np.asarray(r).astype(dtype)
    p = dtype(p)
    rows = r.reshape(len(r), 64, S)
    t = np.arange(S)
    own = p**np.abs(t[:, None] - t[None, :]).astype(dtype)                      # [t, j]
    behind = p**(S - t[:, None] + t[None, :]).astype(dtype)                     # knot j of the next segment: S - t + j away
    before = np.where(t[:, None] < NF, p**(t[:, None] + S - t[None, :]).astype(dtype), 0)      # knot j of the previous one: t + S - j away
    out = rows @ own.T
    out[:, :-1] += rows[:, 1:] @ behind.T
    out[:, 1:] += rows[:, :-1] @ before.T
    return out.reshape(len(r), 64 * S)


def run(emu, r, S, NF, swapped=False):
    out = np.empty_like(r)
    for row, res in zip(r, out):
        assert emu.emu_uniform_recursions(S, NF, row.ctypes.data, res.ctypes.data, int(swapped)) == 0
    return out


@pytest.mark.parametrize('S,NF', CASES)
def test_recursions_and_carries(emu, S, NF):
    p = emu.emu_uniform_recursions_p()
    assert abs(LD(p) - (np.sqrt(LD(3)) - 2)) <= 2.**-55      # sqrt 3 - 2 to half a unit of a double's last place at 0.27
    r = second_differences(S)
    truth, f64 = restate(r, S, NF, p, LD), restate(r, S, NF, p, np.float64)
    top, level = st.levels(truth, f64)
    assert (level <= st.CAP * st.FLOOR).all(), level / st.FLOOR      # the float64 restatement itself
    st.assert_within(f64, truth, f64, what='float64 restatement, S = %d, NF = %d' % (S, NF))
    worst = st.assert_within(run(emu, r, S, NF), truth, f64, what='recursions + carries, S = %d, NF = %d' % (S, NF))
    assert worst <= 1.
    with pytest.raises(AssertionError):
        st.assert_within(run(emu, r, S, NF, swapped=True), truth, f64, what='the carries in the other order')


def test_sizes_that_are_not_built(emu):
    out = np.zeros(64 * 40)
    assert emu.emu_uniform_recursions(40, 40, out.ctypes.data, out.ctypes.data, 0) == 1
    assert emu.emu_uniform_recursions(33, 36, out.ctypes.data, out.ctypes.data, 0) == 1      # the carry stays inside the segment
