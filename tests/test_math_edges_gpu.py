"""The short transcendental forms of csrc/cp_math.h through cp_math_eval on the structured sets of tests/math_truth.py -- the ties of every argument
reduction, every wrap of the tables' index, the piece edges, the hand-off thresholds, subnormal results, results beyond the doubles, the doubles next to
the multiples of pi / 2 -- against ``np.longdouble``: the contracts the header states (math_truth.BOUNDS), 2 units of 2^-1074 where an exponential's
result is subnormal, and the exact answers (0, Inf, NaN, the library's values) where it promises them.  tests/test_math_gpu.py holds the same bounds on
uniform draws; tests/test_math_truth_host.py runs these sets (and the full set of the sine) through the g++ emulation of the header.  Each test prints
its worst figure."""
import numpy as np
import pytest

import math_truth as mt

pytestmark = pytest.mark.gpu


def ev(name, x):
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', 0)
    tx = torch.as_tensor(np.array(x, dtype='f8'), device=dev)
    ty = torch.full_like(tx, -7.25)
    _lib.check(_lib.load().cp_math_eval(_lib.MATH_FUNCTIONS[name], tx.data_ptr(), ty.data_ptr(), tx.numel(), 0, dv.stream_of(dev)))
    return ty.cpu().numpy()


def test_kinds_match():
    from cosmoprimo_amd import _lib
    assert _lib.MATH_FUNCTIONS == mt.KINDS


@pytest.mark.parametrize('name', ['exp_mid', 'exp_tab', 'exp10_mid', 'exp10_tab'])
def test_exponentials(name):
    mt.check_exponential(name, ev, 'device')
    if name == 'exp_tab':
        print('device exp_tab(+Inf) = %r (no promise: the reduced argument is not finite)' % float(ev('exp_tab', [np.inf])[0]))


def test_logarithms():
    mt.check_logarithms(ev, 'device')


def test_sine():
    mt.check_sine(ev, 'device')


def test_reciprocal_root():
    mt.check_reciprocal_root(ev, 'device')
