"""CPU: the argument checks of cp_kirkby2013_rows come before any device call (this box has no device), and map onto ValueError."""
import ctypes

import numpy as np
import pytest

from cosmoprimo_amd import _lib

KNOTS = np.array([49.5, 50., 82., 82.68, 149.32, 150., 190., 191.9])
WEIGHTS = np.array([0., 1., 1., 0., 0., 1., 1., 0.])
FAKE = ctypes.c_void_p(256)      # never dereferenced: every call below is refused first


def call(nrows=4, ns=1024, fit=(300, 473), xi=FAKE, out=FAKE, s=FAKE, rescale=FAKE, per=1, knots=KNOTS, weights=WEIGHTS):
    lib = _lib.load()
    return lib.cp_kirkby2013_rows(xi, out, nrows, ns, s, fit[0], fit[1], rescale, per, None if knots is None else _lib.as_double_p(knots),
                                  None if weights is None else _lib.as_double_p(weights), 0, None)


@pytest.mark.parametrize('kwargs', [dict(nrows=-1), dict(ns=0), dict(ns=-4), dict(per=0), dict(per=-2),
                                    dict(fit=(-1, 100)), dict(fit=(1000, 1025)), dict(fit=(10, 12)), dict(fit=(12, 10)),
                                    dict(knots=None), dict(weights=None), dict(knots=KNOTS[::-1].copy()), dict(knots=KNOTS - 60.),
                                    dict(knots=np.where(np.arange(8) == 3, np.nan, KNOTS)),
                                    dict(xi=None), dict(out=None), dict(s=None), dict(rescale=None)])
def test_bad_arguments(kwargs):
    with pytest.raises(ValueError):
        _lib.check(call(**kwargs))
    assert b'cp_kirkby2013_rows' in _lib.load().cp_last_error()


def test_nothing_to_do():
    assert call(nrows=0, xi=None, out=None, s=None, rescale=None) == _lib.CP_OK
