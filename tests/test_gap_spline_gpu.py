"""GPU: ``cp_gap_spline`` (``gap_spline_kernel``, csrc/cp_spline.hip: wallish2018's removal of a box of knots -- the clamped spline through
z = y x^2 without the knots a .. b, evaluated there and divided by x^2 -- by two sweeps that start at most 64 knots from the box) against the
longdouble truth of tests/spline_truth.py, a clamped spline solved over ALL the remaining knots.
300 knots: boxes of one knot and of all but the end knots, boxes whose sweeps start exactly on the true end ((65, 70): L = 64; (100, 234):
R + 64 = n - 1) and one knot further in, on a centred difference ((66, 70), (100, 233)); 4 knots, the smallest size; boxes that are no boxes (the
identity).  Out of place and in place, 1 and 37 columns (7 base rows times powers of two: the operation is linear).  Outside the box the output
is the input bit for bit; a NaN row leaves the others bit for bit.
Tolerance: the rule of tests/spline_truth.py, 16 levels of the float64 restatement per (row, box); each test prints the largest fraction it used.
Measured on an MI355X, largest fraction of the allowance used by cp_gap_spline: 0.19 (300 knots, box (150, 150)), 0.063 at 4 knots; in place and out of
place give the same figures.  With the sweeps' start cut to 4 knots from the box in a scratch copy of the kernel every 300-knot test fails.
"""
import numpy as np
import pytest

import spline_truth as st

pytestmark = pytest.mark.gpu


def _run(y, boxes, in_place):
    """y (ncol, n) numpy, boxes (ncol, 2) -> (ncol, n)."""
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    ncol, n = y.shape
    ty = torch.as_tensor(y, device=dev)
    box = torch.as_tensor(np.ascontiguousarray(boxes, dtype='i4'), device=dev)
    out = ty if in_place else torch.full_like(ty, -7777.)
    _lib.check(lib.cp_gap_spline(ty.data_ptr(), box.data_ptr(), out.data_ptr(), ncol, n, 0, dv.stream_of(dev)))
    return out.cpu().numpy()


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
@pytest.mark.parametrize('ncol', st.GAP_COUNTS)
@pytest.mark.parametrize('n', sorted(st.GAP_BOXES))
def test_gap_spline(n, ncol, in_place):
    base = st.gap_rows(n)
    y = st.batch(base, ncol)
    worst = 0.
    for a, b in st.GAP_BOXES[n]:
        got = _run(y, np.tile([a, b], (ncol, 1)), in_place)
        inside = np.zeros(n, dtype=bool)
        inside[a:b + 1] = True
        assert np.array_equal(got[:, ~inside], y[:, ~inside])
        worst = max(worst, st.assert_within(got[:, inside], *st.gap_case(n, a, b), what='%d knots, box (%d, %d)' % (n, a, b), scaled=True))
    for a, b in st.GAP_INVALID[n]:
        assert np.array_equal(_run(y, np.tile([a, b], (ncol, 1)), in_place), y), (a, b)
    print('gap spline, %d knots, %d columns, %s: largest fraction %.3g' % (n, ncol, 'in place' if in_place else 'out of place', worst))


@pytest.mark.parametrize('in_place', [False, True], ids=['out_of_place', 'in_place'])
def test_boxes_differ_and_nan_row_stays_alone(in_place):
    """Every column its own box (valid and invalid ones side by side), then a NaN in the reach of one row's sweeps."""
    n, ncol = 300, 37
    boxes = st.GAP_BOXES[n] + st.GAP_INVALID[n]
    y = st.batch(st.gap_rows(n), ncol)
    mine = np.array([boxes[c % len(boxes)] for c in range(ncol)])
    got = _run(y, mine, in_place)
    for c in range(ncol):
        a, b = mine[c]
        assert np.array_equal(got[c], _run(y[c:c + 1], mine[c:c + 1], in_place)[0]), (c, a, b)      # the bits it has alone, which test_gap_spline holds to the truth
    bad = y.copy()
    rows = [c for c in range(ncol) if tuple(mine[c]) == (100, 233)]
    bad[rows[0], 90] = np.nan
    gotb = _run(bad, mine, in_place)
    keep = np.arange(ncol) != rows[0]
    assert np.array_equal(gotb[keep], got[keep]) and np.isnan(gotb[rows[0], 100:234]).all()
