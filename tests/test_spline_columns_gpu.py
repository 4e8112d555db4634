"""GPU: ``cp_spline_columns`` (``column_spline_kernel``, csrc/cp_spline.hip: natural splines with per-column knots, each column cut into up to 8 parts
that eliminate from 32 knots below their run to 32 above) through the C ABI, against the longdouble truth of tests/spline_truth.py -- one solve
over all knots of a column.
Sizes on either side of every change of the number of parts (n - 1 = 160, 240, ..., 640) and 3, 4 knots; 1, 63, 64, 65 and 130 columns; column c
holds family c % 5 stretched by its own factor and shifted, so that the knots where its parts meet are its own; the queries are shared: random
ones over the range of all columns, for column 0 every knot at which a part begins, its first and last knot, a crowded interval and a run of empty
ones, two below and two above every column.  ``out`` is filled with a sentinel first: every (query, column) is written by exactly one part, or the
sentinel (never written) or a value of the neighbouring part's cubic (written twice) remains.  A NaN among one column's values leaves the other
columns bit for bit.  One query alone (the bits it has among the others), and queries all outside, besides.
Tolerance: the rule of tests/spline_truth.py, 16 levels of the float64 restatement per column; each test prints the largest fraction it used.
Measured on an MI355X, largest fraction of the allowance used by cp_spline_columns: 0.23 (641 knots, 8 parts); <= 0.21 at every other size.  With the parts'
elimination cut to 4 knots of halo in a scratch copy of the kernel every case of more than one part fails, at 1e9 to 5e11 allowances; with ``>=`` turned into
``>`` where a part hands a query on its lowest knot to the part below, every case fails (the query is written by neither, or comes back NaN on the first knot).
"""
import numpy as np
import pytest

import spline_truth as st

pytestmark = pytest.mark.gpu
SENTINEL = -7777.


def _run(x, y, xq):
    """x, y (ncol, n) as the tests hold them -> (ncol, nq); the kernel's layout is knot-major, (n, ncol) and (nq, ncol)."""
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', 0)
    lib = _lib.load()
    ncol, n = x.shape
    parts = st.COLUMN_PARTS[st.COLUMN_SIZES.index(n)]
    need = int(lib.cp_spline_columns_scratch_doubles(ncol, n))
    assert need == 2 * parts * (st.column_run(n, parts) + 2 * st.COLUMN_HALO + 2) * ncol, (need, parts)      # the part count the case is built for
    xk, yk = (torch.as_tensor(np.ascontiguousarray(a.T), device=dev) for a in (x, y))
    tq = torch.as_tensor(np.ascontiguousarray(xq, dtype='f8'), device=dev)
    guard = 64      # doubles of sentinel behind the scratch and the output: nothing is written past either
    scratch = torch.full((need + guard,), SENTINEL, dtype=torch.float64, device=dev)
    out = torch.full((xq.size * ncol + guard,), SENTINEL, dtype=torch.float64, device=dev)
    _lib.check(lib.cp_spline_columns(xk.data_ptr(), yk.data_ptr(), ncol, n, tq.data_ptr(), xq.size, out.data_ptr(), scratch.data_ptr(), 0, dv.stream_of(dev)))
    assert bool((scratch[need:] == SENTINEL).all()) and bool((out[xq.size * ncol:] == SENTINEL).all())
    return out[:xq.size * ncol].reshape(xq.size, ncol).cpu().numpy().T


@pytest.mark.parametrize('ncol', st.COLUMN_COUNTS)
@pytest.mark.parametrize('n', st.COLUMN_SIZES)
def test_columns(n, ncol):
    case = st.column_case(n)
    x, y, xq = case['x'][:ncol], case['y'][:ncol], case['xq']
    truth, f64 = case['ld'][:ncol], case['f8'][:ncol]
    parts = st.COLUMN_PARTS[st.COLUMN_SIZES.index(n)]
    run = st.column_run(n, parts)
    assert all(x[0, part * run] in xq for part in range(parts)) and x[0, -1] in xq and (parts - 1) * run < n - 1
    got = _run(x, y, xq)
    assert not (got == SENTINEL).any(), 'not written: (query, column) {}'.format(np.argwhere(got.T == SENTINEL)[:5])
    outside = ~((xq[None, :] >= x[:, :1]) & (xq[None, :] <= x[:, -1:]))
    assert outside[:, :2].all() and outside[:, -2:].all() and np.array_equal(np.isnan(got), outside)
    worst = st.assert_within(got, truth, f64, what='%d knots, %d columns' % (n, ncol))
    if ncol > 1:      # a NaN among the values of column 1, at the lower knot of the interval of its middle query: the others bit for bit
        k = np.flatnonzero(~outside[1])
        k = k[k.size // 2]
        j = min(int(np.searchsorted(x[1], xq[k], side='right')) - 1, n - 2)
        bad = y.copy()
        bad[1, j] = np.nan
        gotb = _run(x, bad, xq)
        keep = np.arange(ncol) != 1
        assert np.array_equal(gotb[keep], got[keep], equal_nan=True) and np.isnan(gotb[1, k])
    print('columns, %d knots in %d parts, %d columns: largest fraction %.3g' % (n, parts, ncol, worst))


@pytest.mark.parametrize('n', [4, 162, 1000])
def test_one_query_and_all_outside(n):
    """A query's value does not depend on the queries around it: alone it gives the bits it has among the others (which test_columns holds to the truth)."""
    case = st.column_case(n)
    ncol = 65
    x, y, xq = case['x'][:ncol], case['y'][:ncol], case['xq']
    full = _run(x, y, xq)
    for k in (xq.size // 2, int(np.searchsorted(xq, x[0, n // 2])), int(np.searchsorted(xq, x[0, 0])), 0, xq.size - 1):      # any; at the middle and on the first knot of column 0; outside
        got = _run(x, y, xq[k:k + 1])
        assert not (got == SENTINEL).any() and np.array_equal(got, full[:, k:k + 1], equal_nan=True), k
    got = _run(x, y, np.array([-50., -10., -1., 2000., 5000., 1e4]))
    assert np.isnan(got).all()
