"""GPU: ``cp_kirkby2013_rows`` (csrc/cp_xi_filter.hip), called through the C ABI, against the longdouble truth of tests/xi_filter_truth.py where its
paths and its window meet:
(A) sizes on both sides of the rule that chooses between ``kirkby_rows_kernel`` ('staged': ns even, <= 1024, xi, xinow and s 16-byte aligned) and
    ``kirkby_rows_any_kernel`` ('any'): 5 to 16 samples, 126 to 130, 1022 to 1026, 1500, and 128 samples with each pointer misaligned alone; ratios 0.75 to 1.3 (0.98 to 1.02 for
    the lists of 5 to 16 samples, which a box sample must not leave; 0.5 to 2 from 1022 samples on);
(B) fit ranges of 63 to 193 samples starting at samples 0, 1 and 37 of 256, ending inside the right box, at ns, and between the boxes;
(C) separations exactly on the 8 knots and on their float64 neighbours, at ratios 1, 0.5, 2 and one that is no power of two, with weights that have a
    step at knots[0], knots[7] (precision) and knots[2], knots[5] (blend), and samples inside the 1e-12 margin of ``maybe_center``;
(D) 1, 3, 4, 5 and 8197 rows (one trip of the grid takes 8192), rows_per_cosmology 1, 3 (not dividing), 8197 and 10000: rows that share a base row
    and a ratio are bit-identical after their 2^e is taken out, across trips and waves;
(E) in place (d_xinow = d_xi) on both paths, bit-identical to out of place;
(F) NaN rows, NaN and inf at a fit sample of weight 0, a NaN outside the fit range and the blend, a NaN ratio and a ratio of 100 (no weighted
    sample: 0 / 0 in the first pivot) inside the 8197 rows: NaN exactly where the truth has it, every other row bit-identical to a run without them.
Every comparison (``xi_filter_truth.check``): NaN exactly where the truth has it; the blended samples (knots[2] <= s / rho <= knots[5]) within
ALLOW = 16 levels of the float64 restatement times the row's largest |truth| over its blended samples; every sample of blend factor 0 equal to the
input bit for bit.  ``staged`` restates the dispatch rule, and every case names the kernel it expects.

Levels the allowances rest on (tests/test_xi_filter_truth_host.py, both summation orders): 2.4e-11 to 5.5e-11 for 6 to 16 samples, 3.8e-11 to 9.0e-11
for 126 to 1500, 3.2e-12 to 1.7e-11 for the fit ranges that cut the right box and 3.9e-11 / 5.2e-11 for those that end between the boxes, 3.1e-11 to
6.9e-11 on the knot grids, 2.0e-11 (16 samples) and 5.0e-11 (15) for the 8197 rows.  One fit sample of weight >= 0.5 less moves the truth of some row by 7.6e4
allowances or more.
Measured on an MI355X, largest fraction of the allowance used: A 0.077 (6 samples; 0.034 or less from 7 to 1500 and with a pointer misaligned), B 0.055
(fit range [37, 100)), C 0.017, D, E and F 0.050 (the 8197 rows of 16 samples; 0.044 with 15): the kernel's rounding stays a factor 13 or more inside
what its float64 restatement is allowed.
In scratch copies of the library, changes that alter numbers and no address outside the arrays:
- the fit loop of ``kirkby_rows_kernel`` without its last partial pass: the 43 tests labelled 'staged' whose fit range is no multiple of 64 fail (all
  eight staged sizes of A, 17 of the 23 ranges of B and both that end between the boxes, C, D, E, F), at 1.4e7 to 5.6e11 allowances; no test labelled
  'any' fails;
- the same in ``kirkby_rows_any_kernel``: the 27 tests labelled 'any' fail (all seven sizes of A -- 5 samples by a row of NaN -- and the six misaligned
  cases, C, D, E, F), at 1.4e7 to 2.4e11 allowances; no test labelled 'staged' fails.  (Before the ratios 2 and 0.5 were added from 1022 samples on,
  1022 to 1500 samples passed both changes: the last partial pass of the filter's fit range lies beyond the window at ratios up to 1.3.)
- ``x > xp[k]`` for ``x >= xp[k]`` in ``interp``: the two knot grids with the general weights fail, at 7.2e7 (any) and 1.2e8 (staged) allowances; with
  the default weights both steps are continuous and the change cannot show;
- ``row % rows_per_cosmology`` (kept inside the ratios) in ``rescale_of``: 64 of the 76 tests fail, first by samples of blend factor 0 that differ from
  the input; those that pass have rows_per_cosmology 1, 8197 or 10000, where the index is the same.
"""
import numpy as np
import pytest

import xi_filter_truth as xt

pytestmark = pytest.mark.gpu
NROWS, PER = 23, 3      # 8 cosmologies, the last with 2 rows


def _env():
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    return torch, _lib, dv, torch.device('cuda', 0)


def staged(ns, xi, out, s):
    """The dispatch rule of cp_kirkby2013_rows: does ``kirkby_rows_kernel`` take these tensors?"""
    return ns % 2 == 0 and ns <= 1024 and all(t.data_ptr() % 16 == 0 for t in (xi, out, s))


def _tensor(values, dev, misaligned=False):
    """A contiguous float64 tensor of the values; ``misaligned``: a view one element into a longer one (8 bytes off a 16-byte boundary)."""
    torch = _env()[0]
    values = np.ascontiguousarray(values, dtype='f8')
    if not misaligned:
        t = torch.tensor(values, device=dev)
        assert t.data_ptr() % 16 == 0
        return t
    whole = torch.zeros(values.size + 1, dtype=torch.float64, device=dev)
    t = whole[1:].view(values.shape)
    t.copy_(torch.tensor(values))
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()
    return t


def run(case, rows, ratios, per, kernel, misaligned=(), in_place=False):
    """xinow (numpy) of the rows at the ratios (one per cosmology of ``per`` rows); ``kernel``: 'staged' or 'any', held to :func:`staged`;
    ``misaligned``: of 'xi', 'out', 's'."""
    torch, _lib, dv, dev = _env()
    rows = np.asarray(rows)
    nrows, ns = rows.shape
    assert ns == case.ns and len(ratios) >= -(-nrows // per)
    xi = _tensor(rows, dev, 'xi' in misaligned)
    out = xi if in_place else _tensor(np.zeros_like(rows), dev, 'out' in misaligned)
    s = _tensor(case.s, dev, 's' in misaligned)
    rescale = _tensor(ratios, dev)
    assert staged(ns, xi, out, s) == (kernel == 'staged'), (ns, misaligned, kernel)
    _lib.check(_lib.load().cp_kirkby2013_rows(xi.data_ptr(), out.data_ptr(), nrows, ns, s.data_ptr(), case.fit[0], case.fit[1], rescale.data_ptr(), per,
                                              _lib.as_double_p(np.ascontiguousarray(case.knots, dtype='f8')), _lib.as_double_p(np.ascontiguousarray(case.weights, dtype='f8')),
                                              dev.index, dv.stream_of(dev)))
    return out.cpu().numpy()


def _ratios(case, nrows, per, index=None):
    ncosmo = -(-nrows // per)
    index = np.arange(ncosmo) % len(case.ratios) if index is None else index[:ncosmo]
    return case.ratios[index]


def _compare(case, kernel, what, **kwargs):
    got = run(case, xt.batch(case.base, NROWS), _ratios(case, NROWS, PER), PER, kernel, **kwargs)
    return xt.check(case, got, NROWS, PER, what='%s (%s kernel)' % (what or case.label, kernel))


# ---- A ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ns', sorted(xt.STAGED_SIZES + xt.ANY_SIZES))
def test_sizes(ns):
    kernel = 'staged' if ns in xt.STAGED_SIZES else 'any'
    assert (kernel == 'staged') == (ns % 2 == 0 and ns <= 1024)
    case = xt.size_case(ns)
    worst = _compare(case, kernel, '')
    if ns == 5:      # all in the boxes: nothing is blended, the output is the input
        assert case.zero.all() and worst == 0.
    print('A, %d samples: largest fraction %.3g' % (ns, worst))


@pytest.mark.parametrize('general', [False, True], ids=['default', 'general'])
@pytest.mark.parametrize('misaligned', [(), ('xi',), ('out',), ('s',)], ids=['aligned', 'xi', 'xinow', 's'])
def test_each_pointer_misaligned(misaligned, general):
    case = xt.size_case(128, general)
    worst = _compare(case, 'any' if misaligned else 'staged', '128 samples, %s misaligned' % (misaligned or 'nothing',), misaligned=misaligned)
    print('A, 128 samples, %s, misaligned %s: largest fraction %.3g' % ('general' if general else 'default', misaligned, worst))


# ---- B ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fit', xt.RANGES, ids=['%d_%d' % r for r in xt.RANGES])
def test_fit_ranges(fit):
    case = xt.range_case(*fit)
    assert case.fit == (fit[0], fit[0] + fit[1]) and case.ns == 256
    print('B, %s: largest fraction %.3g' % (case.label, _compare(case, 'staged', '')))


@pytest.mark.parametrize('fit', xt.RANGES_SHORT, ids=['%d_%d' % r for r in xt.RANGES_SHORT])
def test_fit_range_ends_between_the_boxes(fit):
    case = xt.range_case_short(*fit)
    assert case.blend[:, case.fit[1]:].any()      # blended samples outside the fit range
    print('B, %s: largest fraction %.3g' % (case.label, _compare(case, 'staged', '')))


# ---- C ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('general', [True, False], ids=['general', 'default'])
@pytest.mark.parametrize('odd', [False, True], ids=['staged', 'any'])
def test_knot_edges(odd, general):
    case = xt.edge_case(odd, general)
    print('C, %s: largest fraction %.3g' % (case.label, _compare(case, 'any' if odd else 'staged', '')))


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('nrows', [1, 3, 4, 5])
@pytest.mark.parametrize('ns', [16, 15])
def test_few_rows(ns, nrows):
    case = xt.many_case(ns)
    kernel = 'staged' if ns == 16 else 'any'
    got = run(case, xt.batch(case.base, nrows), _ratios(case, nrows, 2), 2, kernel)
    print('D, %d rows of %d: largest fraction %.3g' % (nrows, ns, xt.check(case, got, nrows, 2, what='%d rows of %d samples (%s kernel)' % (nrows, ns, kernel))))


def _many(ns, per, spoil=None, in_place=False):
    """The 8197 rows of ``ns`` samples at ``per`` rows per cosmology: (case, rows, ratios, index of each cosmology's ratio, output)."""
    case = xt.many_case(ns)
    index = xt.many_ratios(per)
    rows, ratios = xt.batch(case.base, xt.MANY_ROWS), case.ratios[index]
    if spoil is not None:
        spoil(rows, ratios)
    return case, rows, ratios, index, run(case, rows, ratios, per, 'staged' if ns == 16 else 'any', in_place=in_place)


@pytest.mark.parametrize('per', xt.MANY_PER_COSMOLOGY)
@pytest.mark.parametrize('ns', [16, 15])
def test_many_rows(ns, per):
    case, rows, ratios, index, got = _many(ns, per)
    assert ratios.size == {1: 8197, 3: 2733, 8197: 1, 10000: 1}[per] and xt.MANY_ROWS > 2048 * 4
    worst = xt.check(case, got, xt.MANY_ROWS, per, index, what='%d rows of %d samples, %d per cosmology' % (xt.MANY_ROWS, ns, per))
    # rows that share a base row and a ratio: the same bits once their 2^e is out, whichever trip and wave they ran in
    value = xt.unscale(got)
    key = (np.arange(xt.MANY_ROWS) % xt.NBASE) * len(case.ratios) + index[xt.ratio_index(xt.MANY_ROWS, per)]
    groups, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    assert groups.size == xt.NBASE * np.unique(index).size
    assert np.array_equal(value, value[first[inverse]])
    print('D, %d rows of %d, %d per cosmology: largest fraction %.3g' % (xt.MANY_ROWS, ns, per, worst))


# ---- E ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ns', [16, 15])
def test_in_place_many_rows(ns):
    case, rows, ratios, index, apart = _many(ns, 3)
    together = _many(ns, 3, in_place=True)[4]
    assert np.array_equal(together.view('u8'), apart.view('u8'))
    print('E, %d rows of %d in place: largest fraction %.3g' % (xt.MANY_ROWS, ns, xt.check(case, together, xt.MANY_ROWS, 3, index, what='in place, %d samples' % ns)))


@pytest.mark.parametrize('ns', [128, 129, 1024, 1500])
def test_in_place(ns):
    case = xt.size_case(ns)
    kernel = 'staged' if ns in (128, 1024) else 'any'
    rows, ratios = xt.batch(case.base, NROWS), _ratios(case, NROWS, PER)
    apart = run(case, rows, ratios, PER, kernel)
    together = run(case, rows, ratios, PER, kernel, in_place=True)
    assert np.array_equal(together.view('u8'), apart.view('u8'))
    print('E, %d samples in place: largest fraction %.3g' % (ns, xt.check(case, together, NROWS, PER, what='in place, %d samples (%s kernel)' % (ns, kernel))))


# ---- F ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ns', [16, 15])
def test_non_finite_inside_many_rows(ns):
    per = 3
    case, clean_rows, clean_ratios, index, clean = _many(ns, per)
    b, e = case.fit
    nan_row, nan_unweighted, inf_unweighted, nan_outside = 100, 4200, 8196, 5000      # (8196: in the second trip of the grid)
    nan_ratio, no_weight = 2731, 2000                                                 # cosmologies: rows 8193 to 8195, rows 6000 to 6002

    def unweighted(row):
        w = xt.window_of(case.s, clean_ratios[row // per], case.knots, case.weights)[0]
        return b + int(np.flatnonzero(w[b:e] == 0)[0])

    def spoil(rows, ratios):
        rows[nan_row] = np.nan
        rows[nan_unweighted, unweighted(nan_unweighted)] = np.nan
        rows[inf_unweighted, unweighted(inf_unweighted)] = np.inf
        rows[nan_outside, 0] = np.nan
        ratios[nan_ratio] = np.nan
        ratios[no_weight] = 100.

    _, rows, ratios, _, got = _many(ns, per, spoil)
    touched = np.zeros(xt.MANY_ROWS, dtype=bool)
    touched[[nan_row, nan_unweighted, inf_unweighted, nan_outside]] = True
    touched[nan_ratio * per:(nan_ratio + 1) * per] = True
    touched[no_weight * per:(no_weight + 1) * per] = True
    assert touched.sum() == 10 and b == 1 and not case.blend[:, 0].any()
    # every other row: the bits of the run without them
    assert np.array_equal(got[~touched].view('u8'), clean[~touched].view('u8'))
    worst = xt.check(case, got, xt.MANY_ROWS, per, index, rows=~touched, what='the neighbours of non-finite rows, %d samples' % ns)
    # the touched rows: NaN exactly where the truth has it
    for row in np.flatnonzero(touched):
        with np.errstate(invalid='ignore'):
            true = xt.truth(case.s, rows[row], ratios[row // per], b, e, case.knots, case.weights)
        assert np.array_equal(np.isnan(got[row]), np.isnan(true)), row
        assert np.isnan(true).all() or row == nan_outside
    assert np.isnan(got[touched & (np.arange(xt.MANY_ROWS) != nan_outside)]).all()
    alone = got[nan_outside]
    assert np.isnan(alone[0]) and np.array_equal(alone[1:].view('u8'), clean[nan_outside, 1:].view('u8'))      # exactly one NaN comes out
    print('F, non-finite rows among %d of %d samples: largest fraction %.3g' % (xt.MANY_ROWS, ns, worst))
