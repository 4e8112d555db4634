"""GPU: cp_spline_tables_build / cp_spline_tables_apply (csrc/cp_spline_tables.hip) at the edges of their runs and of their dispatch, against the
natural cubic spline and the linear interpolant in extended precision (tests/golden/spline_tables_edges.npz, tools/gen_spline_tables_edges_golden.py).
The tables are the knot families of tests/spline_tables_cases.py -- uniform, geometric, sawtooth and jittered spacings, far from the smooth distance
tables of tests/test_distance_to_redshift_batch_gpu.py -- stacked as the rows of one batch per size and driven through ``DistanceToRedshift``; the
values are its own redshift grid for zmax = 100.  The tolerance is that file's: |d| <= 1e-13 + 1e-11 |truth|.  scipy is no yardstick here (it solves
in float64 and is itself off by hundreds of tolerances on the sawtooth families).

Dispatch of the apply (cp_spline_tables.hip): rows of up to 2048 knots asked at least 4096 queries each are staged in LDS, ``nq // 8192`` workgroups
per row but about 2048 in all; everything else goes one lane per (row, query) through a grid-stride loop of 1 048 576 lanes."""
import numpy as np
import pytest

import spline_tables_cases as stc

pytestmark = pytest.mark.gpu
LDS_QUERIES = 4096


@pytest.fixture(scope='module')
def d2z_of():
    """``DistanceToRedshift`` of a batch of tables (rows, n), built once per (size, order) for the batches of the families."""
    import torch
    assert torch.cuda.is_available()
    from cosmoprimo_amd.utils import DistanceToRedshift
    cache = {}

    def make(table, order=3):
        table = np.ascontiguousarray(table, dtype='f8')
        return DistanceToRedshift(lambda z: table, zmax=stc.ZMAX, nz=table.shape[1], interp_order=order)

    def of(n, order=3):
        if (n, order) not in cache:
            cache[n, order] = make(stc.batch(n), order)
        return cache[n, order]

    of.make = make
    return of


def tile_to(q, nq):
    """Queries (..., m) repeated along the last axis to nq of them."""
    reps = -(-nq // q.shape[-1])
    return np.ascontiguousarray(np.tile(q, (1,) * (q.ndim - 1) + (reps,))[..., :nq])


@pytest.mark.parametrize('order', stc.ORDERS)
@pytest.mark.parametrize('n', stc.SIZES + stc.LARGE_SIZES)
def test_parity_with_the_truth(golden, d2z_of, n, order):
    """1. Every family at every size, both orders, per-cosmology and shared queries: within the tolerance of the extended-precision truth."""
    g = golden('spline_tables_edges')
    d2z = d2z_of(n, order)
    q, qs, truth, truth_shared = g['q_%d' % n], g['qs_%d' % n], g['t%d_%d' % (order, n)], g['ts%d_%d' % (order, n)]
    assert np.array_equal(q, [stc.queries(name, n) for name in stc.families(n)]) and np.array_equal(qs, stc.shared_queries(n))      # the fixture is of these knots
    got, got_shared = d2z(q, per_cosmology=True), d2z(qs)
    assert got.shape == truth.shape and got_shared.shape == truth_shared.shape
    errs = {name: max(stc.excess(got[i], truth[i]), stc.excess(got_shared[i], truth_shared[i])) for i, name in enumerate(stc.families(n))}
    print('parity n = %d, order %d: largest |d| / (1e-13 + 1e-11 |truth|) = %.3e (%s)' % (n, order, max(errs.values()), ', '.join('%s %.2e' % item for item in errs.items())))
    assert max(errs.values()) <= 1., errs


@pytest.mark.parametrize('n', [66, 2048, 2049])
def test_knots_reproduce_their_values(d2z_of, n):
    """2. A query equal to knot k returns zgrid[k] bit for bit, for all k of every row, through both apply kernels (one lane per (row, query); the
    knots repeated to 4096 queries per row for the rows staged in LDS, which 2049 knots never are).
    Knot k < n - 1 opens interval k and is its polynomial at u = 0, the stored value itself.  The last knot is the END of the last interval: a power
    form in x - x_{n-2} gives it within rounding only (an emulation with exact fused multiply-adds missed it by 1 to 109 units in the last place in 11 of
    the 78 (family, size) cases, 102 for alt1e3 at n = 66, and so did the device), so the last interval is stored and evaluated in a form that
    holds the values of both its knots (``table_last``, cp_spline_tables.hip)."""
    d2z = d2z_of(n)
    x = stc.batch(n)
    want = np.broadcast_to(stc.zgrid(n), x.shape)
    for nq in (n, LDS_QUERIES + n):
        got = d2z(tile_to(x, nq), per_cosmology=True)
        diff = got != tile_to(want, nq)
        where = sorted(set(int(k) % n for k in np.nonzero(diff)[1]))
        print('n = %d, %d queries per row: knots that do not come back bit for bit: %s' % (n, nq, where))
        assert not diff.any(), where


@pytest.mark.parametrize('n', [66, 2048])
def test_the_two_apply_kernels_agree(golden, d2z_of, n):
    """3a. The same 256 queries per row repeated to 4096 (rows staged in LDS) and 4095 of them (one lane per (row, query)): bit for bit."""
    g = golden('spline_tables_edges')
    for order in stc.ORDERS:
        d2z = d2z_of(n, order)
        for q, per_cosmology, truth in ((g['q_%d' % n], True, g['t%d_%d' % (order, n)]), (g['qs_%d' % n], False, g['ts%d_%d' % (order, n)])):
            staged = d2z(tile_to(q, LDS_QUERIES), per_cosmology=per_cosmology)
            lanes = d2z(tile_to(q, LDS_QUERIES - 1), per_cosmology=per_cosmology)
            assert staged.shape == (len(stc.families(n)), LDS_QUERIES) and np.array_equal(staged[:, :-1], lanes)
            assert np.array_equal(staged[:, :q.shape[-1]], d2z(q, per_cosmology=per_cosmology))
            assert stc.excess(staged, tile_to(truth, LDS_QUERIES)) <= 1.


def test_one_knot_more_than_lds_holds(golden, d2z_of):
    """3b. 2048 knots at 4096 queries per row are staged in LDS, 2049 knots are not: both against the truth."""
    g = golden('spline_tables_edges')
    for n in (2048, 2049):
        got = d2z_of(n)(tile_to(g['q_%d' % n], LDS_QUERIES), per_cosmology=True)
        err = stc.excess(got, tile_to(g['t3_%d' % n], LDS_QUERIES))
        print('n = %d, 4096 queries per row: %.3e of the tolerance' % (n, err))
        assert err <= 1.


def test_split_rows_with_a_ragged_tail(golden, d2z_of):
    """3c. 3 rows of 16 385 queries: two workgroups per row, the last query alone in its round."""
    g = golden('spline_tables_edges')
    n, nq = 130, 16385
    d2z = d2z_of.make(stc.batch(n)[[3, 4, 5]])      # saw2x40, alt1e3, jitter100
    q = g['q_%d' % n][[3, 4, 5]]
    lanes = d2z(q, per_cosmology=True)
    assert stc.excess(lanes, g['t3_%d' % n][[3, 4, 5]]) <= 1.
    assert np.array_equal(d2z(tile_to(q, nq), per_cosmology=True), tile_to(lanes, nq))
    qs = g['qs_%d' % n]
    assert np.array_equal(d2z(tile_to(qs, nq)), tile_to(d2z(qs), nq))


def test_more_rows_than_workgroups_to_split(golden, d2z_of):
    """3d. 2049 rows at 4096 queries: staged in LDS, one workgroup per row (the share of 2048 workgroups per row rounds to 0)."""
    g = golden('spline_tables_edges')
    n, nrows = 66, 2049
    base = stc.batch(n)
    rows = np.arange(nrows) % len(base)
    qs = g['qs_%d' % n]
    want = d2z_of(n)(qs)
    assert stc.excess(want, g['ts3_%d' % n]) <= 1.
    got = d2z_of.make(base[rows])(tile_to(qs, LDS_QUERIES))
    assert got.shape == (nrows, LDS_QUERIES) and np.array_equal(got, tile_to(want[rows], LDS_QUERIES))


def test_grid_stride_of_the_rows_kernel(golden, d2z_of):
    """3e. 3 rows of 2049 knots at 400 000 shared queries: 1.2e6 results for 1 048 576 lanes.  A strided sample against the truth of the same queries,
    all of them against the 128 distinct ones."""
    import torch
    g = golden('spline_tables_edges')
    n, nq = 2049, 400000
    qs, truth = g['qs_%d' % n], g['ts3_%d' % n][[0, 1, 0]]
    d2z = d2z_of.make(stc.batch(n)[[0, 1, 0]])
    got = d2z(torch.as_tensor(tile_to(qs, nq), device='cuda')).cpu().numpy()
    assert got.shape == (3, nq)
    sample = np.arange(0, nq, 997)
    err = stc.excess(got[:, sample], truth[:, sample % qs.size])
    print('grid stride: %.3e of the tolerance' % err)
    assert err <= 1. and got.size > 1048576
    assert np.array_equal(got, tile_to(d2z(qs), nq))


@pytest.mark.parametrize('n', [66, 2048])
def test_float32(golden, d2z_of, n):
    """3f. float32 in, float32 out: the float64 result of the same (float32) queries rounded once, through both kernels."""
    g = golden('spline_tables_edges')
    d2z = d2z_of(n)
    x = stc.batch(n)
    q32 = tile_to(g['qs_%d' % n], LDS_QUERIES).astype('f4')
    q32 = q32[(q32 >= x[:, 0].max()) & (q32 <= x[:, -1].min())]      # rounding to float32 may leave the tables
    assert q32.size >= LDS_QUERIES - 64
    q32 = tile_to(q32, LDS_QUERIES)
    for nq in (LDS_QUERIES, LDS_QUERIES - 1):
        got = d2z(q32[:nq])
        want = d2z(q32[:nq].astype('f8'))
        assert got.dtype == np.float32 and want.dtype == np.float64 and np.isfinite(want).all()
        assert np.array_equal(got, want.astype('f4'))


@pytest.mark.parametrize('n', [2, 66, 2049])
def test_range(d2z_of, n):
    """4. One unit in the last place outside either end knot: NaN, or ValueError with ``bounds_error``; the end knots themselves are inside.  Both kernels."""
    d2z = d2z_of(n)
    x = stc.batch(n)
    ends = x[:, [0, -1]].copy()
    for nq in (2, LDS_QUERIES):
        inside = tile_to(ends, nq)
        assert np.isfinite(d2z(inside, bounds_error=True, per_cosmology=True)).all()
        for col, direction in ((0, -np.inf), (1, np.inf)):
            q = inside.copy()
            q[:, col] = np.nextafter(ends[:, col], direction)
            expect = np.zeros(q.shape, dtype=bool)
            expect[:, col] = True
            assert np.array_equal(np.isnan(d2z(q, bounds_error=False, per_cosmology=True)), expect)
            with pytest.raises(ValueError):
                d2z(q, bounds_error=True, per_cosmology=True)
            one = inside.copy()      # ... and outside one row's table only
            one[-1, col] = q[-1, col]
            with pytest.raises(ValueError):
                d2z(one, per_cosmology=True)


def bad_rows(kind, rows):
    n = rows.shape[1]
    rows = rows.copy()
    if kind == 'equal':
        rows[:, 78] = rows[:, 77]
    elif kind == 'inf_last':
        rows[:, -1] = np.inf
    elif kind == 'nan_first':
        rows[:, 0] = np.nan
    else:
        k = {'swap_0_1': 0, 'swap_63_64': 63, 'swap_last': n - 2}[kind]
        rows[:, [k, k + 1]] = rows[:, [k + 1, k]]
    return rows


@pytest.mark.parametrize('kind', ['equal', 'inf_last', 'nan_first', 'swap_0_1', 'swap_63_64', 'swap_last'])
def test_bad_rows_stay_alone(d2z_of, kind):
    """5. 130 rows of 130 knots; rows 0, 63 and 64 with two equal neighbours, an infinite last knot, NaN at knot 0, or two knots swapped -- the first
    pair, (63, 64) where the lanes of the validity scan wrap, the last pair: NaN throughout, every other row bit for bit as in the batch without them."""
    n, nrows, positions = 130, 130, [0, 63, 64]
    base = stc.batch(n)
    clean = base[np.arange(nrows) % len(base)]
    table = clean.copy()
    table[positions] = bad_rows(kind, clean[positions])
    others = np.ones(nrows, dtype=bool)
    others[positions] = False
    rng = np.random.default_rng(130)
    per_row = clean[:, :1] + rng.uniform(0., 1., (nrows, 40)) * (clean[:, -1:] - clean[:, :1])
    shared = clean[:, 0].max() + rng.uniform(0., 1., LDS_QUERIES) * (clean[:, -1].min() - clean[:, 0].max())
    ref, d2z = d2z_of.make(clean), d2z_of.make(table)
    for q, per_cosmology in ((per_row, True), (shared, False)):
        want = ref(q, bounds_error=False, per_cosmology=per_cosmology)
        got = d2z(q, bounds_error=False, per_cosmology=per_cosmology)
        assert np.isfinite(want).all()
        assert np.isnan(got[positions]).all()
        assert np.array_equal(got[others], want[others])
    d2z(shared, bounds_error=True)      # a row that cannot be inverted is not out of range
