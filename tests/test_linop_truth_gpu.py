"""GPU: the four operator kernels of csrc/cp_spline.hip -- spline_apply_kernel<4 | 8 | 16>, spline_outer_kernel<2 | 4 | 8>, linop_mfma_kernel<false | true> and
linop_mid_mfma_kernel -- against the longdouble truth of tests/linop_truth.py, through the C ABI (cp_spline_apply_grouped, cp_spline_apply_outer,
cp_linop_apply_mid) into buffers of canaries: every element written, the one behind the output untouched.  tests/test_linop_truth_host.py holds the truth,
the cap of every case used here, the restated plan and the mutations these cases catch.  Allowance: ALLOW = 16 levels of the float64 restatements -- per row
against the row's largest |truth| for spline plans, per (row, 64 queries) against sum_j |W| |y| for dense ones --, + 3 FLOOR of the value for roots (held
squared), ln 10 times the argument's allowance + 4e-15 behind exp10.  A query on a knot (nu = 0, no epilogue, a power of two as scale) returns the sample bit
for bit.  The kernel variant of every launch is asserted from ``plan_of`` and the row count; every test prints the largest fraction of its allowance.

  spline plans   every (family, n, end condition, nu) in use, n in 5, 16, 17, 100, 481, 1000, at the knots / midpoints / random points, beyond the knots with the
                 end cubics continued and without (NaN queries first, last and inside a tile), thinned, crowded and 1 ... 513 queries; the vector route, the
                 matrix-core route where the plan keeps a dense copy, the default bit for bit one of the two; 1 ... 65 rows; 8704 rows x 1030 queries;
                 groups 0, 64, 13, 128; a NaN sample; both post ops; scale 3
  dense plans    full operators (16, 1) ... (1024, 256), bands of 1, 7, 8, 9, 17 weights from knot 0 and to knot n - 1 with rows of zeros and NaN queries,
                 sub_windows true and false, span_max > 512 (R = 8 by the 64 KB bound)
  outer          nq 1, 256, 257 x nz 1 ... 511 x 1 ... 9 rows; 8704 rows; the root; a NaN query
  middle axis    (n, nq, m, nb) from (5, 1, 1, 1) to (33, 130, 129, 350), resident and not; the three epilogues; a NaN query; a NaN sample

Largest fraction of the allowance measured on the MI355X (1 is the limit; 1 / 16 = 0.0625 is a float64 restatement's own distance): spline_apply_kernel<4> 0.252,
<8> 0.350, <16> 0.453; linop_mfma_kernel<false> 0.312, <true> 0.453; spline_outer_kernel<2> 0.121, <4> 0.137, <8> 0.420; linop_mid_mfma_kernel resident 0.071, not
resident 0.087.  No kernel, no part of the restated plan and no truth was found wrong.  What these cases found is on the host: with the float64 weights of
cp_spline_operator the first derivative of the natural spline through 100 uniform knots, one interval below the first knot, stood at 1.36 of its allowance on both
routes (4.1e-15 of the row's largest value; the numpy product with the same weights gives the same figure, with the rounded longdouble weights 0.07).
cp_spline_operator now forms the weights of derivatives, of continued end cubics and of unevenly spaced knots in extended precision (csrc/cp_spline.hip).
"""
import numpy as np
import pytest

import linop_truth as lt
import spline_truth as st
from sigma_device import CANARY, synchronized

pytestmark = pytest.mark.gpu

LD = np.longdouble
WORST = {}
NROWS = 17      # R = 16 of the vector route, one partial row tile of the matrix cores, the default route past its nrows >= 16


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


def note(variant, fraction):
    WORST[variant] = max(WORST.get(variant, 0.), fraction)
    print('MEASURED %-36s largest fraction of the allowance so far %.3f' % (variant, WORST[variant]))
    return fraction


def guarded(env, count):
    torch, dev = env[0], env[3]
    return torch.full((count + 1,), CANARY, dtype=torch.float64, device=dev)


def collect(env, out):
    host = synchronized(env[0], out)
    assert host[-1] == CANARY, 'the element behind the output was written'
    assert not (host[:-1] == CANARY).any(), '{:d} output elements were not written'.format(int((host[:-1] == CANARY).sum()))
    return host[:-1]


def on_device(env, a):
    return env[0].as_tensor(np.ascontiguousarray(a, dtype='f8'), device=env[3])


def apply(env, op, rows, group=0, post=0, scale=1., path=None):
    """(nrows, nq): cp_spline_apply_grouped into canaries, the grouped layout brought back to rows."""
    torch, _lib, lib, dev, stream = env
    tin = rows if torch.is_tensor(rows) else on_device(env, rows)
    nrows = tin.shape[0]
    out = guarded(env, nrows * op.nq)
    _lib.check(lib.cp_spline_apply_grouped(op._handle, tin.data_ptr(), out.data_ptr(), nrows, int(group), int(post) | lt.PATHS[path], float(scale), stream))
    return lt.ungroup(collect(env, out), nrows, op.nq, group)


def routes(plan):
    assert 4 * plan['span_max'] * 8 <= 160 * 1024
    return ['valu', 'mfma'] if plan['dense'] else ['valu']


def variant(plan, nrows, path):
    if path == 'mfma':
        return 'linop_mfma_kernel<%s>' % ('true' if plan['sub_windows'] else 'false')
    return 'spline_apply_kernel<%d>' % lt.apply_rows(plan, nrows)


def on_all_routes(env, op, plan, rows, judge, **kw):
    """Both forced routes judged, the default bit for bit one of the two (the one plan_of names)."""
    got = {}
    for path in routes(plan):
        got[path] = apply(env, op, rows, path=path, **kw)
        assert note(variant(plan, len(rows), path), judge(got[path], path)) <= 1.
    default = apply(env, op, rows, **kw)
    assert np.array_equal(default, got[lt.default_route(plan, len(rows))], equal_nan=True), 'the default route is not the %s route' % lt.default_route(plan, len(rows))
    return got


def check_plan(op, plan):
    assert op.bandwidth == plan['bw'] and op.columns == (plan['col_first'], plan['col_last'] - plan['col_first']), (op.bandwidth, plan['bw'], op.columns)


def spline_operator(env, key, xq, extrapolate):
    from cosmoprimo_amd.spline import LinearOperator, dense_operator
    name, n, bc, nu = key
    x = st.knots(name, n)
    op = LinearOperator.spline(x, xq, bc=bc, nu=nu, extrapolate=extrapolate, device=env[3])
    plan = lt.plan_of(dense_operator(x, xq, bc=bc, nu=nu, extrapolate=extrapolate))
    check_plan(op, plan)
    return op, plan


# ---- spline plans --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('key', lt.spline_used(), ids=lambda key: '%s-%d-%s-nu%d' % key)
def test_spline_plan(env, key):
    name, n, bc, nu = key
    case = lt.spline_case(name, n, bc)
    rows, e = st.batch(case['y'], NROWS), st.exponents(NROWS)
    for label, xq, extrapolate in lt.query_sets(key):
        op, plan = spline_operator(env, key, xq, extrapolate)
        truth, f64 = lt.spline_values(case, nu, xq, extrapolate)
        what = '%s, %s (%d queries)' % (key, label, xq.size)
        got = on_all_routes(env, op, plan, rows, lambda g, path: lt.spline_fraction(g, truth, f64, e=e, what='%s, %s' % (what, path)))
        if nu == 0:      # on_knots_exact: u = 0, one weight of one, the sample bit for bit (the last knot is served by the last interval from its far end)
            on = np.isin(xq, case['x'][:-1])
            at = np.searchsorted(case['x'], xq[on])
            for path, g in got.items():
                assert np.array_equal(g[:, on], rows[:, at]), '%s, %s: a query on a knot does not return the sample' % (what, path)


ROWS_CASE = ('uniform', 481, 'natural', 0)      # 1441 queries: six tiles of the vector route, 23 of the matrix cores


@pytest.mark.parametrize('nrows', lt.ROW_COUNTS)
def test_row_counts(env, nrows):
    case = lt.spline_case(*ROWS_CASE[:3])
    xq, extrapolate = lt.queries(case['x'], 'knots')
    op, plan = spline_operator(env, ROWS_CASE, xq, extrapolate)
    assert lt.apply_rows(plan, nrows) == (4 if nrows <= 4 else 8 if nrows <= 8 else 16) and plan['dense']
    assert lt.default_route(plan, nrows) == ('mfma' if nrows >= 16 and plan['prefer_dense'] else 'valu')
    truth, f64 = lt.spline_values(case, 0, xq, extrapolate)
    on_all_routes(env, op, plan, st.batch(case['y'], nrows), lambda g, path: lt.spline_fraction(g, truth, f64, e=st.exponents(nrows), what='%d rows, %s' % (nrows, path)))


def test_more_rows_than_either_grid(env):
    """8704 rows x 1000 knots -> 1030 queries: 544 x 5 items of the vector route against its grid of 2048, 136 x 5 of the matrix cores against 512."""
    torch, dev = env[0], env[3]
    key = ('sigma_r', 1000, 'natural', 0)
    case = lt.spline_case(*key[:3])
    xq = lt.counted(case['x'], 1030)
    op, plan = spline_operator(env, key, xq, False)
    nrows = lt.MANY_ROWS
    assert -(-nrows // 16) * len(plan['tiles']) > 2048 and -(-nrows // 64) * -(-plan['nq_pad'] // 256) > 512
    truth, f64 = lt.spline_values(case, 0, xq, False)
    assert lt.spline_level(truth, f64) <= lt.CAP
    e = st.exponents(nrows)
    rows = (on_device(env, case['y'])[torch.arange(nrows, device=dev) % lt.NBASE] * on_device(env, np.ldexp(1., e))[:, None]).contiguous()      # exact products
    for path in routes(plan):
        got = apply(env, op, rows, path=path)
        worst = max(lt.spline_fraction(got[a:a + 1001], truth, f64, e=e[a:a + 1001], first=a, what='rows %d ..., %s' % (a, path)) for a in range(0, nrows, 1001))
        assert note(variant(plan, nrows, path), worst) <= 1.


@pytest.mark.parametrize('group,nrows', [(0, 65), (64, 128), (13, 26), (128, 256)])
def test_grouped_store(env, group, nrows):
    """The plain store, the one-group fast store (a group of one row tile, of two) and the general one, on both routes."""
    key = ('geom1.05', 100, 'natural', 0)
    case = lt.spline_case(*key[:3])
    xq, extrapolate = lt.queries(case['x'], 'beyond')
    op, plan = spline_operator(env, key, xq, extrapolate)
    truth, f64 = lt.spline_values(case, 0, xq, extrapolate)
    on_all_routes(env, op, plan, st.batch(case['y'], nrows), lambda g, path: lt.spline_fraction(g, truth, f64, e=st.exponents(nrows), what='group %d, %s' % (group, path)),
                  group=group)


@pytest.mark.parametrize('n', [17, 100, 1000])
def test_nan_sample_stays_in_its_row(env, n):
    """A NaN in knot 0 of one row: the query on knot 0 of that row is NaN, every other row is held -- the row in front of it too, whose last chunk of 16
    knots ends in that sample on the matrix-core route (n is no multiple of 16)."""
    key = ('uniform', n, 'natural', 0)
    case = lt.spline_case(*key[:3])
    xq, extrapolate = lt.queries(case['x'], 'knots')
    op, plan = spline_operator(env, key, xq, extrapolate)
    truth, f64 = lt.spline_values(case, 0, xq, extrapolate)
    rows, e = st.batch(case['y'], NROWS), st.exponents(NROWS)
    bad = 9
    rows[bad, 0] = np.nan
    keep = np.arange(NROWS) != bad
    assert n % 16 and xq[0] == case['x'][0]
    for path in routes(plan):
        got = apply(env, op, rows, path=path)
        assert np.isnan(got[bad, 0])
        got[bad] = apply(env, op, st.batch(case['y'], NROWS)[bad:bad + 1], path='valu')[0]      # (the row without its NaN, for the shape of the rule)
        assert note(variant(plan, NROWS, path), lt.spline_fraction(got, truth, f64, e=e, what='NaN sample, n = %d, %s' % (n, path))) <= 1. and keep.sum() == NROWS - 1


@pytest.mark.parametrize('post,scale', [(lt.POST_SQRT, 1.), (lt.POST_SQRT, 3.), (lt.POST_EXP10, 1.), (lt.POST_EXP10, 0.25), (lt.POST_NONE, 3.), (lt.POST_NONE, 2.**-7)])
def test_spline_post_ops(env, post, scale):
    for key, kind in ((('uniform', 100, 'natural', 0), 'beyond'), (('sigma_r', 481, 'not-a-knot', 0), 'knots')):
        case = lt.spline_case(*key[:3])
        xq, extrapolate = lt.queries(case['x'], kind)
        op, plan = spline_operator(env, key, xq, extrapolate)
        truth, f64 = lt.spline_values(case, 0, xq, extrapolate, scale)
        scaled = post != lt.POST_EXP10
        rows = st.batch(case['y'], NROWS) if scaled else lt.tile(case['y'], NROWS)
        e = st.exponents(NROWS) if scaled else None
        on_all_routes(env, op, plan, rows, lambda g, path: lt.spline_fraction(g, truth, f64, post, e=e, what='%s, post %d, scale %g, %s' % (key, post, scale, path)),
                      post=post, scale=scale)


# ---- dense plans ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(lt.dense_cases()))
def test_dense_plan(env, name):
    from cosmoprimo_amd.spline import LinearOperator
    case = lt.dense_case(name)
    plan = case['plan']
    op = LinearOperator.dense(case['w'], device=env[3])
    check_plan(op, plan)
    if name.startswith('sweep'):
        assert plan['sub_windows']
    if name.startswith('random'):
        assert not plan['sub_windows']
    if name == 'full_1000x1030':
        assert plan['span_max'] > 512 and lt.apply_rows(plan, NROWS) == 8
    for nrows in (NROWS, 5, 3):
        e = st.exponents(nrows)
        on_all_routes(env, op, plan, st.batch(case['y'], nrows),
                      lambda g, path: lt.dense_fraction(g, case['true'], case['scale'], case['level'], e=e, what='%s, %d rows, %s' % (name, nrows, path)))
    root = lt.dense_case(name, False)      # positive rows: the weights are of both signs, the root is NaN where the truth is negative
    on_all_routes(env, op, plan, st.batch(root['y'], NROWS), post=lt.POST_SQRT,
                  judge=lambda g, path: lt.dense_fraction(g, root['true'], root['scale'], root['level'], lt.POST_SQRT, e=st.exponents(NROWS), what='%s, root, %s' % (name, path)))
    on_all_routes(env, op, plan, lt.tile(case['y'], NROWS), post=lt.POST_EXP10,
                  judge=lambda g, path: lt.dense_fraction(g, case['true'], case['scale'], case['level'], lt.POST_EXP10, what='%s, exp10, %s' % (name, path)))
    if name in ('random_bw9', 'full_341x257'):      # the one scale that is no power of two
        three = lt.dense_case(name, True, 3.)
        on_all_routes(env, op, plan, st.batch(three['y'], NROWS), scale=3.,
                      judge=lambda g, path: lt.dense_fraction(g, three['true'], three['scale'], three['level'], e=st.exponents(NROWS), what='%s, scale 3, %s' % (name, path)))


# ---- outer epilogue ------------------------------------------------------------------------------------------------------------------------------
def outer(env, op, rows, g, post=0, scale=1.):
    torch, _lib, lib, dev, stream = env
    tin, tg = rows if torch.is_tensor(rows) else on_device(env, rows), g if torch.is_tensor(g) else on_device(env, g)
    nrows, nz = tin.shape[0], tg.shape[1]
    out = guarded(env, nrows * op.nq * nz)
    _lib.check(lib.cp_spline_apply_outer(op._handle, tin.data_ptr(), tg.data_ptr(), nz, out.data_ptr(), nrows, int(post), float(scale), stream))
    return collect(env, out).reshape(nrows, op.nq * nz)


@pytest.mark.parametrize('nq', lt.OUTER_NQ)
def test_outer_epilogue(env, nq):
    key = lt.OUTER_CASE + (0,)
    case = lt.spline_case(*lt.OUTER_CASE)
    reached = set()
    for nz in lt.OUTER_NZ:
        xq, g, truth, f64 = lt.outer_values(nq, nz)
        op, plan = spline_operator(env, key, xq, False)
        for nrows in lt.OUTER_ROWS:
            for post in ((lt.POST_NONE, lt.POST_SQRT) if nrows in (3, 9) else (lt.POST_NONE,)):
                R = lt.outer_rows(plan, nz, nrows)
                reached.add(R)
                got = outer(env, op, st.batch(case['y'], nrows), lt.tile(g, nrows), post)
                used = lt.spline_fraction(got, truth, f64, post, e=st.exponents(nrows), what='outer nq %d, nz %d, %d rows, post %d' % (nq, nz, nrows, post))
                assert note('spline_outer_kernel<%d>' % R, used) <= 1.
    assert reached == {2, 4, 8}
    if nq == 257:
        xq, g, truth, f64 = lt.outer_values(nq, 2, 3.)      # the one scale that is no power of two
        op, plan = spline_operator(env, key, xq, False)
        got = outer(env, op, st.batch(case['y'], 9), lt.tile(g, 9), 0, 3.)
        assert note('spline_outer_kernel<8>', lt.spline_fraction(got, truth, f64, e=st.exponents(9), what='outer, scale 3')) <= 1.


def test_outer_lds_step_and_more_rows_than_the_grid(env):
    """(span_max + 256 + nz) x rows x 8 bytes against 64 KB: R = 8 -> 4 on a plan whose span fills a tile; 1088 groups of 8 rows x 3 tiles against the grid of 2048."""
    torch, dev = env[0], env[3]
    key = lt.OUTER_CASE + (0,)
    case = lt.spline_case(*lt.OUTER_CASE)
    xq, g, truth, f64 = lt.outer_values(257, 511)
    op, plan = spline_operator(env, key, xq, False)
    assert 8 * (plan['span_max'] + 256 + 511) * 8 > 64 * 1024 and lt.outer_rows(plan, 511, 9) == 4 and lt.outer_rows(plan, 7, 9) == 8
    xq, g, truth, f64 = lt.outer_values(257, 2)
    nrows = lt.MANY_ROWS
    assert -(-nrows // 8) * len(plan['tiles']) > 2048 and lt.outer_rows(plan, 2, nrows) == 8
    e = st.exponents(nrows)
    index = torch.arange(nrows, device=dev) % lt.NBASE
    rows = (on_device(env, case['y'])[index] * on_device(env, np.ldexp(1., e))[:, None]).contiguous()
    got = outer(env, op, rows, on_device(env, g)[index].contiguous())
    worst = max(lt.spline_fraction(got[a:a + 1001], truth, f64, e=e[a:a + 1001], first=a, what='outer, rows %d ...' % a) for a in range(0, nrows, 1001))
    assert note('spline_outer_kernel<8>', worst) <= 1.


# ---- middle axis ---------------------------------------------------------------------------------------------------------------------------------
def mid(env, op, y, post=0, scale=1.):
    torch, _lib, lib, dev, stream = env
    ty = on_device(env, y)
    nb, n, m = ty.shape
    out = guarded(env, nb * op.nq * m)
    _lib.check(lib.cp_linop_apply_mid(op._handle, ty.data_ptr(), out.data_ptr(), nb, m, int(post), float(scale), stream))
    return collect(env, out).reshape(nb, op.nq, m)


@pytest.mark.parametrize('shape', lt.MID_SHAPES, ids=lambda shape: '%dx%dx%dx%d' % shape)
def test_middle_axis(env, shape):
    from cosmoprimo_amd.spline import LinearOperator
    n, nq, m, nb = shape
    case, root = lt.mid_case(shape), lt.mid_case(shape, False)
    plan = case['plan']
    op = LinearOperator.dense(case['w'], device=env[3])
    check_plan(op, plan)
    assert lt.mid_resident(plan) == (shape in ((5, 1, 1, 1), (32, 64, 129, 3))) and plan['dense']
    if nb == 350:
        assert nb * -(-m // 128) * (plan['nq_pad'] // 64) > 2048
    name = 'linop_mid_mfma_kernel, %s' % ('resident' if lt.mid_resident(plan) else 'not resident')
    e = st.exponents(nb)
    judge = lambda got, c, post, e, what: lt.dense_fraction(got, c['true'], c['scale'], c['level'], post, what='%s, %s' % (shape, what), block_axes=2, e=e)
    assert note(name, judge(mid(env, op, st.batch(case['y'].reshape(lt.NBASE, -1), nb).reshape(nb, n, m)), case, 0, e, 'plain')) <= 1.
    assert note(name, judge(mid(env, op, st.batch(root['y'].reshape(lt.NBASE, -1), nb).reshape(nb, n, m), lt.POST_SQRT), root, lt.POST_SQRT, e, 'root')) <= 1.
    assert note(name, judge(mid(env, op, lt.tile(case['y'], nb), lt.POST_EXP10), case, lt.POST_EXP10, None, 'exp10')) <= 1.
    if shape == (30, 65, 128, 2):
        three = lt.mid_case(shape, True, 3.)
        assert note(name, judge(mid(env, op, lt.tile(three['y'], nb), 0, 3.), three, 0, None, 'scale 3')) <= 1.
    # a NaN sample stays in its (batch entry, column)
    y = lt.tile(case['y'], nb).copy()
    b, j, c = nb - 1, n - 1, m // 2
    y[b, j, c] = np.nan
    got = mid(env, op, y)
    finite_query = ~np.isnan(case['w'][:, 0])
    assert np.isnan(got[b, finite_query, c]).all()
    got[b, :, c] = mid(env, op, lt.tile(case['y'], nb)[b:b + 1])[0, :, c]
    assert note(name, judge(got, case, 0, None, 'NaN sample')) <= 1.


def test_every_variant_was_reached():
    """The variants the cases above are there for, by the names the launches were given from plan_of and the row counts."""
    expected = ['spline_apply_kernel<%d>' % r for r in (4, 8, 16)] + ['spline_outer_kernel<%d>' % r for r in (2, 4, 8)]
    expected += ['linop_mfma_kernel<false>', 'linop_mfma_kernel<true>', 'linop_mid_mfma_kernel, resident', 'linop_mid_mfma_kernel, not resident']
    for name in sorted(WORST):
        print('MEASURED %-36s %.3f' % (name, WORST[name]))
    assert sorted(WORST) == sorted(expected)
