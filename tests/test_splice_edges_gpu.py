"""GPU: ``cp_splice_apply`` behind both of its kernels -- ``splice_uniform_kernel<S>`` (csrc/cp_splice_uniform.h, scheme 1) and ``splice_kernel``
(csrc/cp_bao.hip, scheme 0) -- against the longdouble truth of tests/splice_truth.py, a full clamped-spline solve over all knots with no lanes, no halo
and no windows, where the kernels' pieces meet:
(a) a uniform stretch of 256 .. 3648 knots: every S = 33 .. 57 at 64 S knots (lane 63 owns the last knot, ``yu[64 S]``) and at 64 (S - 4) + 1, the last
    knot in a lane's first and last place (``mb0`` = p^-S .. p^-1), windows of 0, 1, 2 and 44 outside knots, one to eight blocks of spline queries,
    the first of them off a block of 64 and behind a block that holds none, queries ``nextafter`` the junctions; each plan under scheme 0 as well, with
    the constant slot of the stretch on both sides of its threshold (257 | 258 knots);
(b) plans the uniform scheme must refuse (3649 and 255 knots, 513 spline queries);
(c) irregular knots, scheme 0: 4 .. 700 knots and the largest plan of every family (S = 1, 3, 5, 11, 37, 39, 61; halos of 8 to 48 knots, fewer knots
    than the halo, one workgroup per CU past 64 KiB of LDS), queries outside the knots and NaN, the refusal one knot later, knots spliced from two arrays;
(d) batches of 1 .. 5 rows and more rows than a launch has waves, a NaN row that stays alone;
(e) wallish2018's own grids, with the levels of their restatements (no cap: DESIGN.md section 5).
Every plan is held to the layout restated in splice_truth (``cp_splice_plan_info`` against ``elimination_plan`` and the host build of the uniform tables).
Tolerance: the rule of tests/spline_truth.py per block (the interval in front of the stretch, the stretch, the interval behind it; a row where there is no
stretch), 16 levels of the worse of the plain float64 solve and the float64 restatement of the scheme that runs; each test prints the largest fraction used.
Measured on an MI355X, largest fraction of the allowance used: splice_uniform_kernel 0.209 (2625 knots, S = 45, tophat; levels up to 3.7 FLOOR), splice_kernel 0.193 on the
stretches (levels up to 5.5) and 0.146 on irregular knots (levels up to 28.4); wallish2018's grids 0.258 (scheme 1, levels of 555 and 41 900 FLOOR in front of and behind the
stretch) and 0.063 (scheme 0).
"""
import numpy as np
import pytest

import splice_truth as sp
import spline_truth as st

pytestmark = pytest.mark.gpu
NROWS = 11


def _env():
    import torch
    from cosmoprimo_amd.spline import SplicedClampedSpline
    return torch, SplicedClampedSpline, torch.device('cuda', 0)


def _stretch_plan(case):
    """The plan of a stretch case, held to the restated layout of both schemes."""
    torch, SplicedClampedSpline, dev = _env()
    op = SplicedClampedSpline(case['knots'], case['pieces'], case['xq'], device=dev)
    layout = op.layout
    uniform = layout.pop('uniform')
    assert layout == sp.layout_of(case['plan']), (layout, sp.layout_of(case['plan']))
    T = case['tables']
    assert uniform == (None if T is None else {key: T[key] for key in ('S', 'nm', 'wl', 'wr', 'gb0', 'ngb')}), (uniform, T)
    assert op.scheme == (0 if T is None else 1)
    return op


def _run_stretch(op, case, scheme, nrows=NROWS, label=None):
    torch, SplicedClampedSpline, dev = _env()
    op.scheme = scheme
    assert op.scheme == scheme
    rows0, rows1 = (torch.as_tensor(st.batch(case[key], nrows), device=dev) for key in ('rows0', 'rows1'))
    label = label or '%s, scheme %d' % (case['name'], scheme)
    worst = sp.assert_blocks(op(rows0, rows1).cpu().numpy(), case, scheme, 'spline', label)
    damped = op(rows0, rows1, tophat=torch.as_tensor(case['tophat'], device=dev)).cpu().numpy()
    return max(worst, sp.assert_blocks(damped, case, scheme, 'damped', label + ', tophat'))


@pytest.mark.parametrize('name', list(sp.STRETCH))
def test_uniform_stretch(name):
    case = sp.stretch_case(name)
    op = _stretch_plan(case)
    worst = max(_run_stretch(op, case, scheme) for scheme in (1, 0))
    print('%s (uniform S = %d, elimination S = %d): largest fraction %.3g' % (name, case['tables']['S'], case['plan']['S'], worst))


def test_every_uniform_kernel_is_launched():
    torch, SplicedClampedSpline, dev = _env()
    seen = set()
    for sizes in sp.UNIFORM_S.values():
        for nm in sizes:
            case = sp.stretch_inputs('nm%d' % nm)
            seen.add(SplicedClampedSpline(case['knots'], case['pieces'], case['xq'], device=dev).layout['uniform']['S'])
    assert seen == {33, 37, 41, 45, 49, 53, 57}


@pytest.mark.parametrize('name', list(sp.ELIMINATION_ONLY))
def test_plans_the_uniform_scheme_refuses(name):
    case = sp.stretch_case(name)
    op = _stretch_plan(case)
    assert op.scheme == 0 and op.layout['uniform'] is None
    with pytest.raises(NotImplementedError):
        op.scheme = 1
    assert op.scheme == 0
    print('%s: largest fraction %.3g' % (name, _run_stretch(op, case, 0)))


def _irregular_plan(case):
    torch, SplicedClampedSpline, dev = _env()
    op = SplicedClampedSpline(case['x'], case['pieces'], case['xq'], device=dev)
    layout = op.layout
    assert layout.pop('uniform') is None and op.scheme == 0
    assert layout == sp.layout_of(case['plan']), (layout, sp.layout_of(case['plan']))
    return op


def _rows(case, nrows):
    torch, SplicedClampedSpline, dev = _env()
    return [None if rows is None else torch.as_tensor(st.batch(rows, nrows), device=dev) for rows in case['rows']]


@pytest.mark.parametrize('name', sp.IRREGULAR_FAMILIES)
def test_irregular_knots(name):
    torch, SplicedClampedSpline, dev = _env()
    largest = sp.largest_irregular(name)
    worst, seen = 0., set()
    for n in sp.IRREGULAR_SIZES + [largest]:
        case = sp.irregular_case(name, n)
        op = _irregular_plan(case)
        seen.add((case['plan']['S'], case['plan']['halo']))
        if (name, n) in sp.IRREGULAR_OVER_CAP:
            continue
        got = op(*_rows(case, NROWS)).cpu().numpy()
        assert np.isnan(got[:, :3]).all()      # two queries outside the knots and a NaN
        worst = max(worst, st.assert_within(got, case['truth'], case['f8'], what='%s, %d knots' % (name, n), scaled=True))
    assert {S for S, halo in seen} == {1, 3, 5, 11, sp.irregular_case(name, largest)['plan']['S']}
    longer = sp.stc.knots(name, largest + 1)
    with pytest.raises(NotImplementedError):
        SplicedClampedSpline(longer, [(0, 0, longer.size)], longer[:8], device=dev)
    print('%s: largest fraction %.3g' % (name, worst))


@pytest.mark.parametrize('pieces', list(sp.PIECES))
def test_knots_spliced_from_two_arrays(pieces):
    case = sp.irregular_case('jitter100', 193, pieces)
    op = _irregular_plan(case)
    got = op(*_rows(case, NROWS)).cpu().numpy()
    st.assert_within(got, case['truth'], case['f8'], what='jitter100, 193 knots in %s pieces' % pieces, scaled=True)


def _alone(op, rows, spoil, plain):
    """A NaN in one knot value of row ``spoil[0]`` (array, column ``spoil[1:]``) leaves every other row bit for bit as it was."""
    torch, SplicedClampedSpline, dev = _env()
    row, which, column = spoil
    bad = [None if r is None else r.clone() for r in rows]
    bad[which][row, column] = float('nan')
    got = op(*bad)
    keep = torch.ones(len(plain), dtype=torch.bool, device=dev)
    keep[row] = False
    assert torch.equal(got[keep].view(torch.int64), plain[keep].view(torch.int64))      # (the bits: queries outside the knots are NaN in every row)
    assert torch.isnan(got[row, 3:]).any()


def test_batches_of_the_uniform_scheme():
    torch, SplicedClampedSpline, dev = _env()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    case = sp.stretch_case('nm256')
    op = _stretch_plan(case)
    worst = 0.
    for nrows in sp.BATCH_ROWS + [4 * cus + 5]:      # one workgroup of four waves per CU: a wave takes a second row
        worst = max(worst, _run_stretch(op, case, 1, nrows, 'nm256, scheme 1, %d rows' % nrows))
        rows = [torch.as_tensor(st.batch(case[key], nrows), device=dev) for key in ('rows0', 'rows1')]
        plain = op(*rows)
        _alone(op, rows, (nrows - 1, 0, 5), plain)                      # a knot in front of the stretch
        _alone(op, rows, (nrows // 2, 1, sp.SPARE[0] + 100), plain)     # a knot of the stretch
    print('batches, scheme 1: largest fraction %.3g' % worst)


def test_batches_of_the_elimination():
    torch, SplicedClampedSpline, dev = _env()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    worst = 0.
    # the largest irregular plan: more than half the LDS of a CU, one workgroup of four waves on each
    name = 'saw1.5x16'
    case = sp.irregular_case(name, sp.largest_irregular(name))
    op = _irregular_plan(case)
    assert op.layout['lds_bytes'] > 80 * 1024
    for nrows in sp.BATCH_ROWS + [4 * cus + 5]:
        rows = _rows(case, nrows)
        plain = op(*rows)
        worst = max(worst, st.assert_within(plain.cpu().numpy(), case['truth'], case['f8'], what='%s, %d knots, %d rows' % (name, case['n'], nrows), scaled=True))
        _alone(op, rows, (nrows - 1, 0, case['n'] // 2), plain)
    # 64 knots: many workgroups per CU.  More rows than the launch has waves where ``spline_truth.batch`` has that many, its 8704 rows otherwise
    case = sp.irregular_case('saw2x40', 64)
    op = _irregular_plan(case)
    resident = 4 * cus * max(160 * 1024 // op.layout['lds_bytes'], 1)
    nrows = min(resident + 5, st.EXPONENTS.size)
    rows = _rows(case, nrows)
    plain = op(*rows)
    worst = max(worst, st.assert_within(plain.cpu().numpy(), case['truth'], case['f8'], what='saw2x40, 64 knots, %d rows (%d waves)' % (nrows, resident), scaled=True))
    _alone(op, rows, (nrows - 1, 0, 31), plain)
    print('batches, scheme 0: largest fraction %.3g' % worst)


def test_the_grids_of_wallish2018():
    torch, SplicedClampedSpline, dev = _env()
    case = sp.production_case()
    op = _stretch_plan(case)
    for scheme in (1, 0):
        worst = _run_stretch(op, case, scheme, label='wallish2018 grids, scheme %d' % scheme)
        print('wallish2018 grids, scheme %d: largest fraction %.3g' % (scheme, worst))
