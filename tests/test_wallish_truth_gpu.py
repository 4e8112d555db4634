"""GPU: the box search and the box removal of wallish2018 (csrc/cp_wallish_dd.h) against the extended-precision truth of tests/wallish_truth.py, through the
two entry points that take sequences: ``cp_wallish_dd_box`` at n = 1024 (the elimination in LDS, two lanes sweeping towards the box) and n = 2048 (the
recursions in registers, the sweeps as composed affine maps) and ``cp_wallish_tail`` (the 2048 text on the XOR layout, rewriting in LDS and in d_coef).
tests/test_wallish_truth_host.py holds every case to the edge it is named for and the mutations to the cases that reject them.

Every output lies between canaries, inputs are compared with what was uploaded, every call is made twice and the two must give the same bits.
  cp_wallish_dd_box   every group of cases at both n, with d_dd present and absent, d_gap absent, out of place and in place: the boxes are the same in all
                      of them and equal to the truth's; d_dd by the rule (16 levels per sequence); the rewritten knots by the rule per (sequence, box), the
                      rest of the sequence bit for bit the input; the rewritten knots against cp_gap_spline on the same box within the sum of both
                      allowances.  A sequence that is not finite has no truth: its box follows numpy's argmax on the device's own second derivatives, and
                      the finite sequences beside it keep the bits they have without it.
                      1, 3, 4, 5 sequences, one trip of the grid plus 5, two trips plus 1: cyclic copies times powers of two, the bits of the short launch.
  cp_wallish_tail     the 2048-knot groups as pairs of sequences per row (CP_DST_SPLIT), the plans of an unrun filter, its own spectrum repeated: d_box equal
                      to the truth's and to cp_wallish_dd_box's, d_coef by the rule inside the box and bit for bit outside; d_out between canaries, and a row
                      with an invalid box has the d_out bits it has alone; a row that is not finite changes nothing of its partner.  The same row counts.

Measured on an MI355X, largest fraction of the allowance used (1 is the limit; 1 / 16 = 0.0625 is a float64 restatement's own distance): second derivatives
0.152 (n = 1024) and 0.148 (2048); rewritten box 0.588 in remove_box<16> (a box of one knot at a level of one FLOOR; the float64 restatement of the two sweeps
uses the same), 0.245 in remove_box_parallel, in cp_wallish_dd_box and in cp_wallish_tail alike.  No kernel was found wrong.
d_out of the tail is not compared with a reference here.  Two rows share one complex transform: a row's d_out differs by rounding with the data of a finite
partner (measured 4e-16 to 6e-15 relative, 2e-12 beside a row with planted dips a thousand times its size), and the second row of a pair (the imaginary half)
rounds differently from the first.  A row whose partner is missing or not finite has the bits of the row alone -- the first row of a pair run alone, the
second one run behind a row of zeros -- and that is what the rows with invalid boxes and the partners of the rows that are not finite are held to."""
import numpy as np
import pytest

import wallish_truth as wt
from sigma_device import CANARY, synchronized

pytestmark = pytest.mark.gpu

GUARD = 64
CANARY_INT = -1234567891
WORST = {}


@pytest.fixture(scope='module')
def env():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', torch.cuda.current_device())
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


def cus(env):
    return env[0].cuda.get_device_properties(env[3]).multi_processor_count


def note(route, fraction):
    WORST[route] = max(WORST.get(route, 0.), fraction)
    print('MEASURED %-44s largest fraction of the allowance so far %.3f' % (route, WORST[route]))


class Guarded(object):
    """A device array between GUARD canaries on either side; ``init`` (numpy) is uploaded, else the array itself is canaries."""

    def __init__(self, env, shape, init=None, integer=False):
        torch = env[0]
        self.env, self.shape, self.count = env, tuple(shape), int(np.prod(shape))
        self.canary = CANARY_INT if integer else CANARY
        self.buf = torch.full((self.count + 2 * GUARD,), self.canary, dtype=torch.int32 if integer else torch.float64, device=env[3])
        self.view = self.buf[GUARD:GUARD + self.count].view(self.shape)
        if init is not None:
            self.view.copy_(torch.as_tensor(np.array(init), device=env[3]))

    def ptr(self):
        return self.view.data_ptr()

    def guards_intact(self):
        torch = self.env[0]
        ends = synchronized(torch, torch.cat([self.buf[:GUARD], self.buf[GUARD + self.count:]]))
        assert (ends == self.canary).all(), 'written outside the array'

    def host(self, written=True):
        """The array on the host: canaries intact, and (``written``) no element left a canary."""
        self.guards_intact()
        out = synchronized(self.env[0], self.view)
        if written:
            assert not (out == self.canary).any(), '{:d} elements were not written'.format(int((out == self.canary).sum()))
        return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view('u1'), b.view('u1'))


def same_values(a, b):
    return np.array_equal(a, b, equal_nan=True)


def dd_box(env, y, n, setting, want_dd, gap, download=True):
    """cp_wallish_dd_box twice on fresh buffers; gap: None, 'out' (a copy of y) or 'in' (y itself).  Returns dict(box, dd, gap) of numpy arrays (None where
    absent), or the Guarded arrays of the first call with ``download=False``."""
    torch, _lib, lib, dev, stream = env
    mf, ms, off0, off1 = setting
    rows = len(y)
    calls = []
    for _ in range(2):
        ty, box = Guarded(env, y.shape, init=y), Guarded(env, (rows, 2), integer=True)
        dd = Guarded(env, y.shape) if want_dd else None
        out = Guarded(env, y.shape, init=y) if gap == 'out' else (ty if gap == 'in' else None)
        _lib.check(lib.cp_wallish_dd_box(ty.ptr(), rows, n, mf, ms, off0, off1, box.ptr(), dd.ptr() if dd else None, out.ptr() if out else None, dev.index, stream))
        calls.append((ty, box, dd, out))
    (ty, box, dd, out), second = calls
    for a, b in zip(calls[0], second):
        if a is not None:
            a.guards_intact()
            b.guards_intact()
            assert bool(synchronized(torch, (a.view.view(torch.int32 if a.view.dtype == torch.int32 else torch.int64)
                                             == b.view.view(torch.int32 if b.view.dtype == torch.int32 else torch.int64)).all())), 'two calls differ'
    if gap != 'in':
        assert same_bits(ty.host(written=False), y), 'the input was written'
    if not download:
        return dict(box=box, dd=dd, gap=out)
    return dict(box=box.host(), dd=dd.host() if dd else None, gap=out.host(written=False) if out else None)


def gap_spline(env, y, boxes):
    torch, _lib, lib, dev, stream = env
    ty, tb, out = Guarded(env, y.shape, init=y), Guarded(env, boxes.shape, init=boxes.astype('i4'), integer=True), Guarded(env, y.shape)
    _lib.check(lib.cp_gap_spline(ty.ptr(), tb.ptr(), out.ptr(), len(y), y.shape[1], dev.index, stream))
    return out.host()


def numpy_rule(g, m):
    return wt.box_rule(m, *g['margins']) + np.array(g['offsets'])


@pytest.mark.parametrize('name', wt.GROUPS)
@pytest.mark.parametrize('n', wt.SIZES)
def test_dd_box(env, n, name):
    g = wt.group(n, name)
    y, setting = g['y'], g['margins'] + g['offsets']
    finite = np.flatnonzero(g['finite'])
    others = np.flatnonzero(~g['finite'])
    base = dd_box(env, y, n, setting, True, None)
    results = {}
    for want_dd in (True, False):
        for gap in ('out', 'in'):
            got = dd_box(env, y, n, setting, want_dd, gap)
            assert np.array_equal(got['box'], base['box']), (want_dd, gap)
            assert got['dd'] is None or same_bits(got['dd'], base['dd']), (want_dd, gap)
            results[(want_dd, gap)] = got
    assert np.array_equal(dd_box(env, y, n, setting, False, None)['box'], base['box'])
    rewritten = results[(True, 'out')]['gap']
    for key, got in results.items():
        assert same_bits(got['gap'], rewritten), key
    # the finite sequences against the truth
    fails, worst_m, worst_gap = wt.judge(g, finite, m=base['dd'][finite], boxes=base['box'][finite], rewritten=rewritten[finite])
    assert not fails, [(g['labels'][r][:2], what, figure) for r, what, figure in fails[:6]]
    note('second derivatives, n = %d' % n, worst_m)
    note('rewritten box in cp_wallish_dd_box, n = %d' % n, worst_gap)
    # ... and against cp_gap_spline on the same boxes: within the sum of both allowances; outside the boxes cp_gap_spline copies the input
    separately = gap_spline(env, y, base['box'])
    for r in finite:
        inside = np.zeros(n, dtype=bool)
        if r in g['gap_ld']:
            a, b = g['boxes'][r]
            inside[a:b + 1] = True
            allowed = wt.allowance(g['gap_ld'][r][None], g['gap_f8'][r][None])[0] + wt.allowance(g['gap_ld'][r][None], g['gap_plain'][r][None])[0]
            assert np.abs(rewritten[r, inside].astype(wt.LD) - separately[r, inside].astype(wt.LD)).max() <= allowed, g['labels'][r][:2]
        assert same_bits(separately[r, ~inside], y[r, ~inside])
    # the sequences that are not finite: numpy's rule on the device's own second derivatives; the finite ones keep the bits they have without them
    for r in others:
        assert not np.isfinite(base['dd'][r]).all(), g['labels'][r][:2]
        assert tuple(base['box'][r]) == tuple(numpy_rule(g, base['dd'][r])[0]), g['labels'][r][:2]
    if len(others):
        calm = y.copy()
        calm[others] = y[finite[-1]]
        alone = dd_box(env, calm, n, setting, True, 'out')
        assert np.array_equal(alone['box'][finite], base['box'][finite]) and same_bits(alone['dd'][finite], base['dd'][finite])
        assert same_bits(alone['gap'][finite], rewritten[finite])


def expected_copies(torch, dev, short, count, scale):
    """Row i of a cyclic batch: row i % len(short) of the short launch times 2**e_i (``scale`` None: the row itself)."""
    index = torch.as_tensor(np.arange(count) % len(short), device=dev)
    rows = short[index]
    return rows if scale is None else rows * scale[:, None]


def equal_or_both_nan(torch, a, b):
    return bool(synchronized(torch, ((a == b) | (torch.isnan(a) & torch.isnan(b))).all()))


@pytest.mark.parametrize('n', wt.SIZES)
def test_dd_box_trips(env, n):
    """1, 3, 4, 5 sequences; one trip of the grid plus 5 (a second trip for two workgroups); two trips plus 1 (the prefetch in the middle of the loop)."""
    torch, dev = env[0], env[3]
    g = wt.group(n, 'm20_5')
    y, setting = g['y'], g['margins'] + g['offsets']
    counts = wt.dd_box_counts(n, cus(env))
    assert [wt.dd_box_plan(c, n, cus(env))[1] for c in counts] == [1, 1, 1, 1, 2, 3]
    short = dd_box(env, y, n, setting, True, 'out', download=False)
    for count in counts:
        batch = wt.cyclic(y, count)
        got = dd_box(env, batch, n, setting, True, 'out', download=False)
        scale = torch.as_tensor(np.ldexp(1., wt.st.exponents(count)), device=dev)
        assert bool(synchronized(torch, (got['box'].view == expected_copies(torch, dev, short['box'].view, count, None)).all())), count
        assert equal_or_both_nan(torch, got['dd'].view, expected_copies(torch, dev, short['dd'].view, count, scale)), count
        assert equal_or_both_nan(torch, got['gap'].view, expected_copies(torch, dev, short['gap'].view, count, scale)), count
        assert not bool(synchronized(torch, (got['dd'].view == CANARY).any())) and not bool(synchronized(torch, (got['box'].view == CANARY_INT).any()))


# ---- cp_wallish_tail ------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tail_plans(env):
    from test_analytic_front_bits_gpu import wallish_filter
    from cosmoprimo_amd import power as pw
    f = wallish_filter()
    ops = f._operators()
    spectrum = pw.analytic('eisenstein_hu', 'matter', f.k, bg=dict(h=np.array([0.7]), Omega_cdm=np.array([0.25]), Omega_b=np.array([0.05])), pk=dict(n_s=0.96),
                           device=env[3])
    spectrum = synchronized(env[0], spectrum).reshape(-1, f.k.size)[0]
    assert np.isfinite(spectrum).all() and (spectrum > 0).all()
    return ops, spectrum


def tail_rows(g):
    """(coef (rows, 4096), order): the sequences of a 2048-knot group two per row (CP_DST_SPLIT: the even-indexed coefficients' sequence, then the odd-indexed
    ones'); order[k] = the sequence of g at place k.  Two rows share one complex transform, so the bits of a row's d_out depend on a finite partner's data (at
    the level of rounding); a partner that is not finite is left out of the transform, which is the state of a row without a partner.  The rows are ordered
    for that: every row with a sequence that is not finite stands in front of a finite one, the rows with an invalid box first among those; and where the
    group has invalid boxes the number of rows is odd and the last row, the one without a partner, has one."""
    n = g['y'].shape[1]
    ok, others = [int(r) for r in np.flatnonzero(g['finite'])], [int(r) for r in np.flatnonzero(~g['finite'])]
    if len(others) % 2:
        others.append(ok[-1])
    if len(ok) % 2:
        ok.append(ok[-1])
    bad = [others[k:k + 2] for k in range(0, len(others), 2)]
    good = [ok[k:k + 2] for k in range(0, len(ok), 2)]
    assert len(good) >= len(bad)

    def has_invalid(pair):
        return any(not wt.valid_box(*g['boxes'][r], n) for r in pair)

    good.sort(key=lambda pair: not has_invalid(pair))
    rows = []
    for k in range(len(good)):      # (finite, not finite), (not finite, finite), ...: a finite row in either slot of the pair
        rows += ([good[k], bad[k]] if k % 2 == 0 else [bad[k], good[k]]) if k < len(bad) else [good[k]]
    if has_invalid(good[0]):
        rows += [good[0]] if len(rows) % 2 == 0 else [good[-1], good[0]]
    order = np.array(rows).reshape(-1)
    return g['y'][order].reshape(len(rows), 2 * n), order


def tail(env, plans, coef, setting, download=True):
    """cp_wallish_tail twice on fresh buffers: dict(coef, box (2 rows, 2), out)."""
    torch, _lib, lib, dev, stream = env
    ops, spectrum = plans
    mf, ms, off0, off1 = setting
    rows, npk = len(coef), spectrum.size
    pk_host = np.ascontiguousarray(np.broadcast_to(spectrum, (rows, npk)))
    calls = []
    for _ in range(2):
        tc, pk = Guarded(env, coef.shape, init=coef), Guarded(env, (rows, npk), init=pk_host)
        box, out = Guarded(env, (2 * rows, 2), integer=True), Guarded(env, (rows, npk))
        _lib.check(lib.cp_wallish_tail(ops['dst']._handle, ops['splice']._handle, tc.ptr(), pk.ptr(), npk, rows, mf, ms, off0, off1, ops['tophat'].data_ptr(), box.ptr(),
                                       out.ptr(), stream))
        calls.append((tc, pk, box, out))
    for a, b in zip(*calls):
        a.guards_intact()
        b.guards_intact()
        assert bool(synchronized(torch, (a.view.view(torch.int32 if a.view.dtype == torch.int32 else torch.int64)
                                         == b.view.view(torch.int32 if b.view.dtype == torch.int32 else torch.int64)).all())), 'two calls differ'
    tc, pk, box, out = calls[0]
    assert bool(synchronized(torch, (pk.view == torch.as_tensor(pk_host, device=dev)).all())), 'the spectrum was written'
    assert not bool(synchronized(torch, (out.view == CANARY).any())), 'elements of d_out were not written'
    if not download:
        return dict(coef=tc, box=box, out=out)
    return dict(coef=tc.host(written=False), box=box.host(), out=out.host())


@pytest.mark.parametrize('name', wt.GROUPS)
def test_tail(env, tail_plans, name):
    n = 2048
    g = wt.group(n, name)
    setting = g['margins'] + g['offsets']
    coef, order = tail_rows(g)
    rows = len(coef)
    got = tail(env, tail_plans, coef, setting)
    after = got['coef'].reshape(2 * rows, n)
    # the boxes: those of cp_wallish_dd_box on the same sequences, and the truth's
    assert np.array_equal(got['box'], dd_box(env, g['y'][order], n, setting, False, None)['box'])
    places = [k for k, r in enumerate(order) if g['finite'][r]]
    finite = order[places]
    fails, _, worst = wt.judge(g, finite, boxes=got['box'][places], rewritten=after[places])
    assert not fails, [(g['labels'][r][:2], what, figure) for r, what, figure in fails[:6]]
    note('rewritten box in cp_wallish_tail', worst)
    # Rows whose half of the packed transform stands alone -- the partner is not finite, or there is none: d_out, d_coef and d_box have the bits of the
    # same row run alone.  Those are the rows with invalid boxes (the row must still transform) and the partners of the rows that are not finite.
    bad = sorted(set(k // 2 for k, r in enumerate(order) if not g['finite'][r]))
    lonely = [row for row in range(rows) if row not in bad and ((row ^ 1) in bad or (row == rows - 1 and rows % 2 == 1))]
    assert all((row ^ 1) in lonely for row in bad)

    def invalid(row):
        return any(not wt.valid_box(*got['box'][k], n) for k in (2 * row, 2 * row + 1))

    assert any(invalid(row) for row in lonely) or all(wt.valid_box(*box, n) for box in g['boxes'][g['finite']])
    for row in lonely:
        # the first row of a pair alone is that row without a partner; the second row's half of the transform is the imaginary one, which rounds
        # differently: it stands alone behind a row of zeros, whose half of the packed spectrum is the zero a row that is not finite is replaced by
        alone = tail(env, tail_plans, coef[row:row + 1] if row % 2 == 0 else np.stack([np.zeros(2 * n), coef[row]]), setting)
        at = row % 2
        assert same_bits(alone['out'][at], got['out'][row]) and same_bits(alone['coef'][at], got['coef'][row]), (row, invalid(row))
        assert np.array_equal(alone['box'][2 * at:2 * at + 2], got['box'][2 * row:2 * row + 2]), row
    for row in bad:
        assert np.isnan(got['out'][row]).any(), row
    # (measured, not asserted: what a finite partner changes of a row's d_out)
    paired = [row for row in range(rows) if row not in bad and row not in lonely and (row ^ 1) < rows]
    if paired:
        row = paired[0]
        alone = tail(env, tail_plans, coef[row:row + 1], setting)['out'][0]
        print('MEASURED d_out of a row beside a finite partner against the row alone: largest relative difference %.3g' % float(np.abs(alone / got['out'][row] - 1.).max()))


def test_tail_trips(env, tail_plans):
    """1, 3, 4, 5 rows; one trip of the grid plus 5 rows; two trips plus 1: the odd counts end on a row without a partner."""
    torch, dev = env[0], env[3]
    n = 2048
    g = wt.group(n, 'm20_5')
    setting = g['margins'] + g['offsets']
    coef, order = tail_rows(g)
    counts = wt.tail_counts(cus(env))
    assert [wt.tail_plan(c, cus(env))[1] for c in counts] == [1, 1, 1, 1, 2, 3]
    short = tail(env, tail_plans, coef, setting, download=False)
    short_box = short['box'].view.view(len(coef), 4)
    for count in counts:
        got = tail(env, tail_plans, wt.cyclic(coef, count), setting, download=False)
        scale = torch.as_tensor(np.ldexp(1., wt.st.exponents(count)), device=dev)
        assert bool(synchronized(torch, (got['box'].view.view(count, 4) == expected_copies(torch, dev, short_box, count, None)).all())), count
        assert equal_or_both_nan(torch, got['coef'].view, expected_copies(torch, dev, short['coef'].view, count, scale)), count
        assert not bool(synchronized(torch, (got['box'].view == CANARY_INT).any()))
