"""GPU: the results of the two kernels that run the segmented spline elimination of csrc/cp_spline_sweeps.h -- ``spline_rows_kernel<R>``
(csrc/cp_spline_rows.hip; ``SplineRows``) and ``splice_kernel`` (csrc/cp_bao.hip; ``SplicedClampedSpline`` under scheme 0) -- bit for bit, against
tests/golden/spline_sweep_bits.npz: what the library gave while both sweeps were written out in either kernel and the plans' factors, halo search and
query weights in either plan (recorded on an MI355X by tools/gen_spline_sweep_bits.py, every call run twice there and refused if its two runs
differed).  The sweeps' arithmetic is explicit ``fma`` and single operations and the plans' is plain host C++, so equal source arithmetic gives equal
bits whatever the schedule: every output must be EQUAL.  A tolerance would not see a ``wave_lds_phase`` moved past a neighbour's read.

The inputs come from the case builders of tests/spline_truth.py and tests/splice_truth.py, so the file holds outputs only: SHA-256 digests (32 bytes)
and the names and shapes of the entries they belong to -- one digest per output row, one per 64 rows for an entry of more than 256 rows; a mismatch
names its entry and its first rows.  The cases are the smallest that reach every branch of the shared text:
  SplineRows at 9 knots (S = 1, the halo as long as the row), 433 (R = 2) and 1633 (R = 1): the three end conditions; the families uniform and
    saw2x40 where ``spline_truth.rows_used`` takes them; 23 rows (the last group of a wave partly dead); values plain and with root, scale and the
    grouped store, ``second_derivatives``, ``pairs=True``;
  the window (1000, 300, 400), which ends inside the row on both sides; the trip ('uniform', 432, 8203, 13): more rows than the grid takes at once;
  one NaN row among 23 at 433 knots;
  SplicedClampedSpline forced to scheme 0: ``irregular_case`` at 4, 65 and 700 knots (saw2x40, geom1.05), 193 knots spliced from PIECES['three'],
    ``stretch_inputs('generic60')`` (the constant slot of the stretch) with and without tophat, 11 rows each; 4 x CUs + 5 rows at 65 knots, and at
    the largest plan of saw1.5x16 (one workgroup per CU: a wave takes a second row); one NaN row among 11 at 65 knots."""
import hashlib
import os

import numpy as np
import pytest

import splice_truth as sp
import spline_truth as st

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'spline_sweep_bits.npz')
ROWS_SIZES = [9, 433, 1633]
ROWS_FAMILIES = ['uniform', 'saw2x40']
NROWS = 23            # 23 mod 4 = 3, 23 mod 2 = 1
WINDOW = (1000, 300, 400)
TRIP = ('uniform', 432, 8203, 13)
SCALE = 0.3
SPLICE_ROWS = 11
SPLICE_IRREGULAR = [(name, n) for name in ('saw2x40', 'geom1.05') for n in (4, 65, 700)]
BLOCK = 64            # rows per digest of an entry of more than 256 rows


def _device():
    import torch
    return torch.device('cuda', 0)


def _up(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array), device=_device())


def _host(x):
    import torch
    torch.cuda.synchronize()
    return np.ascontiguousarray(x.cpu().numpy())


def _blocks(value):
    rows = np.ascontiguousarray(value).reshape(-1, value.shape[-1])
    step = BLOCK if len(rows) > 256 else 1
    return [rows[i:i + step] for i in range(0, len(rows), step)]


def digests(entries):
    """(labels 'name shape dtype', (blocks, 32) uint8: the SHA-256 of every row -- the last axis; of every 64 rows where an entry has more than 256 --
    of every entry, in the order of the names)."""
    names = sorted(entries)
    labels = np.array(['%s %s %s' % (name, entries[name].shape, entries[name].dtype) for name in names])
    found = [hashlib.sha256(block.tobytes()).digest() for name in names for block in _blocks(entries[name])]
    return labels, np.frombuffer(b''.join(found), dtype='u1').reshape(-1, 32)


def assert_equal_rows(got, recorded, group):
    labels, rows = digests(got)
    assert list(labels) == list(recorded[group + '.entries']) and rows.shape == recorded[group].shape
    offset = 0
    for label, name in zip(labels, sorted(got)):
        count = len(_blocks(got[name]))
        differ = np.flatnonzero((rows[offset:offset + count] != recorded[group][offset:offset + count]).any(axis=1))
        assert differ.size == 0, '%s: %s: digests %s differ' % (group, label, differ[:8])
        offset += count


def _rows_outputs(out, tag, op, y, group, values=True, m=True):
    """values plain and rooted, scaled and grouped (stored back row by row), second derivatives, pairs."""
    nrows, n = y.shape
    if values:
        out[tag + '.values'] = _host(op(y))
        rooted = op(y.reshape(nrows // group, group, n), sqrt=True, scale=SCALE, last_axis_first=True)
        out[tag + '.rooted'] = _host(rooted.transpose(-1, -2).reshape(nrows, -1))
    if m:
        out[tag + '.m'] = _host(op.second_derivatives(y))
        out[tag + '.pairs'] = _host(op.second_derivatives(y, pairs=True)).reshape(nrows, -1)


def rows_entries(n):
    from cosmoprimo_amd.spline import SplineRows
    dev, out = _device(), {}
    for bc in st.BCS:
        for name in ROWS_FAMILIES:
            values, m = st.rows_used(name, n, bc, 'values'), st.rows_used(name, n, bc, 'm')
            if not (values or m):
                continue
            case = st.rows_case(name, n, bc)
            op = SplineRows(case['x'], st.rows_queries(case['x']), bc=bc, device=dev)
            assert op.window[:2] == (0, n) and op.window[2] == {9: 4, 433: 2, 1633: 1}[n]
            _rows_outputs(out, '%s.%s' % (bc, name), op, _up(st.batch(case['y'], NROWS)), NROWS, values, m)
    return out


def rows_window_entries():
    from cosmoprimo_amd.spline import SplineRows
    dev, out = _device(), {}
    n, first, last = WINDOW
    for bc in st.BCS:
        for name in ROWS_FAMILIES:
            if not st.rows_used(name, n, bc, 'values'):
                continue
            case = st.rows_case(name, n, bc)
            op = SplineRows(case['x'], st.rows_queries(case['x'], first, last), bc=bc, device=dev)
            assert op.window[0] > 0 and op.window[0] + op.window[1] < n
            _rows_outputs(out, '%s.%s' % (bc, name), op, _up(st.batch(case['y'], NROWS)), NROWS, m=False)
    return out


def rows_trip_entries():
    from cosmoprimo_amd.spline import SplineRows
    dev, out = _device(), {}
    name, n, nrows, group = TRIP
    case = st.rows_case(name, n, 'natural')
    x = case['x']
    xq = np.unique(np.concatenate([x[:2], st.rows_queries(x)[::17], x[-2:]]))
    op = SplineRows(x, xq, bc='natural', device=dev)
    assert op.window[2] == 4
    _rows_outputs(out, 'trip', op, _up(st.batch(case['y'], nrows)), group)
    return out


def rows_nan_entries():
    from cosmoprimo_amd.spline import SplineRows
    dev, out = _device(), {}
    case = st.rows_case('uniform', 433, 'natural')
    op = SplineRows(case['x'], st.rows_queries(case['x']), bc='natural', device=dev)
    y = st.batch(case['y'], NROWS)
    y[5, 433 // 2] = np.nan
    _rows_outputs(out, 'nan', op, _up(y), NROWS)
    return out


def _splice(knots, pieces, xq):
    from cosmoprimo_amd.spline import SplicedClampedSpline
    op = SplicedClampedSpline(knots, pieces, xq, device=_device())
    op.scheme = 0
    assert op.scheme == 0
    return op


def _splice_rows(case, nrows, spoil=None):
    rows = [None if r is None else st.batch(r, nrows) for r in case['rows']]
    if spoil is not None:
        rows[0][spoil] = np.nan
    return [None if r is None else _up(r) for r in rows]


def splice_entries():
    out = {}
    for name, n in SPLICE_IRREGULAR:
        case = sp.irregular_case(name, n)
        op = _splice(case['x'], case['pieces'], case['xq'])
        out['%s.%d' % (name, n)] = _host(op(*_splice_rows(case, SPLICE_ROWS)))
    case = sp.irregular_case('jitter100', 193, 'three')
    out['three.193'] = _host(_splice(case['x'], case['pieces'], case['xq'])(*_splice_rows(case, SPLICE_ROWS)))
    case = sp.stretch_inputs('generic60')
    assert case['plan']['ntab_left'] < case['plan']['uniform_end'] < case['plan']['n']      # the stretch has its one slot
    op = _splice(case['knots'], case['pieces'], case['xq'])
    rows0, rows1 = (_up(st.batch(case[key], SPLICE_ROWS)) for key in ('rows0', 'rows1'))
    out['generic60'] = _host(op(rows0, rows1))
    out['generic60.tophat'] = _host(op(rows0, rows1, tophat=_up(case['tophat'])))
    case = sp.irregular_case('saw2x40', 65)
    out['nan.65'] = _host(_splice(case['x'], case['pieces'], case['xq'])(*_splice_rows(case, SPLICE_ROWS, spoil=(5, 31))))
    return out


def splice_batch_entries():
    import torch
    cus = torch.cuda.get_device_properties(_device()).multi_processor_count
    nrows, out = 4 * cus + 5, {}
    name = 'saw1.5x16'
    for label, case in (('65', sp.irregular_case('saw2x40', 65)), ('largest', sp.irregular_case(name, sp.largest_irregular(name)))):
        op = _splice(case['x'], case['pieces'], case['xq'])
        assert label == '65' or op.layout['lds_bytes'] > 80 * 1024      # one workgroup of four waves per CU: fewer waves than rows
        out[label] = _host(op(*_splice_rows(case, nrows)))
    return out


def groups():
    """[(group, call)]: what tools/gen_spline_sweep_bits.py records and the tests below compare."""
    return [('rows%d' % n, lambda n=n: rows_entries(n)) for n in ROWS_SIZES] + [('rows_window', rows_window_entries), ('rows_trip', rows_trip_entries),
                                                                                 ('rows_nan', rows_nan_entries), ('splice', splice_entries),
                                                                                 ('splice_batch', splice_batch_entries)]


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize('n', ROWS_SIZES)
def test_spline_rows(recorded, n):
    assert_equal_rows(rows_entries(n), recorded, 'rows%d' % n)


def test_spline_rows_window(recorded):
    assert_equal_rows(rows_window_entries(), recorded, 'rows_window')


def test_spline_rows_trip(recorded):
    assert_equal_rows(rows_trip_entries(), recorded, 'rows_trip')


def test_spline_rows_nan_row(recorded):
    assert_equal_rows(rows_nan_entries(), recorded, 'rows_nan')


def test_splice(recorded):
    assert_equal_rows(splice_entries(), recorded, 'splice')


def test_splice_batches(recorded):
    assert_equal_rows(splice_batch_entries(), recorded, 'splice_batch')
