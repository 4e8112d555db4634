"""GPU: the results of the kernels that run the uniform-grid spline recursions of csrc/cp_uniform_recursions.h -- ``splice_uniform_kernel<S>``
(csrc/cp_splice_uniform.h; ``SplicedClampedSpline`` under scheme 1), ``wallish_dd_box_kernel<32>`` and ``brieden_resample_kernel<S, PEAKS, OPLDS>``
(csrc/cp_bao.hip) -- and of the two that read the shared arg-max merge, ``wallish_dd_box_kernel<16>`` and ``wallish_box_kernel`` (csrc/cp_spline.hip),
bit for bit, against tests/golden/uniform_recursion_bits.npz: what the library gave while the recursions, the carries, the wave shifts and the merge
were written out at every site (recorded on an MI355X by tools/gen_uniform_recursion_bits.py, every call run twice there and refused if its two runs
differed).  The recursions are explicit ``fma`` and single operations, so equal source arithmetic gives equal bits whatever the schedule: every output
must be EQUAL.  A tolerance would not see the carries added in the other order, or a ``-0`` carry turned into ``+0``.  (cp_wallish_tail, cp_wallish_full
and cp_dst_forward_analytic_box, which run the same text, are pinned by tests/test_row_transform_bits_gpu.py.)

The inputs come from the case builders of tests/splice_truth.py, tests/spline_truth.py and tests/brieden_truth.py, so the file holds outputs only:
SHA-256 digests and the names and shapes of the entries (tests/test_spline_sweep_bits_gpu.py: ``digests``).  The cases are the smallest that reach every
branch of the shared text:
  SplicedClampedSpline, scheme 1: the stretch of 64 S knots for every S = 33 .. 57 of ``splice_truth.UNIFORM_S``, with and without tophat, 5 rows (a
    second workgroup with one live wave); at S = 33 also 4 x CUs + 5 rows (a wave takes a second row through the prefetch) and one NaN row among 5;
  cp_wallish_dd_box at 2048 coefficients, margins (20, 5), offsets (-10, 20): 5 sequences with ``dd`` and ``gap`` absent or present and ``gap`` in
    place; a sequence that holds a NaN (the general arg-max walk) and one with an exact tie of its maximum; 4 x CUs + 5 sequences;
  cp_wallish_dd_box at 1024 coefficients (the elimination, which reads the shared merge): the 5 sequences with the NaN and the tie;
  cp_wallish_box: five columns of 2048 with a NaN column and a tie;
  cp_brieden_resample at n = 129 .. 449 (S = 3 .. 8) and at 192 and 512 (the last lane exactly full), cp_brieden_smooth at ``brieden_truth.SMOOTH``
    (the operator in LDS and from memory, at the smallest and the largest S): 13 cosmologies each."""
import os

import numpy as np
import pytest

import brieden_truth as bt
import splice_truth as sp
import spline_truth as st
from test_brieden_edges_gpu import _resample, _smooth
from test_spline_sweep_bits_gpu import assert_equal_rows, digests  # noqa: F401 (digests: tools/gen_uniform_recursion_bits.py)

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'uniform_recursion_bits.npz')
SPLICE_ROWS = 5
SEQUENCES = 5
MARGINS, OFFSETS = (20, 5), (-10, 20)
NAN_AT, TIE_ROW, NAN_ROW = 100, 3, 1
RESAMPLE_SIZES = [129, 193, 257, 321, 385, 449, 192, 512]


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


def _cus():
    import torch
    return torch.cuda.get_device_properties(_device()).multi_processor_count


# ---- SplicedClampedSpline under the uniform scheme ----------------------------------------------------------------------------------------------

def _uniform(case, S):
    from cosmoprimo_amd.spline import SplicedClampedSpline
    op = SplicedClampedSpline(case['knots'], case['pieces'], case['xq'], device=_device())
    assert op.scheme == 1 and op.layout['uniform']['S'] == S
    return op


def splice_entries(S):
    case = sp.stretch_inputs('nm%d' % sp.UNIFORM_S[S][0])
    op, out = _uniform(case, S), {}
    rows0, rows1 = (st.batch(case[key], SPLICE_ROWS) for key in ('rows0', 'rows1'))
    out['plain'] = _host(op(_up(rows0), _up(rows1)))
    out['tophat'] = _host(op(_up(rows0), _up(rows1), tophat=_up(case['tophat'])))
    if S == 33:
        nrows = 4 * _cus() + 5
        many0, many1 = (_up(st.batch(case[key], nrows)) for key in ('rows0', 'rows1'))
        out['many'] = _host(op(many0, many1, tophat=_up(case['tophat'])))
        rows1 = rows1.copy()
        rows1[2, sp.SPARE[0] + 1000] = np.nan      # a knot of the stretch
        out['nan'] = _host(op(_up(rows0), _up(rows1), tophat=_up(case['tophat'])))
    return out


# ---- the boxes of wallish2018 ---------------------------------------------------------------------------------------------------------------------

def sequences(n, nseq=SEQUENCES, special=True):
    """(nseq, n): the DST-like rows of ``spline_truth.gap_rows``; ``special``: row 1 holds a NaN, row 3 is two equal bumps at the same place of two
    lanes' segments (of 16 and of 32 knots) with zeros around them: the same arithmetic on the same values, an exact tie of the maximum."""
    y = st.batch(st.gap_rows(n), nseq)
    if special:
        y[NAN_ROW, NAN_AT] = np.nan
        bump = 3e-3 * np.exp(-0.5 * (np.arange(-8, 9) / 3.)**2) * (1. + 0.05 * np.arange(17))      # (lopsided: one maximum per bump)
        y[TIE_ROW] = 0.
        for centre in (32 * 10 + 7, 32 * 25 + 7):
            y[TIE_ROW, centre - 8:centre + 9] = bump
    return y


def _dd_box(y, with_dd, gap):
    """cp_wallish_dd_box on y (nseq, n); gap: None, 'out' or 'inplace'.  {box, dd, gap} as far as asked for."""
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    dev = _device()
    ty = _up(y)
    nseq, n = y.shape
    box = torch.empty((nseq, 2), dtype=torch.int32, device=dev)
    dd = torch.empty_like(ty) if with_dd else None
    filled = ty if gap == 'inplace' else (ty.clone() if gap == 'out' else None)
    _lib.check(_lib.load().cp_wallish_dd_box(ty.data_ptr(), nseq, n, *MARGINS, *OFFSETS, box.data_ptr(), dd.data_ptr() if with_dd else None,
                                             filled.data_ptr() if gap else None, 0, dv.stream_of(dev)))
    out = {'box': _host(box)}
    if with_dd:
        out['dd'] = _host(dd)
    if gap:
        out['gap'] = _host(filled)
    return out


def _tagged(out, tag, entries):
    out.update({'%s.%s' % (tag, key): value for key, value in entries.items()})


def dd_box_entries(n):
    out = {}
    if n == 2048:
        plain = sequences(n, special=False)
        for with_dd in (False, True):
            for gap in (None, 'out', 'inplace'):
                _tagged(out, 'dd%d.%s' % (with_dd, gap), _dd_box(plain, with_dd, gap))
        _tagged(out, 'many', _dd_box(sequences(n, 4 * _cus() + 5), True, 'out'))
    special = _dd_box(sequences(n), True, 'out')
    first = special['box'][TIE_ROW, 0] - OFFSETS[0]
    dd = special['dd'][TIE_ROW]
    assert dd[first] == dd[MARGINS[0]:n - MARGINS[0]].max() and (dd == dd[first]).sum() == 2 and first == np.flatnonzero(dd == dd[first])[0]      # the tie is one
    assert np.isnan(special['dd'][NAN_ROW]).any()
    _tagged(out, 'special', special)
    return out


def box_entries():
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    dev, n = _device(), 2048
    dd = np.random.default_rng(2048).normal(size=(SEQUENCES, n))
    dd[NAN_ROW, NAN_AT] = np.nan
    dd[TIE_ROW, 300] = dd[TIE_ROW, 900] = 10.
    t = _up(dd)
    box = torch.empty((SEQUENCES, 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.load().cp_wallish_box(t.data_ptr(), SEQUENCES, n, *MARGINS, *OFFSETS, box.data_ptr(), 0, dv.stream_of(dev)))
    return {'box': _host(box)}


# ---- brieden2022 --------------------------------------------------------------------------------------------------------------------------------------

def resample_entries(n):
    assert bt.samples_per_lane(n) == {129: 3, 192: 3, 193: 4, 257: 5, 321: 6, 385: 7, 449: 8, 512: 8}[n]
    return {'out': _resample(bt.resample_case(n), bt.NB)[0]}


def smooth_entries(n, npk):
    return {'out': _smooth(bt.smooth_case(n, npk), bt.NB)[0]}


def groups():
    """[(group, call)]: what tools/gen_uniform_recursion_bits.py records and the tests below compare."""
    assert {bt.oplds(n, npk)[0] for n, npk in bt.SMOOTH} == {False, True}
    return ([('splice%d' % S, lambda S=S: splice_entries(S)) for S in sp.UNIFORM_S] + [('dd_box%d' % n, lambda n=n: dd_box_entries(n)) for n in (2048, 1024)]
            + [('box', box_entries)] + [('resample%d' % n, lambda n=n: resample_entries(n)) for n in RESAMPLE_SIZES]
            + [('smooth%d_%d' % pair, lambda pair=pair: smooth_entries(*pair)) for pair in bt.SMOOTH])


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


@pytest.mark.parametrize('S', list(sp.UNIFORM_S))
def test_splice_uniform(recorded, S):
    assert_equal_rows(splice_entries(S), recorded, 'splice%d' % S)


@pytest.mark.parametrize('n', [2048, 1024])
def test_wallish_dd_box(recorded, n):
    assert_equal_rows(dd_box_entries(n), recorded, 'dd_box%d' % n)


def test_wallish_box(recorded):
    assert_equal_rows(box_entries(), recorded, 'box')


@pytest.mark.parametrize('n', RESAMPLE_SIZES)
def test_brieden_resample(recorded, n):
    assert_equal_rows(resample_entries(n), recorded, 'resample%d' % n)


@pytest.mark.parametrize('n,npk', bt.SMOOTH)
def test_brieden_smooth(recorded, n, npk):
    assert_equal_rows(smooth_entries(n, npk), recorded, 'smooth%d_%d' % (n, npk))
