"""GPU: ``brieden_resample_kernel<S, PEAKS, OPLDS>`` (csrc/cp_bao.hip) through both of its entry points, cp_brieden_resample and cp_brieden_smooth, against
the longdouble truth of tests/brieden_truth.py -- the samples, their log10, the four knots of ``_pad_log`` and a full natural-spline solve, no lanes and
no closed forms -- at the shapes where the kernel's pieces meet:
(a) every S = 3 .. 8 with the last lane full, owning one knot or straddling the last knot (n = 129 .. 512), rescales of 1 exactly, 1 +- 1e-9, 0.85, 1.2
    and between, the k_fid range in the middle, at the start and at the end of the rows, ``out`` aliasing ``pk``;
(b) extrapolation bounds inside the k_fid range (the second argument of fmin / fmax);
(c) batches of 1 .. 13 cosmologies and more than one launch has waves (12 x CUs + 5);
(d) cp_brieden_smooth with 1 .. 64 extrema, odd and even, extrema at knot 0 and n - 1, the operator's columns in LDS (768 threads) and not;
(e) a log_k_fid that is not uniform: NaN over the k_fid range of every row and nothing else, at S = 5 and S = 7; the sizes either side of the kernel.
Tolerance: the rule of tests/spline_truth.py in v = log10(out), 16 levels of the worse of two float64 results per row (tests/brieden_truth.py); each test
prints the largest fraction it used.  S and the OPLDS form follow from (n, np) by the launch code's own formulas, restated in brieden_truth and held to
what the cases claim by tests/test_brieden_truth_host.py.
Measured on an MI355X, largest fraction of the allowance used: cp_brieden_resample 0.400 (257 samples at the start of the rows; levels up to 21.7 FLOOR), cp_brieden_smooth
0.616 with the operator read from memory (512 samples, 23 extrema, 3077 cosmologies) and 0.313 with it in LDS (256 samples, 2 extrema).
"""
import numpy as np
import pytest

import brieden_truth as bt

pytestmark = pytest.mark.gpu


def _env():
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    dev = torch.device('cuda', 0)
    return torch, _lib, _lib.load(), dev, dv.stream_of(dev)


def _up(a, dtype='f8'):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=torch.device('cuda', 0))


def _resample(case, nb, alias=False, log_k_fid=None):
    """cp_brieden_resample on a batch of nb rows of the case: (out (nb, nk), pk (nb, nk)) as numpy."""
    torch, _lib, lib, dev, stream = _env()
    base, which, _ = bt.rows_of(nb)
    n, nk, first = case['n'], case['nk'], case['first']
    pk = bt.rest_of_the_rows(nb, nk)
    d_pk = _up(pk)
    out = d_pk if alias else torch.full((nb, nk), -1., dtype=torch.float64, device=dev)
    args = [_up(case['envelope'][base]), _up(case['pknow'][base]), _up(case['ratio_now_fid']), _up(case['k_fid']),
            _up(case['log_k_fid'] if log_k_fid is None else log_k_fid), _up(case['rescale'][which])]
    _lib.check(lib.cp_brieden_resample(*[a.data_ptr() for a in args], case['bounds'][0], case['bounds'][1], d_pk.data_ptr(), out.data_ptr(), nb, n, nk, first, 0, stream))
    return out.cpu().numpy(), pk


def _smooth(case, nb, alias=False, log_k_fid=None):
    torch, _lib, lib, dev, stream = _env()
    base, which, _ = bt.rows_of(nb)
    n, nk, first = case['n'], case['nk'], case['first']
    pk = bt.rest_of_the_rows(nb, nk)
    d_pk = _up(pk)
    out = d_pk if alias else torch.full((nb, nk), -1., dtype=torch.float64, device=dev)
    args = [_up(case['pk_peaks'][base]), _up(case['now'][base]), _up(case['g0'][base]), _up(case['correction']), _up(case['ratio_fid']), _up(case['peaks'], 'i4'),
            _up(case['op'])]
    more = [_up(case['ratio_now_fid']), _up(case['k_fid']), _up(case['log_k_fid'] if log_k_fid is None else log_k_fid), _up(case['rescale'][which])]
    _lib.check(lib.cp_brieden_smooth(*[a.data_ptr() for a in args], case['np'], *[a.data_ptr() for a in more], case['bounds'][0], case['bounds'][1], d_pk.data_ptr(),
                                     out.data_ptr(), nb, n, nk, first, 0, stream))
    return out.cpu().numpy(), pk


def _check(out, pk, case, what):
    """The k_fid range against the truth, the rest of the rows bit for bit; rows of rescale 1: the samples themselves."""
    first, n = case['first'], case['n']
    assert np.array_equal(out[:, :first], pk[:, :first]) and np.array_equal(out[:, first + n:], pk[:, first + n:]), what
    assert np.isfinite(out).all() and (out[:, first:first + n] > 0.).all(), what
    worst = bt.assert_within(out, case, what)
    unique = bt.rows_of(len(out))[2]
    on_knots = case['row_rescale'][unique] == 1.
    np.testing.assert_allclose(out[on_knots, first:first + n], case['samples'][unique][on_knots], rtol=2e-14)
    return worst


@pytest.mark.parametrize('n', bt.SIZES)
def test_resample_sizes(n):
    case = bt.resample_case(n)
    out, pk = _resample(case, bt.NB)
    worst = _check(out, pk, case, 'cp_brieden_resample %d samples (S = %d, last lane %s)' % (n, bt.samples_per_lane(n), bt.last_lane(n)))
    aliased, pk = _resample(case, bt.NB, alias=True)
    assert np.array_equal(aliased, out)
    print('sizes, %d samples: largest fraction %.3g' % (n, worst))


@pytest.mark.parametrize('first', ['zero', 'end'])
@pytest.mark.parametrize('n', [191, 257, 512])
def test_resample_at_the_ends_of_the_rows(n, first):
    worst = 0.
    for bounds in ((bt.KMIN, bt.KMAX), bt.TIGHT):
        case = bt.resample_case(n, first, bounds)
        out, pk = _resample(case, bt.NB)
        worst = max(worst, _check(out, pk, case, 'cp_brieden_resample %d samples, first %d, bounds %s' % (n, case['first'], bounds)))
        aliased, pk = _resample(case, bt.NB, alias=True)
        assert np.array_equal(aliased, out)
    print('ends of the rows, %d samples, %s: largest fraction %.3g' % (n, first, worst))


def test_resample_batches():
    torch, _lib, lib, dev, stream = _env()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    worst = 0.
    for n in (193, 511):      # a lane that owns one knot, a lane that straddles
        case = bt.resample_case(n)
        for nb in bt.BATCHES + [12 * cus + 5]:
            out, pk = _resample(case, nb)
            worst = max(worst, _check(out, pk, case, 'cp_brieden_resample %d samples, %d cosmologies' % (n, nb)))
    print('batches: largest fraction %.3g' % worst)


@pytest.mark.parametrize('n,npk', bt.SMOOTH)
def test_smooth(n, npk):
    torch, _lib, lib, dev, stream = _env()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    case = bt.smooth_case(n, npk)
    form = 'operator in LDS' if bt.oplds(n, npk)[0] else 'operator from memory'
    worst = 0.
    for nb in ([bt.NB, 1, 12 * cus + 5] if (n, npk) in ((512, 23), (129, 64)) else [bt.NB]):
        out, pk = _smooth(case, nb)
        worst = max(worst, _check(out, pk, case, 'cp_brieden_smooth %d samples, %d extrema (%s), %d cosmologies' % (n, npk, form, nb)))
    aliased, pk = _smooth(case, bt.NB, alias=True)
    assert np.array_equal(aliased, _smooth(case, bt.NB)[0])
    print('smooth, %d samples, %d extrema (%s): largest fraction %.3g' % (n, npk, form, worst))


@pytest.mark.parametrize('n', bt.BENT)
def test_a_bent_log_k_fid_gives_nan_over_its_range(n):
    npk = 24
    for case, run in ((bt.resample_case(n), _resample), (bt.smooth_case(n, npk), _smooth)):
        first = case['first']
        bent = case['log_k_fid'].copy()
        bent[n // 2] += 1e-3 * (bent[1] - bent[0])
        out, pk = run(case, bt.NB, log_k_fid=bent)
        assert np.isnan(out[:, first:first + n]).all() and np.array_equal(out[:, :first], pk[:, :first]) and np.array_equal(out[:, first + n:], pk[:, first + n:])
        straight, pk = run(case, bt.NB)      # and the same arrays with the grid as it was
        _check(straight, pk, case, 'after the bent grid, %d samples' % n)


def test_sizes_either_side_of_the_kernel():
    torch, _lib, lib, dev, stream = _env()
    buf = torch.ones(64 * 1024, dtype=torch.float64, device=dev)
    idx = torch.zeros(64, dtype=torch.int32, device=dev)
    p = buf.data_ptr()
    for n in bt.UNSUPPORTED:
        assert lib.cp_brieden_resample(p, p, p, p, p, p, bt.KMIN, bt.KMAX, p, p, 1, n, n + 300, 137, 0, stream) == _lib.CP_EUNSUPPORTED
        assert lib.cp_brieden_smooth(p, p, p, p, p, idx.data_ptr(), p, 23, p, p, p, p, bt.KMIN, bt.KMAX, p, p, 1, n, n + 300, 137, 0, stream) == _lib.CP_EUNSUPPORTED
    torch.cuda.synchronize(dev)
