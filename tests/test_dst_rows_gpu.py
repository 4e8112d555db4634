"""GPU: the batched DST-II / DST-III (cp_dst_execute, ``dst_kernel`` of csrc/cp_dst.hip) against an extended-precision truth, with more pairs of rows
than workgroups: the kernel transforms two rows per trip, fetches the next pair's rows while it works on this one, resets its flags for rows that are
not finite in LDS at the top of every trip and, on the way back, stages the pair in the LDS of the FFT -- none of which another test makes it do twice
in one workgroup.

Truth and rows: tests/transform_truth.py (the direct sum in longdouble of seven base rows per length; row i of a batch is base row i % 7 times
2^e_i, e_i in [-300, 300], and so is its truth -- batch and expected values are formed on the device).  The fused maps log(k x) / exp(y) / k are not
linear: their rows are the seven base rows repeated, unscaled.
Bounds: the project's own for these kernels (tests/test_dst_gpu.py, test_dst_roundtrip_and_scipy): per row |got - truth|.max() < 1e-13 |truth|.max();
fused inverse |got / truth - 1|.max() < 1e-12; the split layout holds the same numbers, bit for bit.

The two rows of a pair share one complex FFT, whose rounding errors are relative to the larger of the two spectra: the hardest pair is the unit impulse
(rows 3 mod 7), whose transform nowhere exceeds sqrt(2 / n), next to the constant row, whose transform peaks at 0.6 sqrt(n) of its samples.  The kernel
brings the two rows' largest samples and then their 2-norms -- the size of their spectra -- to the same power of two before they meet.

Every mode is held to the project's bound (LIMITS = 1).  The fractions of the bound that the kernel takes, per length and direction, have not been
recorded for the kernel as it is: every test prints its own (pytest -rA).
"""
import functools

import numpy as np
import pytest

import transform_truth as tt

pytestmark = pytest.mark.gpu

G = 512      # pairs of rows: the grid cap of cp_dst_execute, ``const int grid = (int)(npairs < 512 ? npairs : 512);`` (csrc/cp_dst.hip)
LENGTHS = [256, 1024, 4096]
# 2 G + 1: 513 pairs, the last row without a partner is workgroup 0's second trip; 4 G + 3: 1026 pairs, workgroups 0 and 1 make three trips, the
# row without a partner is workgroup 1's third
ROW_COUNTS = [2 * G + 1, 4 * G + 3]
LD = tt.LD


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device='cuda:0')


def kx_of(n):
    return np.linspace(1e-7, 2., n)


@functools.lru_cache(maxsize=None)
def truths(n):
    """Seven base rows, their DST-II and their DST-III as (hi, lo) pairs of doubles, on the device."""
    x = tt.base_rows(n, 'real')
    return {'x': dev(x), 'forward': tuple(map(dev, tt.split_double(tt.dst2_truth(x)))), 'inverse': tuple(map(dev, tt.split_double(tt.idst2_truth(x))))}


@functools.lru_cache(maxsize=None)
def fused_truths(n):
    """The filter's maps around the transform: forward dst(log(k p)) of p = exp(0.1 normal) / k, the logarithm in longdouble; inverse exp(idst(y)) / k
    of y = the forward truth rounded to double."""
    k = kx_of(n)
    p = np.exp(0.1 * np.random.default_rng(77 + n).standard_normal((tt.NBASE, n))) / k
    forward = tt.dst2_truth(np.log(k.astype(LD) * p.astype(LD)))
    y = forward.astype('f8')
    inverse = np.exp(tt.idst2_truth(y)) / k.astype(LD)
    return {'p': dev(p), 'y': dev(y), 'forward': tuple(map(dev, tt.split_double(forward))), 'inverse': tuple(map(dev, tt.split_double(inverse)))}


def to_split(y):
    """[Y_0, Y_2, ... | Y_1, Y_3, ...]: the de-interleaved layout of the coefficients."""
    import torch
    return torch.cat([y[:, 0::2], y[:, 1::2]], dim=1).contiguous()


LIMITS = {'plain': 1., 'fused forward': 1., 'fused inverse': 1.}      # of the bound, see above


def fractions(got, truth, nrows, scaled, relative=False):
    """Per row, the fraction of its bound that the error takes: 1e-13 of the row's largest |truth|, or (``relative``) 1e-12 of each value."""
    hi, lo = (tt.batch(part, nrows, scaled) for part in truth)
    assert got.shape == hi.shape and got.dtype == hi.dtype
    error = ((got - hi) - lo).abs()
    if relative:
        return ((error / hi.abs()).amax(dim=1) / 1e-12).cpu().numpy()
    return (error.amax(dim=1) / (1e-13 * hi.abs().amax(dim=1))).cpu().numpy()


def check_rows(name, got, truth, nrows, n, scaled=True, relative=False, bad=(), limit='plain'):
    """Rows ``bad`` hold nothing but NaN, every other row meets the bound (and is therefore finite)."""
    import torch
    nan_rows = torch.isnan(got).all(dim=1).cpu().numpy()
    frac = fractions(got, truth, nrows, scaled, relative)
    good = np.ones(nrows, dtype=bool)
    good[list(bad)] = False
    assert good.sum() == nrows - len(bad)
    masked = np.where(good, frac, 0.)
    worst = float(np.nanmax(masked))
    print('dst %s n %d rows %d: %.3g of the bound (row %d)' % (name, n, nrows, worst, int(np.nanargmax(masked))))
    for i in bad:
        assert nan_rows[i], '%s n %d: row %d holds %d numbers that are not NaN' % (name, n, i, int((~torch.isnan(got[i])).sum()))
    assert np.flatnonzero(nan_rows).tolist() == sorted(bad)
    failing = np.flatnonzero(good & ~(frac < LIMITS[limit]))
    assert failing.size == 0, '%s n %d: rows %s (workgroups %s, trips %s) at %s of the bound' % (
        name, n, failing[:8].tolist(), (failing[:8] // 2 % G).tolist(), (failing[:8] // (2 * G)).tolist(), frac[failing[:8]].tolist())
    return frac


@pytest.mark.parametrize('nrows', ROW_COUNTS)
@pytest.mark.parametrize('n', LENGTHS)
def test_scaled_batches(n, nrows):
    """Plain and split layout, forward and inverse."""
    import torch
    from cosmoprimo_amd.dst import DST
    plan, t = DST(n), truths(n)
    x = tt.batch(t['x'], nrows)
    y = plan(x)
    check_rows('forward', y, t['forward'], nrows, n)
    assert torch.equal(plan(x, split=True), to_split(y))
    back = plan(x, inverse=True)
    check_rows('inverse', back, t['inverse'], nrows, n)
    assert torch.equal(plan(to_split(x), inverse=True, split=True), back)


@pytest.mark.parametrize('nrows', ROW_COUNTS)
@pytest.mark.parametrize('n', LENGTHS)
def test_fused_batches(n, nrows):
    """The fused maps of the wallish2018 filter, with and without the split layout."""
    import torch
    from cosmoprimo_amd.dst import DST
    plan, t = DST(n, kx=kx_of(n)), fused_truths(n)
    p = tt.batch(t['p'], nrows, scaled=False)
    y = plan(p, fused=True)
    check_rows('fused forward', y, t['forward'], nrows, n, scaled=False, limit='fused forward')
    assert torch.equal(plan(p, fused=True, split=True), to_split(y))
    coefficients = tt.batch(t['y'], nrows, scaled=False)
    back = plan(coefficients, inverse=True, fused=True)
    check_rows('fused inverse', back, t['inverse'], nrows, n, scaled=False, relative=True, limit='fused inverse')
    assert torch.equal(plan(to_split(coefficients), inverse=True, fused=True, split=True), back)


BAD = (3, 2 * G + 10, 4 * G + 2)
# the partners of rows 3 and 2 G + 10, and the other rows of workgroups 1 (pairs 1, G + 1, 2 G + 1) and 5 (pairs 5, G + 5: its third trip would be pair
# 2 G + 5, rows 4 G + 10 and 4 G + 11, which a batch of 4 G + 3 rows does not have)
NEIGHBOURS = (2, 2 * G + 11, 2 * G + 2, 2 * G + 3, 10, 11)


@pytest.mark.parametrize('mode', ['forward', 'inverse', 'inverse-split', 'fused-forward'])
@pytest.mark.parametrize('n', LENGTHS)
def test_rows_that_are_not_finite_across_trips(n, mode):
    """4 G + 3 rows.  A NaN in row 3 (pair 1: trip 0 of workgroup 1, its partner is row 2), +inf in row 2 G + 10 (pair G + 5: trip 1 of workgroup 5, the
    first of its pair), -inf in the last row, which has no partner (pair 2 G + 1: trip 2 of workgroup 1, the workgroup whose first trip met the
    NaN); under the fused logarithm a zero and a negative sample in the place of the infinities.  Those three rows come out as NaN and nothing else
    does: their partners and every other row of workgroups 1 and 5 meet the bound like all the rest."""
    from cosmoprimo_amd.dst import DST
    nrows = 4 * G + 3
    assert BAD[2] == nrows - 1 and nrows % 2 == 1
    fused = mode == 'fused-forward'
    if fused:
        plan, t = DST(n, kx=kx_of(n)), fused_truths(n)
        x = tt.batch(t['p'], nrows, scaled=False)
        values = (float('nan'), 0., -1.)
    else:
        plan, t = DST(n), truths(n)
        x = tt.batch(t['x'], nrows)
        values = (float('nan'), float('inf'), -float('inf'))
    for row, column, value in zip(BAD, (3, n // 2 + 1, n - 1), values):
        x[row, column] = value
    if mode == 'inverse-split':
        x = to_split(x)
    got = plan(x, inverse=mode.startswith('inverse'), fused=fused, split=mode == 'inverse-split')
    frac = check_rows(mode + ', three bad rows,', got, t['inverse' if mode.startswith('inverse') else 'forward'], nrows, n, scaled=not fused, bad=BAD,
                      limit='fused forward' if fused else 'plain')
    assert (frac[list(NEIGHBOURS)] < LIMITS['fused forward' if fused else 'plain']).all(), frac[list(NEIGHBOURS)]


def test_unknown_flag_is_refused():
    """cp_dst_execute knows CP_DST_FUSED (1) and CP_DST_SPLIT (2): any other bit is CP_EINVAL and nothing is launched."""
    import torch
    from cosmoprimo_amd import _lib, _device as dv
    from cosmoprimo_amd.dst import DST
    plan, lib = DST(256), _lib.load()
    x = torch.ones((2, 256), dtype=torch.float64, device=plan.device)
    out = torch.full_like(x, -7.25)
    for flags in (4, 8, 1 | 4, 2 | 16, -1):
        assert lib.cp_dst_execute(plan._handle, x.data_ptr(), out.data_ptr(), 2, 0, flags, dv.stream_of(plan.device)) == _lib.CP_EINVAL
        assert b'unknown flags' in lib.cp_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.25).all())
