"""The headline FFTLog kernel (N = 2048, zero padding) may hold the four waves of a workgroup apart between the barrier behind its first phase and
the barrier in front of its last (cp_fftlog_body.h: CP_WAVE_SKEW).  In that span the waves exchange through LDS slots of their own and share only read-only
tables and one screening slot per wave, so the offset decides when a wave runs and never what it computes: a pair of rows gives the same bits alone and
inside a batch in which some workgroups take three pairs, the fix-ups of NaN and unequal rows still reach the right rows, and launches of one plan on two
streams equal one launch.  N = 2048 with the defaults of PowerToCorrelation(ell=0) is the instantiation that balances_cu() selects."""
import numpy as np
import pytest

from conftest import tilted_err
from oracle import fftlog as ofl

pytestmark = pytest.mark.gpu

N = 2048
NB = 2051       # 1026 pairs over 512 workgroups: workgroups 0 and 1 take three pairs, and workgroup 1 ends on the incomplete pair (row 2050 alone)
TOL_NORM = 1e-13        # tests/test_fftlog_gpu.py, this size: tilted-space norm-wise ...
TOL_POINT = 1e-10       # ... and pointwise for s in [1e-2, 2e2] Mpc/h
TOL_ROW = 5e-14         # tests/test_fftlog_gpu.py, test_rows_are_independent_through_the_c_abi: relative to the row's own tilted magnitude


def execute(plan, tin, tout, first, nbatch, stream=0):
    """cp_fftlog_execute on rows [first, first + nbatch) of two (rows, n) device tensors, zero padding."""
    from cosmoprimo_amd import _lib
    step = tin.shape[-1] * 8
    _lib.check(_lib.load().cp_fftlog_execute(plan.handle, tin.data_ptr() + first * step, tout.data_ptr() + first * step, nbatch, 0, 0., 0, 0., 0, stream))


@pytest.fixture(scope='module')
def batch(golden):
    """k, the plan, NB config-2-like rows on the device, and their transform in one launch (computed once, never modified)."""
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    import cosmoprimo_amd as cp
    pkd = golden('pk_eh_default')
    k, pk = pkd['k%d' % N], pkd['pk%d' % N]
    rng = np.random.default_rng(2051)
    rows_h = rng.uniform(0.5, 2., NB)[:, None] * (k[None, :] / 0.05) ** rng.uniform(-0.1, 0.1, NB)[:, None] * pk[None, :]
    dev = torch.device('cuda', torch.cuda.current_device())
    rows = torch.as_tensor(rows_h, device=dev)
    plan = cp.PowerToCorrelation(k, ell=0)._get_plan(dev)
    whole = torch.full_like(rows, np.nan)
    execute(plan, rows, whole, 0, NB)
    torch.cuda.synchronize()
    return dict(k=k, plan=plan, rows=rows, rows_h=rows_h, whole=whole, dev=dev)


def pointwise(g, ref, s, lo=1e-2, hi=2e2):
    m = (s > lo) & (s < hi)
    return np.abs(g[..., m] / ref[..., m] - 1.).max()


def test_the_large_batch_spreads_three_pairs_over_some_workgroups(batch):
    import ctypes
    from cosmoprimo_amd import _lib
    grid, block, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().cp_fftlog_plan_info(batch['plan'].handle, NB, ctypes.byref(grid), ctypes.byref(block), ctypes.byref(lds)))
    npairs = (NB + 1) // 2
    assert block.value == 256 and 2 * grid.value < npairs <= 3 * grid.value, (grid.value, npairs)


@pytest.mark.parametrize('nb', [2, 3, NB])
def test_sampled_rows_against_the_oracle(batch, nb):
    import torch
    k, rows = batch['k'], batch['rows']
    if nb == NB:
        got_d = batch['whole']
        grid = 512
        sample = sorted({0, 1, 2, 3, 2 * grid - 1, 2 * grid, 2 * grid + 1, NB // 2, NB // 2 + 1, 4 * grid - 2, 4 * grid - 1, 4 * grid, 4 * grid + 1, NB - 2, NB - 1})
    else:
        got_d = torch.full_like(rows[:nb], np.nan)
        execute(batch['plan'], rows, got_d, 0, nb)
        sample = list(range(nb))
    got = got_d[sample].cpu().numpy()
    t = ofl.power_to_correlation(k, ell=0)
    ref = ofl.apply(t, batch['rows_h'][sample][:, None, :])[:, 0]
    s = t.y[0]
    errs = [tilted_err(got[i], ref[i], s, 1.5) for i in range(len(sample))]
    print('nb = %d: worst tilted error %.2e, worst pointwise %.2e' % (nb, max(errs), pointwise(got, ref, s)))
    assert np.isfinite(got).all()
    assert max(errs) < TOL_NORM
    assert pointwise(got, ref, s) < TOL_POINT


def test_pairs_alone_equal_the_large_launch(batch):
    """Pairs (2 q, 2 q + 1) of first, middle and last workgroups, of their first, second and third turn; the last is the incomplete pair."""
    import torch
    rows, whole = batch['rows'], batch['whole']
    alone = torch.full_like(rows, np.nan)
    qs = [0, 1, 255, 256, 511, 512, 768, 1023, 1024, 1025]
    for q in qs:
        execute(batch['plan'], rows, alone, 2 * q, min(2, NB - 2 * q))
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all()
    for q in qs:
        assert torch.equal(alone[2 * q:2 * q + 2], whole[2 * q:2 * q + 2]), q


def test_fix_ups_reach_the_right_rows(batch):
    """A NaN row beside a finite one, and two rows 2^40 apart (the kernel rescales such a pair): the partner equals what it gives when paired with a copy of
    itself, to the row-independence tolerance; in the middle of a batch whose other pairs need no fix-up."""
    import torch
    k, rows = batch['k'], batch['rows']
    mixed = rows[:64].clone()
    mixed[10, N // 3] = float('nan')        # pair (10, 11): 11 is the finite partner
    mixed[21] = mixed[21] * 2.**40          # pair (20, 21): both finite, exponents 40 apart
    partners = [11, 20, 21]
    selfp = torch.stack([mixed[i] for i in partners for _ in range(2)])
    got, gots = torch.full_like(mixed, np.nan), torch.full_like(selfp, np.nan)
    execute(batch['plan'], mixed, got, 0, mixed.shape[0])
    execute(batch['plan'], selfp, gots, 0, selfp.shape[0])
    torch.cuda.synchronize()
    assert bool(torch.isnan(got[10]).all())
    untouched = [i for i in range(64) if i not in (10, 11, 20, 21)]
    assert torch.equal(got[untouched], batch['whole'][untouched])
    t = ofl.power_to_correlation(k, ell=0)
    post = np.abs(t.post[0, t.out_left:t.out_left + t.n])
    for j, i in enumerate(partners):
        a, b = got[i].cpu().numpy(), gots[2 * j].cpu().numpy()
        scale = np.abs(ofl.pad(mixed[i].cpu().numpy()[None, None, :], (t.in_left, t.in_right), 0) * t.pre).max()
        err = (np.abs(a - b) / post / scale).max()
        print('row %d: %.2e of its own tilted magnitude from its self-paired value' % (i, err))
        assert np.isfinite(a).all() and err < TOL_ROW, (i, err)


def test_two_streams_of_one_plan_equal_one_launch(batch):
    import torch
    rows, whole = batch['rows'], batch['whole']
    out = torch.full_like(rows, np.nan)
    half = 1026     # even: the pairs are those of the single launch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    execute(batch['plan'], rows, out, 0, half, s1.cuda_stream)
    execute(batch['plan'], rows, out, half, NB - half, s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    assert torch.equal(out, whole)
