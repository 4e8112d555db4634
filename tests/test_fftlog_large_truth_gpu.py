"""GPU: the four-step FFTLog of csrc/cp_fftlog_large.hip (padded lengths Np = 2^14 ... 2^24) against exact longdouble truth at EVERY column plan,
through the C ABI (cp_fftlog_plan_create with synthetic tables, cp_fftlog_execute, cp_fftlog_plan_destroy).  The kernel table u is made of five
taps, which turns the promised transform into a sparse circular correlation that needs no FFT (tests/fftlog_taps_truth.py, held to a direct DFT and
to oracle.fftlog.apply by tests/test_fftlog_taps_host.py).  Allowance: ALLOW = 16 x the rounding level of the float64 numpy restatement, per row,
relative to the row's largest |truth|; every test prints the largest fraction of it that was used.

  test_every_column_plan     N1 = Np / 4096 = 4, 8, 16 (column_direct_kernel), 32 ... 256 (two passes of column_kernel, radices (16, 2 / 4 / 8 / 16),
                             C = 128 ... 16 columns per tile), 512 ... 2048 (three passes, C = 8, 4, 2) and 4096 (C = 1, one column per tile, and a
                             chunk of one pair: the two pairs are two trips through the scratch); odd n and odd Np - n; the second pair without a
                             partner; every output element written and none beyond
  test_second_chunk          516 pairs of three kernel indices against a chunk of 512 at Np = 2^14: pair0 = 512 is no multiple of 3
  test_screening_three_pass  zero, NaN, +Inf and subnormal rows in mixed pairs at Np = 2^21
  test_two_streams_one_plan  two host threads, two streams, one plan of Np = 2^16 (the scratch ordered by the plan's event): bit-equal results

Largest fraction of the allowance measured on the MI355X, per Np (against the truth; 1 is the limit):
  2^14 0.083   2^15 0.079   2^16 0.063   2^17 0.063   2^18 0.073   2^19 0.069   2^20 0.070   2^21 0.063   2^22 0.058   2^23 0.066   2^24 0.061
  (levels 5.1 ... 7.4 FLOOR: the device is as far from the truth as numpy is, 1/16 = 0.0625); second chunk 0.076; screening 0.057, its subnormal row 0.127.
Found by test_screening_three_pass: a row of zeros packed with a live partner came back as rounding noise of the packed transform (up to 2.1e-15 in every
element); row_scale now stores such a row as zeros.  Mutations of a scratch copy of the kernel file: the kernel index of row_kernel taken from the slot
inside the chunk fails test_second_chunk alone; mask_b one bit short fails every size, the chunk and the screening test; freq_of_pos with the radices in
reverse order fails N1 = 32 ... 128 and 512 ... 2048 on the canary.  Two entries of rd.r swapped at N1 = 512 change nothing: every order is a valid plan.
"""
import threading
import time

import numpy as np
import pytest

import fftlog_taps_truth as tt
from fftlog_device import CANARY, Plan, lib      # noqa: F401  (lib: the fixture)

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize('npad', tt.LADDER)
def test_every_column_plan(lib, npad):
    start = time.time()
    n, nbatch, nker, modes = tt.ladder_case(npad)
    cases = [(mode, tt.ladder_truth(npad, *mode)) for mode in modes]
    with Plan(lib, n, cases[0][1][0]) as plan:
        for (extrap, keep), (syn, base, true, level) in cases:
            assert syn is plan.syn
            got = plan(tt.batch(base, nbatch, nker), extrap, keep)
            true, level = tt.expected(true, level, nbatch)
            what = 'Np = 2^%d (N1 = %d), %s, keep_padding=%s' % (npad.bit_length() - 1, npad // 4096, extrap, keep)
            assert tt.check(tt.unscale(got, nbatch, nker), true, level, what) <= 1.
    print('Np = 2^%d: %.1f s' % (npad.bit_length() - 1, time.time() - start))


def test_second_chunk(lib):
    """A second trip through the scratch at the smallest size: 343 batch items of three kernel indices are 172 x 3 = 516 pairs against a chunk of
    128 MB / (16 x 2^14) = 512.  The second chunk starts at pair0 = 512, 512 mod 3 = 2: a kernel index taken from the slot inside the chunk would be
    the wrong one; it holds four pairs, the last batch item without a partner.  Every row against the truth."""
    npad, n, nker, nbatch = 1 << 14, 5001, 3, 343
    assert ((nbatch + 1) // 2) * nker == 516 and (npad - n) % 2 == 1
    syn = tt.tables(npad, nker, seed=1)
    base, true, level = tt.base_case(n, npad, syn, 0, False, seed=1)
    with Plan(lib, n, syn) as plan:
        got = plan(tt.batch(base, nbatch, nker), 0, False)
    true, level = tt.expected(true, level, nbatch)
    got = tt.unscale(got, nbatch, nker)
    first = 2 * (512 // nker)      # the first batch item with a pair in the second chunk
    assert tt.check(got[:first], true[:first], level[:first], 'Np = 2^14, batch items of the first chunk') <= 1.
    assert tt.check(got[first:], true[first:], level[first:], 'Np = 2^14, batch items %d ... %d (second chunk from pair 512 on)' % (first, nbatch - 1)) <= 1.


def test_screening_three_pass(lib):
    """Row screening (screen_kernel, row_scale, the stores of column_kernel with and without a partner) at a three-pass size, Np = 2^21: nine rows in
    the pairs (zero, 2^24) (NaN, 2^-40) (2^10, +Inf) (subnormal, 2^3) and a single 2^-13.  A row that is not finite comes back NaN throughout, the
    zero row exactly 0, every other row -- the partners of those included -- within its own allowance.
    The subnormal row is base row 0 times 2^-1030 (rounded: its truth and its level are formed from the row as it is, by the same rule as every
    other row's).  Its tilted samples are subnormal float64 products and so is its result: the level of the restatement is 245 FLOOR there, and the
    device is measured at two such levels (0.127 of the allowance): row_scale stops at 2^1022, which leaves the row at 2^-7 of its partner in the
    packed transform.  (An allowance worked out from the number format alone -- the base row's level, half a quantum 2^-1075 per tilted sample
    through the tap sum and half a quantum of the result -- was tried first and is missed by a factor 1.84 for that reason.)"""
    npad, extrap = tt.THREE_PASS, 'edge'
    n, _, nker, _ = tt.ladder_case(npad)
    syn, base, base_true, base_level = tt.ladder_truth(npad, extrap, False)      # (shared with test_every_column_plan)
    pre, post, tap = syn.pre[0], syn.post[0], syn.taps[0]
    scaled = {1: (1, 24), 3: (1, -40), 4: (0, 10), 7: (1, 3), 8: (0, -13)}      # row: (base row, exponent)
    rows = np.zeros((9, 1, n))
    true = np.zeros((9, 1, n), dtype=tt.LD)
    level = np.full((9, 1), tt.FLOOR)
    for i, (b, e) in scaled.items():
        rows[i, 0], true[i, 0], level[i, 0] = np.ldexp(base[b], e), np.ldexp(base_true[b, 0], e), base_level[b, 0]
    rows[2, 0], rows[5, 0] = base[0], base[1]
    rows[2, 0, n // 3], rows[5, 0, 0] = np.nan, np.inf
    true[2], true[5] = np.nan, np.nan
    rows[6, 0] = np.ldexp(base[0], -1030)
    in_left, in_right, _ = tt.widths(n, npad)
    tilted = np.abs(tt.ofl.pad(rows[6, 0], (in_left, in_right), extrap) * pre)
    assert 0. < tilted.max() < 2.**-1022
    true[6, 0] = tt.truth(rows[6, 0], n, npad, pre, post, tap, extrap)
    level[6, 0] = tt.levels(true[6, 0], tt.restated(rows[6, 0], n, npad, pre, post, syn.u[0], extrap))[1]
    with Plan(lib, n, syn) as plan:
        with np.errstate(all='ignore'):
            got = plan(rows, extrap, False)
    assert np.isnan(got[2]).all() and np.isnan(got[5]).all()
    assert (got[0] == 0.).all(), 'the zero row: {:d} elements are not 0, the largest {:.3g}'.format(int((got[0] != 0.).sum()), float(np.abs(got[0]).max()))
    normal = np.arange(9) != 6
    assert tt.check(got[normal], true[normal], level[normal], 'Np = 2^21, screening, all rows but the subnormal one') <= 1.
    assert tt.check(got[6:7], true[6:7], level[6:7], 'Np = 2^21, screening, the subnormal row') <= 1.


def test_two_streams_one_plan(lib):
    """One LARGE plan from two streams (the shape of test_two_host_threads_on_one_plan, whose n = 2048 runs the fused kernel): the scratch of the
    plan is shared, an execute waits on its own stream for the event the previous execute recorded.  Two host threads, each with its own stream,
    rows and outputs, six executes each; every output bit-equal to the one-stream result of the same rows."""
    import torch
    npad, nbatch, reps = 1 << 16, 5, 6
    n = (npad // 3) | 1
    syn = tt.tables(npad, 1)
    with Plan(lib, n, syn) as plan:
        inputs, expect = [], []
        for i in range(2):
            rows = tt.batch(tt.base_rows(n, seed=10 + i), nbatch, 1) * (1. + i)
            expect.append(plan(rows, 'edge', False))
            inputs.append(torch.as_tensor(rows, device=plan.dev))
        outs = [[torch.full((nbatch, 1, n), CANARY, dtype=torch.float64, device=plan.dev) for _ in range(reps)] for _ in range(2)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        errors = []
        begin = threading.Barrier(2)

        def work(i):
            try:
                begin.wait()
                for r in range(reps):
                    plan.enqueue(inputs[i], outs[i][r], 'edge', False, streams[i].cuda_stream)
                streams[i].synchronize()
            except Exception as exc:      # noqa: BLE001
                errors.append(exc)

        threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        torch.cuda.synchronize()
    assert not errors, errors
    for i in range(2):
        for r in range(reps):
            np.testing.assert_array_equal(outs[i][r].cpu().numpy(), expect[i], err_msg='thread %d, execute %d' % (i, r))
