"""The headline FFTLog kernel (N = 2048, zero padding) lets the two workgroups of a CU trade the hardware priority once per launch, by the parity of a
ticket each takes from a per-CU counter that lives in the plan and is never reset (cp_fftlog_kernel.h: balances_cu).  The ticket decides when a wave is
served and never what it computes, so: a row's result does not depend on the batch it is transformed in, on how the batch divides over the grid, on
earlier launches of the plan, or on launches that run beside it -- all bit for bit."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def cp():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    import cosmoprimo_amd
    return cosmoprimo_amd


def execute(lib, plan, tin, tout, first, nbatch, stream=0):
    """cp_fftlog_execute on rows [first, first + nbatch) of two (rows, n) device tensors, zero padding."""
    from cosmoprimo_amd import _lib
    step = tin.shape[-1] * 8
    _lib.check(lib.cp_fftlog_execute(plan.handle, tin.data_ptr() + first * step, tout.data_ptr() + first * step, nbatch, 0, 0., 0, 0., 0, stream))


def batch_and_pairs(cp, k, rows):
    """rows (nb, n) on the device -> (one launch over all rows, one launch per pair of rows (2 i, 2 i + 1))."""
    import torch
    from cosmoprimo_amd import _lib
    f = cp.PowerToCorrelation(k, ell=0)
    dev = rows.device
    plan, lib = f._get_plan(dev), _lib.load()
    nb = rows.shape[0]
    whole, pairs = torch.full_like(rows, np.nan), torch.full_like(rows, np.nan)
    execute(lib, plan, rows, whole, 0, nb)
    for i in range(0, nb, 2):
        execute(lib, plan, rows, pairs, i, min(2, nb - i))
    torch.cuda.synchronize()
    return whole, pairs


def test_config2_golden_rows_alone_and_together(cp, golden):
    import torch
    from oracle.workloads import config2_rows
    g = golden('fftlog_transforms')
    pkd = golden('pk_eh_default')
    k, pk = pkd['k2048'], pkd['pk2048']
    rows = torch.as_tensor(np.concatenate([config2_rows(k, pk, i, i + 1) for i in g['config2_idx']]), device='cuda')
    whole, pairs = batch_and_pairs(cp, k, rows)
    assert torch.isfinite(whole).all()
    assert torch.equal(whole, pairs)
    # and through the facade, as test_config2_golden_rows calls it
    assert torch.equal(torch.as_tensor(cp.PowerToCorrelation(k, ell=0)(rows)[1], device='cuda'), whole)


@pytest.mark.parametrize('nb', [1, 3, 1001, 100001])
def test_batches_that_do_not_divide_over_the_grid(cp, golden, nb):
    """1 row, 3 rows, an odd count below the grid's 512 pairs x 2 rows... and 100 001 rows: 50 001 pairs over 512 workgroups, the last pair half empty."""
    import torch
    pkd = golden('pk_eh_default')
    k, pk = pkd['k2048'], pkd['pk2048']
    rng = np.random.default_rng(nb)
    dev = torch.device('cuda')
    amp, dn = torch.as_tensor(rng.uniform(0.5, 2., nb), device=dev), torch.as_tensor(rng.uniform(-0.1, 0.1, nb), device=dev)
    tk, tpk = torch.as_tensor(k, device=dev), torch.as_tensor(pk, device=dev)
    rows = (amp[:, None] * (tk[None, :] / 0.05) ** dn[:, None] * tpk[None, :]).contiguous()
    whole, pairs = batch_and_pairs(cp, k, rows)
    assert torch.isfinite(whole).all()
    assert torch.equal(whole, pairs)


def test_repeated_launches_and_two_plans_on_three_streams(cp):
    """The ticket counters belong to a plan and are never reset.  Three host threads, each with its own stream, rows and outputs: two of them share one
    plan, the third has a plan of its own; every one of their repeated launches equals the result of a quiet, single launch bit for bit."""
    import torch
    from cosmoprimo_amd import _lib
    n, nb, reps = 2048, 4096, 12      # 2048 pairs: the whole grid, two workgroups on every CU
    k = np.logspace(-5, 2, n)
    fs = [cp.PowerToCorrelation(k, ell=0), cp.PowerToCorrelation(k * 1.5, ell=0)]
    dev = torch.device('cuda', torch.cuda.current_device())
    lib = _lib.load()
    plans = [fs[0]._get_plan(dev), fs[0]._get_plan(dev), fs[1]._get_plan(dev)]
    assert plans[0].handle == plans[1].handle and plans[2].handle != plans[0].handle
    rng = np.random.default_rng(12)
    inputs = [torch.as_tensor(rng.uniform(0.5, 2., (nb, 1)) * k**-1.2, device=dev) for _ in range(3)]
    expected = [(fs[0], fs[0], fs[1])[i](inputs[i])[1] for i in range(3)]
    torch.cuda.synchronize()
    outs = [[torch.empty_like(rows) for _ in range(reps)] for rows in inputs]
    streams = [torch.cuda.Stream() for _ in range(3)]
    errors = []
    start = threading.Barrier(3)

    def work(i):
        try:
            start.wait()
            for r in range(reps):
                execute(lib, plans[i], inputs[i], outs[i][r], 0, nb, streams[i].cuda_stream)
            streams[i].synchronize()
        except Exception as exc:      # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(3)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(3):
        for r in range(reps):
            assert torch.equal(outs[i][r], expected[i]), (i, r)


def test_plan_info_with_the_ticket_word(cp):
    """cp_fftlog_plan_info of the headline plan: the LDS it reports (the kernel's own plus the 16-byte ticket word) still lets two workgroups share a
    CU's 160 KiB, and the grid is what the runtime's occupancy gives for that amount: two workgroups per CU."""
    import ctypes
    import torch
    from cosmoprimo_amd import _lib
    dev = torch.device('cuda', torch.cuda.current_device())
    plan = cp.PowerToCorrelation(np.logspace(-5, 2, 2048), ell=0)._get_plan(dev)
    grid, block, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _lib.check(_lib.load().cp_fftlog_plan_info(plan.handle, 100000, ctypes.byref(grid), ctypes.byref(block), ctypes.byref(lds)))
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    assert (grid.value, block.value) == (2 * ncu, 256)
    assert lds.value % 16 == 0 and 16 * 4096 + 16 < lds.value and 2 * lds.value <= 160 * 1024
