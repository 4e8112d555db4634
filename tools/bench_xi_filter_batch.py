"""kirkby2013 over batches of cosmologies (cp_kirkby2013_rows): the filter's _compute at B x nz = 1024 x 30 and 10 000 x 30 rows of ns = 1024, device
events over `--calls` calls after a warm-up, against the bytes the kernel must move (16 ns B per row: xi read once, xinow written once); then the
per-cosmology time of the route for one cosmology at a time (a dense operator built per rs_drag ratio on the host), a loop of 64 cosmologies.
    python tools/bench_xi_filter_batch.py [--calls 20]"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8e12      # B/s, MI355X spec


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--calls', type=int, default=20)
    parser.add_argument('--warmup', type=int, default=3)
    args = parser.parse_args()
    import torch
    import cosmoprimo_amd as cp
    from cosmoprimo_amd.bao_filter import Kirkby2013CorrelationFunctionBAOFilter
    warnings.simplefilter('ignore')
    dev = torch.device('cuda:0')
    fid = cp.Cosmology(engine='eisenstein_hu')
    xi2 = fid.get_fourier().pk_interpolator().clone(extrap_kmin=1e-5, extrap_kmax=1e2).to_xi()        # (ns, nz) of one cosmology
    nz = 30
    z = np.linspace(0., 3., nz)
    x1 = cp.CorrelationFunctionInterpolator2D(xi2.s, z, xi2(xi2.s, z), interp_order_z=3)
    f = Kirkby2013CorrelationFunctionBAOFilter(x1, cosmo_fid=fid)
    rows_1 = f._xi_rows                                                                                   # (nz, 1024)
    ns = rows_1.shape[1]
    results = dict(ns=ns, nz=nz, calls=args.calls, bytes_per_row=16 * ns)
    for nb in (1024, 10000):
        rng = np.random.default_rng(nb)
        batch = cp.Cosmology(engine='eisenstein_hu', Omega_cdm=rng.uniform(0.2, 0.32, nb), h=rng.uniform(0.6, 0.78, nb))
        amp = torch.tensor(rng.uniform(0.8, 1.2, nb), device=dev)
        f._xi_rows = (rows_1[None] * amp[:, None, None]).reshape(nb * nz, ns).contiguous()
        f._cosmo = batch
        for _ in range(args.warmup):
            f._compute()
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.calls):
            f._compute()
        stop.record()
        torch.cuda.synchronize()
        ms = start.elapsed_time(stop) / args.calls
        nrows = nb * nz
        gbs = nrows * 16 * ns / (ms * 1e-3) / 1e9
        assert bool(torch.isfinite(f._xinow_rows).all())
        results['B{}'.format(nb)] = dict(rows=nrows, ms_per_call=ms, rows_per_s=nrows / (ms * 1e-3), GB_per_s=gbs, fraction_of_8TBs=gbs * 1e9 / HBM_PEAK)
        print('B x nz = {:5d} x {:d} = {:6d} rows: {:.4f} ms per call, {:.3e} rows/s, {:.0f} GB/s at {:d} B per row, {:.1%} of 8 TB/s'.format(
            nb, nz, nrows, ms, nrows / (ms * 1e-3), gbs, 16 * ns, gbs * 1e9 / HBM_PEAK), flush=True)
        f._xi_rows = f._xinow_rows = None
        torch.cuda.empty_cache()
    # the route for one cosmology at a time: a dense operator per rs_drag ratio (built on the host, uploaded), applied to the cosmology's nz rows
    nloop = 64
    rng = np.random.default_rng(64)
    singles = [cp.Cosmology(engine='eisenstein_hu', Omega_cdm=float(o), h=float(h)) for o, h in zip(rng.uniform(0.2, 0.32, nloop), rng.uniform(0.6, 0.78, nloop))]
    f._xi_rows = rows_1
    for c in singles:
        c.rs_drag      # (the sound horizons computed before the clock starts)
    f._cosmo = singles[0]
    f._compute()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in singles:
        f._cosmo = c
        f._compute()
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / nloop * 1e3
    results['one_cosmology_at_a_time'] = dict(cosmologies=nloop, ms_per_cosmology=per)
    print('one cosmology at a time (dense operator per ratio), {:d} cosmologies x {:d} rows: {:.2f} ms per cosmology'.format(nloop, nz, per), flush=True)
    print(json.dumps(results))


if __name__ == '__main__':
    main()
