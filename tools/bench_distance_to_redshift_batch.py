"""DistanceToRedshift over a batch of cosmologies against the loop over one-cosmology objects (what the package offered before):
python tools/bench_distance_to_redshift_batch.py [--runs 3]

Shapes: 64 cosmologies x 10^6 resident distances in float64 and in float32 (the catalogue regime), 2 10^4 cosmologies x 16 distances (the samples
regime).  Build (the table of every cosmology -> spline coefficients) and apply (distances -> redshifts) are timed apart, per sample = per
(cosmology, distance); the runs alternate between the batch and the loop.  The loop of the samples regime is timed on its first 200 cosmologies."""
import argparse
import os
import sys
import time
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, warm=True):
    import torch
    out = fn() if warm else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def tables(nb, nz=512, zmax=100., seed=1):
    import torch
    from cosmoprimo_amd import background as bgm
    rng = np.random.default_rng(seed)
    p = dict(h=rng.uniform(0.6, 0.8, nb), Omega_cdm=rng.uniform(0.2, 0.3, nb), Omega_b=rng.uniform(0.04, 0.06, nb), Omega_k=rng.uniform(-0.05, 0.05, nb),
             w0_fld=rng.uniform(-1.2, -0.8, nb), wa_fld=rng.uniform(-0.3, 0.3, nb))
    zgrid = 1. / np.geomspace(1. / (1. + zmax), 1., nz)[::-1] - 1.
    return bgm.distance('comoving_radial_distance', torch.as_tensor(zgrid, device='cuda'), params=p)


def main():
    import torch
    from cosmoprimo_amd.utils import DistanceToRedshift
    parser = argparse.ArgumentParser()
    parser.add_argument('--runs', type=int, default=3)
    args = parser.parse_args()
    warnings.simplefilter('ignore')
    shapes = [('64 x 1e6 f64', 64, 10**6, torch.float64, 64, 5), ('64 x 1e6 f32', 64, 10**6, torch.float32, 64, 5), ('20000 x 16 f64', 20000, 16, torch.float64, 200, 5)]
    for name, nb, nq, dtype, nloop, reps in shapes:
        table = tables(nb)
        gen = torch.Generator(device='cuda').manual_seed(3)
        d = (torch.rand((nb, nq), dtype=torch.float64, device='cuda', generator=gen) * table[:, -1:]).to(dtype)
        for run in range(args.runs):
            t_build, d2z = timed(lambda: DistanceToRedshift(lambda z: table), reps)
            t_apply, out = timed(lambda: d2z(d, bounds_error=False, per_cosmology=True), reps)

            def loop_build():
                return [DistanceToRedshift(lambda z, i=i: table[i].cpu().numpy()) for i in range(nloop)]

            def loop_apply(objs):
                return [obj(d[i], bounds_error=False) for i, obj in enumerate(objs)]

            # fresh objects, no warm-up call: the first call of a one-cosmology object solves its spline (on the host), as every pass of such a loop does
            l_build, objs = timed(loop_build, 1, warm=False)
            l_apply, ref = timed(lambda: loop_apply(objs), 1, warm=False)
            worst = max(float((out[i].double() - ref[i].double()).abs().max()) for i in range(nloop))
            print('%-15s run %d  batch: build %9.3f ms (%8.3f us / cosmology)  apply %9.3f ms (%8.4f ns / sample) | loop: build %8.3f us / cosmology  apply %8.4f ns / sample'
                  '  | max |dz| batch - loop %.2e' % (name, run, t_build * 1e3, t_build / nb * 1e6, t_apply * 1e3, t_apply / (nb * nq) * 1e9, l_build / nloop * 1e6,
                                                      l_apply / (nloop * nq) * 1e9, worst), flush=True)


if __name__ == '__main__':
    main()
