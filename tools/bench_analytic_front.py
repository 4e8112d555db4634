"""Host time per call of the analytic-spectrum entry points through their Python wrappers, where they are launch-bound (one cosmology) and where the
device bounds them (16 384 cosmologies).

    python tools/bench_analytic_front.py [--repeats 20] [--json FILE] [--tree DIR]
    python tools/bench_analytic_front.py --summarise 'parent_*.json' 'result_*.json'

``power.analytic`` (EH98, 1024 wavenumbers, one redshift), ``sigma8_normalise``, ``sigma_rz_analytic`` by its three one-kernel routes (the functional
with one radius; 64 radii through the fused kernel, prefiltered and plain) and the wallish2018 filter of an analytic batch (``cp_wallish_full`` through
``Wallish2018PowerSpectrumBAOFilter._full``).  n calls are made back to back after a synchronisation (n = 50 for one cosmology, 5 for 16 384) and two
times are taken, each divided by n: ``host`` until the last call has returned, ``through`` until the device has finished them (tools/bench_emulator_front.py).

To compare two builds run it in five processes per build, alternating (``--tree DIR``: the package of another, built, checkout), each with
``--json``; ``--summarise`` then prints, per call, every process's median (host for one cosmology, through for 16 384) and whether the second build's
median of medians stays at or below the first build's slowest process -- the first build's own spread is the margin.  Needs neither the reference nor the
oracle."""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tools'), os.path.join(ROOT, 'tests')]


def cases(torch, dev):
    from cosmoprimo_amd import power as pw, interpolator as itp
    from test_analytic_front_bits_gpu import wallish_filter
    rng = np.random.default_rng(0)
    k, z, found = np.geomspace(1e-4, 10., 1024), np.array([0.5]), []
    radii = {'functional': np.array([8.]), 'prefiltered': np.geomspace(1., 60., 64), 'plain': np.geomspace(1., 60., 64)}
    for B in (1, 16384):
        bg = dict(h=rng.uniform(0.6, 0.8, B), Omega_cdm=rng.uniform(0.2, 0.3, B), Omega_b=rng.uniform(0.04, 0.06, B))
        pk = dict(n_s=rng.uniform(0.9, 1., B))
        bg, pk = {name: torch.as_tensor(v, device=dev) for name, v in bg.items()}, {name: torch.as_tensor(v, device=dev) for name, v in pk.items()}
        growth_sq = torch.as_tensor(rng.uniform(0.3, 1., (B, 2)), device=dev)
        found.append(('power.analytic', B, lambda bg=bg, pk=pk: pw.analytic('eisenstein_hu', 'matter', k, z=z, bg=bg, pk=pk, device=dev)))
        found.append(('sigma8_normalise', B, lambda bg=bg, pk=pk: itp.sigma8_normalise('eisenstein_hu', bg, pk, 0.8, dev)))
        for route, r in radii.items():
            def sigma(bg=bg, pk=pk, g=growth_sq, r=r, prefiltered=route != 'plain'):
                itp._SIGMA_RZ_PREFILTERED = prefiltered
                return itp.sigma_rz_analytic('eisenstein_hu', bg, pk, r, g, dev)
            found.append(('sigma_rz_analytic (%s)' % route, B, sigma))
        f = wallish_filter()
        f._pk_rows = pw.analytic('eisenstein_hu', 'matter', f.k, bg=bg, pk=pk, device=dev).reshape(B, -1)
        dst = f._operators()['dst']
        found.append(('wallish2018 (cp_wallish_full)', B, lambda f=f, bg=bg, pk=pk, dst=dst: f._full('eisenstein_hu', bg, pk, dst)))
    return found


def summarise(first, second):
    runs = [[json.load(open(path)) for path in sorted(glob.glob(pattern))] for pattern in (first, second)]
    assert runs[0] and runs[1], 'no files'
    print('%-36s %6s  %-8s %s' % ('call', 'B', 'time', 'medians per process, microseconds: first build | second build | second median <= first max'))
    ok = True
    for key in runs[0][0]:
        name, B = key.rsplit(' ', 1)
        a, b = [[run[key] for run in build] for build in runs]
        passed = float(np.median(b)) <= max(a)
        ok = ok and passed
        print('%-36s %6s  %-8s %s | %s | %.1f <= %.1f %s' % (name, B, 'host' if B == '1' else 'through', ' '.join('%.1f' % t for t in a), ' '.join('%.1f' % t for t in b),
                                                         np.median(b), max(a), 'yes' if passed else 'NO'))
    return 0 if ok else 1


def main():
    from bench_emulator_front import per_call
    parser = argparse.ArgumentParser()
    parser.add_argument('--repeats', type=int, default=20)
    parser.add_argument('--json', default=None)
    parser.add_argument('--summarise', nargs=2, default=None)
    parser.add_argument('--tree', default=None, help='import cosmoprimo_amd from this checkout instead of the one the tool lies in')
    args = parser.parse_args()
    if args.summarise:
        return summarise(*args.summarise)
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    dev = torch.device('cuda', 0)
    print('%-36s %6s  %26s  %26s   (microseconds per call: median (min .. max))' % ('call', 'B', 'host', 'through'))
    medians = {}
    for name, B, fn in cases(torch, dev):
        host, through = per_call(torch, fn, 50 if B == 1 else 5, args.repeats)
        print('%-36s %6d  %s  %s' % ((name, B) + tuple('%8.1f (%6.1f .. %6.1f)' % (np.median(t), t.min(), t.max()) for t in (host, through))))
        medians['%s %d' % (name, B)] = float(np.median(host if B == 1 else through))
    if args.json:
        with open(args.json, 'w') as file:
            json.dump(medians, file)
    return 0


if __name__ == '__main__':
    sys.exit(main())
