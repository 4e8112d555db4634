"""Host time of every plan constructor and destructor, and the drift of the free device memory over create / destroy cycles, for two builds of the library:

    python tools/bench_plan_tables.py --first PATH/libcosmoprimo_amd.so [--second PATH] [--processes 5] [--out FILE]

The cases are those of tests/test_plan_cycles_gpu.py (every plan type at the smallest size at which all of its device tables exist).  ``--first`` is the
build to compare against (the parent commit's library), ``--second`` the build under test (default: the tree's).  Five processes per build, alternating
between the builds, one at a time; each process makes one untimed cycle of every case, then times 40 constructor calls and 40 destructor calls per
case (host microseconds, the median) and runs the test's own loop of 100 cycles for the drift (bytes of free device memory before the first cycle
minus behind the last).  A row is inside the first build's own spread when the second build's median of medians does not exceed the first build's slowest
process.  Prints the table (and appends it to ``--out``)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
TIMED = 40


def child():
    import torch
    from cosmoprimo_amd import _lib
    from test_plan_cycles_gpu import CASES, cases, cycle
    lib = _lib.load()
    device = torch.device('cuda', 0)
    table, free_shared = cases(lib)
    result = {}
    for name in CASES:
        cycle(lib, name, table[name], torch, device, cycles=1)
    for name in CASES:
        create, _, destroy, _, _ = table[name]
        made, freed = [], []
        for i in range(TIMED):
            t0 = time.perf_counter()
            handle = create()
            t1 = time.perf_counter()
            status = destroy(handle)
            t2 = time.perf_counter()
            _lib.check(status)
            made.append(1e6 * (t1 - t0))
            freed.append(1e6 * (t2 - t1))
        first, last, drift = cycle(lib, name, table[name], torch, device)
        assert torch.equal(first.view(torch.int64), last.view(torch.int64)), name
        result[name] = {'create_us': statistics.median(made), 'destroy_us': statistics.median(freed), 'drift_bytes': int(drift)}
    free_shared()
    print('RESULT ' + json.dumps(result))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--first')
    parser.add_argument('--second', default=None)
    parser.add_argument('--processes', type=int, default=5)
    parser.add_argument('--out', default=None)
    parser.add_argument('--child', action='store_true')
    args = parser.parse_args()
    if args.child:
        return child()
    runs = {'first': [], 'second': []}
    for i in range(args.processes):
        for build, path in (('first', args.first), ('second', args.second)):
            env = dict(os.environ)
            env.pop('COSMOPRIMO_AMD_LIBRARY', None)
            if path:
                env['COSMOPRIMO_AMD_LIBRARY'] = os.path.abspath(path)
            done = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=600, check=True)
            runs[build].append(json.loads([line for line in done.stdout.splitlines() if line.startswith('RESULT ')][-1][7:]))
            print('process %d of the %s build done' % (i + 1, build), flush=True)
    lines = ['%-22s %-8s medians per process, host microseconds: first build | second build | second median <= first max' % ('plan', 'call')]
    outside = []
    for name in runs['first'][0]:
        for call in ('create', 'destroy'):
            first, second = ([run[name][call + '_us'] for run in runs[build]] for build in ('first', 'second'))
            inside = statistics.median(second) <= max(first)
            if not inside:
                outside.append('%s %s' % (name, call))
            lines.append('%-22s %-8s %s | %s | %.1f <= %.1f %s' % (name, call, ' '.join('%.1f' % v for v in first), ' '.join('%.1f' % v for v in second),
                                                                 statistics.median(second), max(first), 'yes' if inside else 'NO'))
    lines.append('rows outside the first build\'s spread: %s' % (', '.join(outside) or 'none'))
    lines.append('%-22s drift of the free device memory over 100 cycles, bytes, per process: first build | second build' % 'plan')
    for name in runs['first'][0]:
        lines.append('%-22s %s | %s' % (name, ' '.join('%d' % run[name]['drift_bytes'] for run in runs['first']), ' '.join('%d' % run[name]['drift_bytes'] for run in runs['second'])))
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        with open(args.out, 'a') as file:
            file.write(text)


if __name__ == '__main__':
    main()
