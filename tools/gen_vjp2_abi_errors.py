"""Write tests/golden/vjp2_abi_errors.json: (entry point, arguments, status, message) of every bad call of cp_mlp_vjp2 and cp_taylor_vjp2 in the table below,
as the built library answers.

    python tools/gen_vjp2_abi_errors.py [--out tests/golden/vjp2_abi_errors.json]

Run on the CPU (no device is needed: every call comes back before its first device call) against the library whose answers are to be pinned.  Every
pointer is a fake non-null one or null, so a call that got past the checks would launch on it: an answer other than CP_EINVAL, CP_EUNSUPPORTED, or CP_OK
for an empty batch is refused and nothing is written.  tests/test_vjp2_abi_errors_host.py replays the file."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from test_vjp2_abi_errors_host import ENTRIES, call, comes_back_early  # noqa: E402

BIG = 2**40                                   # a workspace nobody allocates
RANGES = [(-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)]      # of M = 8
ROW_TILES = (2**31 - 1) * 64                  # rows of the largest grid
POINTERS = {'cp_mlp_vjp2': ['x', 'params', 'xoffset', 'xscale', 'yoffset', 'yscale', 'cot', 'hess', 'work'],      # (a null d_value is no fault)
            'cp_taylor_vjp2': ['x', 'center', 'powers', 'derivatives', 'cot', 'hess', 'work']}
STRIDES = {'cp_mlp_vjp2': ['ldc', 'ldv'], 'cp_taylor_vjp2': ['ldc']}


def arguments(entry, B=4, ndim=3, widths=(5, 17), acts=0, M=8, yfunction=0, T=20, max_power=3, col0=0, ncols=8, work=BIG, null=(), **strides):
    """The argument list of ``entry`` in the fixture's notation; ``null``: names of POINTERS[entry] to pass as null, or 'all'."""
    p = {name: None if null == 'all' or name in null else 'ptr' for name in POINTERS[entry] + ['value']}
    ld = lambda name: strides.get(name, 8)  # noqa: E731
    mlp = entry.startswith('cp_mlp')
    if mlp:
        head = [p['x'], B, ndim, len(widths), list(widths), None if acts is None else [acts] * len(widths), M, p['params'], p['xoffset'], p['xscale'], p['yoffset'],
                p['yscale'], yfunction]
    else:
        head = [p['x'], B, p['center'], p['powers'], ndim, T, max_power, p['derivatives'], M]
    return head + [col0, ncols, p['cot'], ld('ldc')] + ([p['value'], ld('ldv')] if mlp else []) + [p['hess'], p['work'], work] + [0, None]


def table(lib):
    """[(entry, what, arguments)]"""
    cases = []
    widths = (ctypes.c_int * 2)(5, 17)
    for entry in ENTRIES:
        mlp = entry.startswith('cp_mlp')
        add = lambda what, **options: cases.append((entry, what, arguments(entry, **options)))  # noqa: E731
        for name in POINTERS[entry]:
            add('null d_' + name, null=(name,))
        add('B = -1', B=-1)
        add('B = 0, every pointer null', B=0, null='all', work=0)
        for ndim in (0, 33):
            add('ndim = %d' % ndim, ndim=ndim)
        strides = STRIDES[entry]
        for col0, ncols in RANGES:
            add('columns (%d, %d) of 8' % (col0, ncols), col0=col0, ncols=ncols, **{name: 16 for name in strides})
        for name in strides:
            add(name + ' one short', **{name: 7})
        if mlp:
            for yfunction in (-1, 3):
                add('yfunction = %d' % yfunction, yfunction=yfunction)
            for w in ((5, 65), (5, 0), (8,) * 9):
                add('widths %s' % (w,), widths=w)
            add('no activation codes', acts=None)
        else:
            for max_power in (-1, 16):
                add('max_power = %d' % max_power, max_power=max_power)
            add('T = 0', T=0)
        # a row per point and pair i <= j: 6 pairs at ndim = 3, 528 at ndim = 32
        for ndim, npairs in ((3, 6), (32, 528)):
            add('ndim = %d, one past the grid' % ndim, ndim=ndim, B=ROW_TILES // npairs + 1)
            add('ndim = %d, the grid full, every pointer null' % ndim, ndim=ndim, B=ROW_TILES // npairs, null='all')
        if mlp:      # under a y function the cotangents B ncols are capped as well (a thread each in 2^31 - 1 workgroups of 256); no y function: no such cap
            wide = dict(M=2**22, ncols=2**22, ldc=2**22, ldv=2**22)
            add('yfunction = 1, one past the cotangents', yfunction=1, B=2**17, **wide)
            add('yfunction = 1, the cotangents full, every pointer null', yfunction=1, B=2**17 - 1, null='all', **wide)
            add('yfunction = 0, as many cotangents, every pointer null', yfunction=0, B=2**17, null='all', **wide)
        needs = [(0, 4 * 20)] if not mlp else [(y, int(lib.cp_mlp_vjp2_workspace_doubles(4, 3, 2, widths, 8, 8, y))) for y in (0, 1, 2)]
        for yfunction, need in needs:
            add('yfunction = %d, workspace one short' % yfunction, yfunction=yfunction, work=need - 1)
        add('null d_x and a short workspace', null=('x',), work=needs[0][1] - 1)
        # two faults at once: the first check in the order of the entry point answers
        add('B = -1 and a bad range', B=-1, col0=4, ncols=5)
        add('a bad range and ndim = 33', col0=4, ncols=5, ndim=33)
        add('a bad range and a short stride', col0=0, ncols=9, **{name: 7 for name in strides})
        add('a short stride and one past the grid', B=ROW_TILES // 6 + 1, ldc=7)
        add('one past the grid and a null pointer', B=ROW_TILES // 6 + 1, null=('cot',))
        if mlp:
            add('yfunction = 3 and a bad range', yfunction=3, col0=4, ncols=5)
    return cases


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'vjp2_abi_errors.json'))
    args = parser.parse_args()
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    recorded = []
    for entry, what, arguments_ in table(lib):
        status, message = call(lib, entry, arguments_)
        case = {'entry': entry, 'what': what, 'args': arguments_, 'status': status, 'message': message}
        if not comes_back_early(case):
            sys.exit('%s, %s: status %d (%s) -- this call got past the checks; nothing written' % (entry, what, status, message))
        recorded.append(case)
    with open(args.out, 'w') as file:
        file.write('[\n' + ',\n'.join(json.dumps(case) for case in recorded) + '\n]\n')
    print('%d calls written to %s' % (len(recorded), args.out))


if __name__ == '__main__':
    main()
