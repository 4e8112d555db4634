"""Write tests/golden/jvp2_abi_errors.json: (entry point, arguments, status, message) of every bad call of cp_mlp_jvp2 and cp_taylor_jvp2 in the table below,
as the built library answers.

    python tools/gen_jvp2_abi_errors.py [--out tests/golden/jvp2_abi_errors.json]

Run on the CPU (no device is needed: every call comes back before its first device call) against the library whose answers are to be pinned, in the way
of tools/gen_emulator_abi_errors.py: every pointer is a fake non-null one or null, so a call that got past the checks would launch on it; an answer other
than CP_EINVAL, CP_EUNSUPPORTED, or CP_OK for an empty batch is refused and nothing is written.  tests/test_jvp2_host.py replays the file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from test_emulator_abi_errors_host import call, comes_back_early  # noqa: E402

ENTRIES = ['cp_mlp_jvp2', 'cp_taylor_jvp2']
RANGES = [(-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)]      # of M = 8
ROW_TILES = (2**31 - 1) * 64                  # rows of the largest grid
POINTERS = {'cp_mlp_jvp2': ['x', 'params', 'xoffset', 'xscale', 'yoffset', 'yscale', 'tan_u', 'value', 'out'],      # (tan_v, first_u, first_v: below)
            'cp_taylor_jvp2': ['x', 'center', 'powers', 'derivatives', 'tan_u', 'out']}
OPTIONAL = ['tan_v', 'first_u', 'first_v']
STRIDES = {'cp_mlp_jvp2': ['ldv', 'ldf', 'ldo'], 'cp_taylor_jvp2': ['ldo']}


def arguments(entry, B=4, ndim=3, widths=(5, 17), acts=0, M=8, yfunction=0, T=20, max_power=3, col0=0, ncols=8, K=2, null=(), **strides):
    """The argument list of ``entry`` in the fixture's notation; ``null``: names of POINTERS[entry] or OPTIONAL to pass as null, or 'all'."""
    p = {name: None if null == 'all' or name in null else 'ptr' for name in POINTERS[entry] + OPTIONAL}
    ld = lambda name: strides.get(name, 8)  # noqa: E731
    if entry == 'cp_mlp_jvp2':
        return [p['x'], B, ndim, len(widths), list(widths), None if acts is None else [acts] * len(widths), M, p['params'], p['xoffset'], p['xscale'], p['yoffset'], p['yscale'],
                yfunction, col0, ncols, p['tan_u'], p['tan_v'], K, p['value'], ld('ldv'), p['first_u'], p['first_v'], ld('ldf'), p['out'], ld('ldo'), 0, None]
    return [p['x'], B, p['center'], p['powers'], ndim, T, max_power, p['derivatives'], M, col0, ncols, p['tan_u'], p['tan_v'], K, p['out'], ld('ldo'), 0, None]


def table():
    """[(entry, what, arguments)]"""
    cases = []
    for entry in ENTRIES:
        mlp = entry == 'cp_mlp_jvp2'
        strides = STRIDES[entry]
        add = lambda what, **options: cases.append((entry, what, arguments(entry, **options)))  # noqa: E731
        for name in POINTERS[entry]:
            add('null d_' + name, null=(name,))
        add('B = -1', B=-1)
        add('B = 0, every pointer null', B=0, null='all')
        for ndim in (0, 33):
            add('ndim = %d' % ndim, ndim=ndim)
        for col0, ncols in RANGES:
            add('columns (%d, %d) of 8' % (col0, ncols), col0=col0, ncols=ncols, **{name: 16 for name in strides})
        for name in strides:
            add(name + ' one short', **{name: 7})
        for K in (0, -1):
            add('K = %d' % K, K=K)
        add('K = 2^31', B=1, K=2**31)
        for K in (1, 3, 64):
            add('one past the grid, K = %d' % K, B=ROW_TILES // K + 1, K=K)
            add('the grid full, every pointer null, K = %d' % K, B=ROW_TILES // K, K=K, null='all')
        add('B = 2^62', B=2**62)
        if mlp:
            for yfunction in (-1, 3):
                add('yfunction = %d' % yfunction, yfunction=yfunction)
            for widths in ((5, 65), (5, 0), (8,) * 9):
                add('widths %s' % (widths,), widths=widths)
            add('no activation codes', acts=None)
            # the first-order products: optional without a y function, needed with one; d_first_v belongs to d_tan_v
            add('d_first_v without d_tan_v', null=('tan_v',))
            add('d_first_v without d_tan_v, y function', null=('tan_v',), yfunction=1)
            for yfunction in (1, 2):
                add('y function %d without d_first_u' % yfunction, null=('first_u',), yfunction=yfunction)
                add('y function %d, d_tan_v without d_first_v' % yfunction, null=('first_v',), yfunction=yfunction)
                add('y function %d without both' % yfunction, null=('first_u', 'first_v'), yfunction=yfunction)
            add('ldf one short, no first-order products, no y function: B = 0', B=0, ldf=7, null=('first_u', 'first_v'))
            add('ldf one short, no first-order products, y function', ldf=7, null=('first_u', 'first_v'), yfunction=2)
        else:
            for max_power in (-1, 16):
                add('max_power = %d' % max_power, max_power=max_power)
            add('T = 0', T=0)
        # two faults at once: the first check in the order of the entry point answers
        add('B = -1 and a bad range', B=-1, col0=4, ncols=5)
        add('a bad range and ndim = 33', col0=4, ncols=5, ndim=33)
        add('a bad range and a short stride', col0=0, ncols=9, **{name: 7 for name in strides})
        add('a bad range, a short stride and K = 0', col0=0, ncols=0, K=0, **{name: -1 for name in strides})
        add('a short stride and K = 0', K=0, ldo=7)
        add('K = 0 and one past the grid', K=0, B=ROW_TILES + 1)
        add('K = 0 and a null pointer', K=0, null=('x',))
        if mlp:
            add('yfunction = 3 and a bad range', yfunction=3, col0=4, ncols=5)
            add('ldv and ldf short', ldv=7, ldf=6)
            add('ldf and ldo short', ldf=7, ldo=6)
        else:
            add('a short stride and ndim = 33', ldo=7, ndim=33)
            add('K = 0 and ndim = 33', K=0, ndim=33)
    return cases


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'jvp2_abi_errors.json'))
    args = parser.parse_args()
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    recorded = []
    for entry, what, arguments_ in table():
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
