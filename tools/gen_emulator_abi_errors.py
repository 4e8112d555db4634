"""Write tests/golden/emulator_abi_errors.json: (entry point, arguments, status, message) of every bad call in the table below, as the built library answers.

    python tools/gen_emulator_abi_errors.py [--out tests/golden/emulator_abi_errors.json]

Run on the CPU (no device is needed: every call comes back before its first device call) against the library whose answers are to be pinned.  Every
pointer is a fake non-null one or null, so a call that got past the checks would launch on it: an answer other than CP_EINVAL, CP_EUNSUPPORTED, or CP_OK
for an empty batch is refused and nothing is written.  For that reason the two predict entries' call beyond the grid is not in the table (it is refused
only at the launch).  tests/test_emulator_abi_errors_host.py replays the file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from test_emulator_abi_errors_host import ENTRIES, call, comes_back_early  # noqa: E402

BIG = 2**40                                   # a workspace nobody allocates
RANGES = [(-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)]      # of M = 8
ROW_TILES = (2**31 - 1) * 64                  # rows of the largest grid
POINTERS = {'cp_mlp_predict': ['x', 'params', 'xoffset', 'xscale', 'yoffset', 'yscale', 'out'],
            'cp_mlp_jacobian': ['x', 'params', 'xoffset', 'xscale', 'yoffset', 'yscale', 'value', 'jac'],
            'cp_mlp_vjp': ['x', 'params', 'xoffset', 'xscale', 'yoffset', 'yscale', 'cot', 'grad', 'work'],      # (a null d_value is no fault)
            'cp_taylor_predict': ['x', 'center', 'powers', 'derivatives', 'out'],
            'cp_taylor_jacobian': ['x', 'center', 'powers', 'derivatives', 'jac'],
            'cp_taylor_vjp': ['x', 'center', 'powers', 'derivatives', 'cot', 'grad', 'work']}
for _engine in ('mlp', 'taylor'):
    POINTERS['cp_%s_predict_columns' % _engine] = POINTERS['cp_%s_predict' % _engine]
STRIDES = {'predict_columns': ['ldo'], 'mlp_jacobian': ['ldv', 'ldj'], 'mlp_vjp': ['ldc', 'ldv'], 'taylor_jacobian': ['ldj'], 'taylor_vjp': ['ldc']}


def arguments(entry, B=4, ndim=3, widths=(5, 17), acts=0, M=8, yfunction=0, T=20, max_power=3, col0=0, ncols=8, work=BIG, null=(), **strides):
    """The argument list of ``entry`` in the fixture's notation; ``null``: names of POINTERS[entry] to pass as null, or 'all'."""
    p = {name: None if null == 'all' or name in null else 'ptr' for name in POINTERS[entry] + ['value']}
    ld = lambda name: strides.get(name, 8)  # noqa: E731
    mlp, kind = entry.startswith('cp_mlp'), entry.split('_', 2)[2]
    if mlp:
        head = [p['x'], B, ndim, len(widths), list(widths), None if acts is None else [acts] * len(widths), M, p['params'], p['xoffset'], p['xscale'], p['yoffset'],
                p['yscale'], yfunction]
    else:
        head = [p['x'], B, p['center'], p['powers'], ndim, T, max_power, p['derivatives'], M]
    tail = {'predict': [p.get('out')],
            'predict_columns': [col0, ncols, p.get('out'), ld('ldo')],
            'jacobian': [col0, ncols] + ([p['value'], ld('ldv')] if mlp else []) + [p.get('jac'), ld('ldj')],
            'vjp': [col0, ncols, p.get('cot'), ld('ldc')] + ([p['value'], ld('ldv')] if mlp else []) + [p.get('grad'), p.get('work'), work]}[kind]
    return head + tail + [0, None]


def table():
    """[(entry, what, arguments)]"""
    cases = []
    for entry in ENTRIES:
        mlp, kind = entry.startswith('cp_mlp'), entry.split('_', 2)[2]
        ranged = kind != 'predict'
        add = lambda what, **options: cases.append((entry, what, arguments(entry, **options)))  # noqa: E731
        for name in POINTERS[entry]:
            add('null d_' + name, null=(name,))
        add('B = -1', B=-1)
        add('B = 0, every pointer null', B=0, null='all', work=0)
        for ndim in (0, 33):
            add('ndim = %d' % ndim, ndim=ndim)
        strides = STRIDES.get(kind if kind == 'predict_columns' else entry[3:], [])
        if ranged:
            for col0, ncols in RANGES:
                add('columns (%d, %d) of 8' % (col0, ncols), col0=col0, ncols=ncols, **{name: 16 for name in strides})
        for name in strides:
            add(name + ' one short', **{name: 7})
        if mlp:
            for yfunction in (-1, 3):
                add('yfunction = %d' % yfunction, yfunction=yfunction)
            for widths in ((5, 65), (5, 0), (8,) * 9):
                add('widths %s' % (widths,), widths=widths)
            add('no activation codes', acts=None)
        else:
            for max_power in (-1, 16):
                add('max_power = %d' % max_power, max_power=max_power)
            add('T = 0', T=0)
        if kind in ('jacobian', 'vjp'):      # a row per point and parameter, but for the MLP's vjp: a row per point
            most = ROW_TILES if entry == 'cp_mlp_vjp' else ROW_TILES // 3
            add('one past the grid', B=most + 1)
            add('the grid full, every pointer null', B=most, null='all')
        if kind == 'vjp':
            need = 4 * (5 + 17) + 4 * 8 + 4 * 17 if mlp else 4 * 20
            add('workspace one short', work=need - 1)
            add('null d_x and a short workspace', null=('x',), work=need - 1)
        # two faults at once: the first check in the order of the entry point answers
        if ranged:
            add('B = -1 and a bad range', B=-1, col0=4, ncols=5)
            add('a bad range and ndim = 33', col0=4, ncols=5, ndim=33)
            add('a bad range and a short stride', col0=0, ncols=9, **{name: 7 for name in strides})
            if mlp:
                add('yfunction = 3 and a bad range', yfunction=3, col0=4, ncols=5)
    return cases


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'emulator_abi_errors.json'))
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
