"""Write tests/golden/plan_abi_errors.json: (entry point, arguments, status, message) of every call in the table below, as the built library answers.

    python tools/gen_plan_abi_errors.py [--out tests/golden/plan_abi_errors.json]

Run on a machine WITHOUT a device against the library whose answers are to be pinned (COSMOPRIMO_AMD_LIBRARY names another build than the tree's): the
good calls (``valid``) must end in the device selection there, CP_EDEVICE "...: cannot select device 0" with the plan pointer null.  A constructor whose
good call the library answers otherwise is written ``by_hand`` with that answer (and the library's own is printed); any other call that does not come
back CP_EINVAL / CP_EUNSUPPORTED (or CP_OK from an entry that builds nothing), or that leaves something in the plan pointer, ends the run with nothing
written.  tests/test_plan_abi_errors_host.py replays the file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from test_plan_abi_errors_host import CONSTRUCTORS, OTHERS, call  # noqa: E402

ONES = lambda n: {'ones': n}  # noqa: E731
GEOM = lambda *a: {'geomspace': list(a)}  # noqa: E731
LIN = lambda *a: {'linspace': list(a)}  # noqa: E731
W = lambda name: {'named': 'wallish_' + name}  # noqa: E731
# entry -> [(argument, value of a good call)]
GOOD = {
    'cp_fftlog_plan_create': [('out', 'out'), ('n', 128), ('npad', 256), ('nker', 1), ('pre', ONES(256)), ('post', ONES(256)), ('u', ONES(258)), ('device', 0)],
    'cp_rfft_plan_create': [('out', 'out'), ('size', 256), ('device', 0)],
    'cp_dst_plan_create': [('out', 'out'), ('n', 256), ('kx', GEOM(1e-3, 10., 256)), ('device', 0)],
    'cp_spline_plan_create': [('out', 'out'), ('n', 64), ('x', LIN(0., 1., 64)), ('nq', 256), ('xq', LIN(0., 1., 256)), ('bc', 0), ('nu', 0), ('extrapolate', 0),
                              ('device', 0)],
    'cp_linop_plan_create': [('out', 'out'), ('n', 8), ('nq', 8), ('w', ONES(64)), ('device', 0)],
    'cp_spline_rows_plan_create': [('out', 'out'), ('n', 128), ('x', LIN(0., 1., 128)), ('bc', 0), ('extrapolate', 0), ('nq', 64), ('xq', LIN(0.1, 0.9, 64)),
                                   ('device', 0)],
    'cp_splice_plan_create': [('out', 'out'), ('nknots', 3666), ('x', W('knots')), ('npieces', 3), ('piece_src', W('src')), ('piece_start', W('start')),
                              ('piece_count', W('count')), ('nq', 1024), ('xq', W('queries')), ('device', 0)],
    'cp_interp_table_create': [('out', 'out'), ('n', 64), ('x', LIN(0., 1., 64)), ('f', ONES(64)), ('device', 0)],
    'cp_geospline_plan_create': [('out', 'out'), ('knots', GEOM(1e-2, 1e2, 1024)), ('n', 1024), ('queries', GEOM(1., 10., 64)), ('nq', 64), ('device', 0)],
    'cp_geospline_plan_create_prefiltered': [('out', 'out'), ('n', 1024), ('npad', 2048), ('pre', ONES(2048)), ('post', GEOM(1., 100., 2048)), ('u', ONES(2050)),
                                             ('knots', GEOM(1e-2, 1e2, 1024)), ('queries', GEOM(1., 10., 64)), ('nq', 64), ('device', 0)],
}
# the constructors that select the device inside another one answer under its name
SELECTS = {'cp_linop_plan_create': 'cp_spline_plan_create', 'cp_geospline_plan_create_prefiltered': 'cp_fftlog_plan_create'}
DECREASING = {'doubles': [0., 1., 2., 1.5, 3., 4., 5., 6.]}
# entry -> [(what, {argument: value}, valid)]; two faults at once: the first check in the order of the entry point answers
CALLS = {
    'cp_fftlog_plan_create': [
        ('a good call', {}, True), ('a good call of the large-size path', dict(n=8192, npad=16384, pre=ONES(16384), post=ONES(16384), u=ONES(16386)), True),
        ('null out', dict(out=None)), ('null pre', dict(pre=None)), ('null post', dict(post=None)), ('null u', dict(u=None)), ('n = 1', dict(n=1)),
        ('nker = 0', dict(nker=0)), ('npad = 100', dict(npad=100)), ('npad = 64 < n', dict(npad=64)), ('npad = 2^25', dict(npad=1 << 25)),
        ('2^15 kernels of 2^14', dict(nker=1 << 15, npad=1 << 14)), ('n = npad = 2', dict(n=2, npad=2)), ('null out and n = 1', dict(out=None, n=1)),
        ('null pre and n = 1', dict(pre=None, n=1)), ('n = 1 and npad = 100', dict(n=1, npad=100)), ('npad = 100 and nker = 0', dict(npad=100, nker=0)),
        ('npad = 2^25 and 2^4 kernels', dict(npad=1 << 25, nker=16))],
    'cp_rfft_plan_create': [
        ('a good call', {}, True), ('a good call of the largest size', dict(size=16384), True), ('null out', dict(out=None)), ('size = 4', dict(size=4)),
        ('size = 32768', dict(size=32768)), ('size = 100', dict(size=100)), ('size = 0', dict(size=0)), ('size = -8', dict(size=-8)),
        ('null out and size = 4', dict(out=None, size=4))],
    'cp_dst_plan_create': [
        ('a good call', {}, True), ('a good call without the abscissa', dict(kx=None), True), ('a good call of 1024', dict(n=1024, kx=GEOM(1e-3, 10., 1024)), True),
        ('null out', dict(out=None)), ('n = 0', dict(n=0)), ('n = 512', dict(n=512)), ('n = 8192', dict(n=8192)), ('n = -256', dict(n=-256)),
        ('null out and n = 512', dict(out=None, n=512))],
    'cp_spline_plan_create': [
        ('a good call', {}, True), ('a good call, clamped first derivative', dict(bc=1, nu=1), True), ('null out', dict(out=None)), ('nq = 0', dict(nq=0)),
        ('2^15 x 2^15 weights', dict(n=1 << 15, nq=1 << 15)), ('n = 1', dict(n=1)), ('null x', dict(x=None)), ('null xq', dict(xq=None)), ('nu = 3', dict(nu=3)),
        ('bc = 99', dict(bc=99)), ('knots that decrease', dict(n=8, x=DECREASING)), ('not-a-knot through 3 knots', dict(n=3, bc=2)),
        ('nq = 0 and null x', dict(nq=0, x=None)), ('nu = 3 and n = 1', dict(nu=3, n=1)), ('nu = 3 and bc = 99', dict(nu=3, bc=99)),
        ('bc = 99 and knots that decrease', dict(bc=99, n=8, x=DECREASING)), ('null out and nq = 0', dict(out=None, nq=0))],
    'cp_linop_plan_create': [
        ('a good call', {}, True), ('null out', dict(out=None)), ('n = 0', dict(n=0)), ('nq = 0', dict(nq=0)), ('n = -1', dict(n=-1)), ('null w', dict(w=None)),
        ('2^15 x 2^15 weights', dict(n=1 << 15, nq=1 << 15)), ('null out and n = 0', dict(out=None, n=0)), ('null w and 2^15 x 2^15 weights', dict(w=None, n=1 << 15, nq=1 << 15))],
    'cp_spline_rows_plan_create': [
        ('a good call', {}, True), ('a good call, not-a-knot', dict(bc=2), True), ('null out', dict(out=None)), ('n = 3', dict(n=3)), ('null x', dict(x=None)),
        ('nq = 0', dict(nq=0)), ('null xq', dict(xq=None)), ('nq = 2^26 + 1', dict(nq=(1 << 26) + 1)), ('n = 2^26 + 1', dict(n=(1 << 26) + 1)), ('bc = 7', dict(bc=7)),
        ('knots that decrease', dict(n=8, x=DECREASING)), ('not-a-knot through 4 knots', dict(n=4, bc=2)), ('bc = 7 and knots that decrease', dict(bc=7, n=8, x=DECREASING)),
        ('n = 3 and bc = 7', dict(n=3, bc=7)), ('nq = 2^26 + 1 and bc = 7', dict(nq=(1 << 26) + 1, bc=7)), ('null out and n = 3', dict(out=None, n=3))],
    'cp_splice_plan_create': [
        ('a good call (knots with a uniform stretch)', {}, True),
        ('a good call (geometric knots)', dict(nknots=700, x=GEOM(1e-4, 1., 700), npieces=1, piece_src={'ints': [0]}, piece_start={'ints': [0]}, piece_count={'ints': [700]},
                                               nq=300, xq=GEOM(2e-4, 0.9, 300)), True),
        ('null out', dict(out=None)), ('nknots = 3', dict(nknots=3)), ('null x', dict(x=None)), ('npieces = 0', dict(npieces=0)), ('npieces = 4', dict(npieces=4)),
        ('null piece_src', dict(piece_src=None)), ('nq = 0', dict(nq=0)), ('null xq', dict(xq=None)), ('nknots = 2^24 + 1', dict(nknots=(1 << 24) + 1)),
        ('a piece of a third array', dict(piece_src={'ints': [0, 2, 0]})), ('a piece that starts at -1', dict(piece_start={'ints': [0, -1, 0]})),
        ('pieces of 3665 knots', dict(piece_count={'ints': [1, 3051, 613]})),
        ('knots that decrease', dict(nknots=8, x=DECREASING, npieces=1, piece_src={'ints': [0]}, piece_start={'ints': [0]}, piece_count={'ints': [8]})),
        ('a piece of a third array and knots that decrease', dict(nknots=8, x=DECREASING, npieces=1, piece_src={'ints': [2]}, piece_start={'ints': [0]}, piece_count={'ints': [8]})),
        ('nknots = 2^24 + 1 and a piece of a third array', dict(nknots=(1 << 24) + 1, piece_src={'ints': [0, 2, 0]})),
        ('null out and nknots = 3', dict(out=None, nknots=3))],
    'cp_interp_table_create': [
        ('a good call (uniform knots)', {}, True), ('a good call (irregular knots)', dict(x={'named': 'irregular'}), True), ('null out', dict(out=None)), ('n = 0', dict(n=0)),
        ('null x', dict(x=None)), ('null f', dict(f=None)), ('n = 2^27 + 1', dict(n=(1 << 27) + 1)), ('knots that decrease', dict(n=8, x=DECREASING)),
        ('null out and n = 0', dict(out=None, n=0)), ('n = 0 and null x', dict(n=0, x=None)), ('n = 2^27 + 1 and null f', dict(n=(1 << 27) + 1, f=None))],
    'cp_geospline_plan_create': [
        ('a good call', {}, True), ('null out', dict(out=None)), ('null knots', dict(knots=None)), ('null queries', dict(queries=None)), ('n = 3', dict(n=3)),
        ('nq = 0', dict(nq=0)), ('nq = 513', dict(nq=513)), ('uniform knots', dict(knots=LIN(1., 2., 1024))), ('knots from zero', dict(knots=LIN(0., 2., 1024))),
        ('no query inside the knots', dict(queries=GEOM(1e3, 1e4, 64))), ('queries next to the first knot', dict(queries=GEOM(1.01e-2, 10., 64))),
        ('nq = 513 and uniform knots', dict(nq=513, knots=LIN(1., 2., 1024))), ('uniform knots and no query inside', dict(knots=LIN(1., 2., 1024), queries=GEOM(1e3, 1e4, 64))),
        ('null out and n = 3', dict(out=None, n=3))],
    'cp_geospline_plan_create_prefiltered': [
        ('a good call', {}, True), ('null out', dict(out=None)), ('null pre', dict(pre=None)), ('null knots', dict(knots=None)), ('nq = 0', dict(nq=0)),
        ('512 samples padded to 1024', dict(n=512, npad=1024)), ('npad = 4096', dict(npad=4096)), ('nq = 513', dict(nq=513)), ('uniform knots', dict(knots=LIN(1., 2., 1024))),
        ('a postfactor from zero', dict(post=LIN(0., 1., 2048))), ('a uniform postfactor', dict(post=LIN(1., 2., 2048))),
        ('no query inside the knots', dict(queries=GEOM(1e3, 1e4, 64))), ('queries next to the first knot', dict(queries=GEOM(1.01e-2, 10., 64))),
        ('npad = 4096 and nq = 513', dict(npad=4096, nq=513)), ('nq = 513 and uniform knots', dict(nq=513, knots=LIN(1., 2., 1024))),
        ('uniform knots and a uniform postfactor', dict(knots=LIN(1., 2., 1024), post=LIN(1., 2., 2048))), ('null out and npad = 4096', dict(out=None, npad=4096))],
}
# (entry, what, arguments as they are): the entries that take a plan, on a null one
NULL_PLAN = [('cp_fftlog_plan_info', 'null plan', [None, 4, None, None, None]), ('cp_spline_plan_info', 'null plan', [None, None, None, None]),
             ('cp_spline_plan_columns', 'null plan', [None, None, None]), ('cp_spline_rows_plan_info', 'null plan', [None, None, None, None, None]),
             ('cp_geospline_plan_info', 'null plan', [None, None, None, None]), ('cp_interp_table_law', 'null table', [None, None, None]),
             ('cp_splice_plan_scheme', 'null plan (scheme 0)', [None]), ('cp_splice_plan_set_scheme', 'null plan', [None, 0]),
             ('cp_splice_plan_set_scheme', 'null plan and scheme 5', [None, 5]), ('cp_splice_plan_info', 'null plan', [None, None, None])] + [(entry, 'destroy(NULL)', [None]) for entry in OTHERS if entry.endswith('_destroy')]


def table():
    """[(entry, what, arguments, valid)]"""
    cases = []
    for entry in CONSTRUCTORS:
        names = [name for name, _ in GOOD[entry]]
        for what, options, *valid in CALLS[entry]:
            assert not set(options) - set(names), (entry, what)
            cases.append((entry, what, [options.get(name, value) for name, value in GOOD[entry]], bool(valid)))
    return cases + [(entry, what, arguments, False) for entry, what, arguments in NULL_PLAN]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'plan_abi_errors.json'))
    args = parser.parse_args()
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    if lib.cp_device_count() > 0:
        sys.exit('this machine has a device: the good calls would build plans; nothing written')
    recorded = []
    for entry, what, arguments, valid in table():
        status, message, out = call(lib, entry, arguments)
        case = {'entry': entry, 'what': what, 'args': arguments, 'status': status, 'message': message}
        if out is not None:
            sys.exit('%s, %s: the plan pointer holds %#x behind status %d; nothing written' % (entry, what, out, status))
        if valid:
            case['valid'] = True
            expected = (_lib.CP_EDEVICE, '%s: cannot select device 0' % SELECTS.get(entry, entry))
            if (status, message) != expected:
                print('%s, %s: the library answers %d (%s); written by hand as %d (%s)' % ((entry, what, status, message) + expected))
                case['status'], case['message'] = expected
                case['by_hand'] = True
        elif not (status in (_lib.CP_EINVAL, _lib.CP_EUNSUPPORTED) or (status == _lib.CP_OK and entry in OTHERS)):
            sys.exit('%s, %s: status %d (%s) -- this call got past the checks; nothing written' % (entry, what, status, message))
        recorded.append(case)
    with open(args.out, 'w') as file:
        file.write('[\n' + ',\n'.join(json.dumps(case) for case in recorded) + '\n]\n')
    print('%d calls written to %s (%d by hand); per entry: %s' % (len(recorded), args.out, sum('by_hand' in case for case in recorded),
                                                                   {entry: sum(case['entry'] == entry for case in recorded) for entry in CONSTRUCTORS + OTHERS}))


if __name__ == '__main__':
    main()
