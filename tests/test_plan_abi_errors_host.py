"""CPU: what the entry points of the plan types answer without touching a device -- every refusal of the ten constructors (cp_fftlog_plan_create on both
of its paths, cp_rfft_plan_create, cp_dst_plan_create, cp_spline_plan_create, cp_linop_plan_create, cp_spline_rows_plan_create, cp_splice_plan_create,
cp_interp_table_create, cp_geospline_plan_create and _create_prefiltered), the null-plan answers of their *_info / *_columns / *_law / *_scheme /
*_set_scheme entries (cp_splice_plan_info among them) and *_destroy(NULL) -- against tests/golden/plan_abi_errors.json: status AND message of each call as the library answered before
its plans were given one owner of their device tables (tools/gen_plan_abi_errors.py holds the table of calls and wrote the file).  The calls with two
faults at once pin the order of the checks.  Every constructor is called with an output pointer that holds garbage, and must leave it null on every
failure.

The cases marked ``valid`` are good calls with real host arrays.  Without a device they answer CP_EDEVICE, "<entry>: cannot select device 0", and leave
the plan pointer null; with a device they would build a plan, so the replay leaves them out there (and runs everything else).  Those of two
constructors are marked ``by_hand`` as well: before the change cp_spline_rows_plan_create and cp_splice_plan_create folded a failed device selection
into their placement failure (CP_ENOMEM, "cannot place the tables on device 0"); they now answer it as every other constructor does, and the file
holds that answer."""
import ctypes
import json
import os

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plan_abi_errors.json')
CONSTRUCTORS = ['cp_fftlog_plan_create', 'cp_rfft_plan_create', 'cp_dst_plan_create', 'cp_spline_plan_create', 'cp_linop_plan_create',
                'cp_spline_rows_plan_create', 'cp_splice_plan_create', 'cp_interp_table_create', 'cp_geospline_plan_create',
                'cp_geospline_plan_create_prefiltered']
OTHERS = ['cp_fftlog_plan_info', 'cp_spline_plan_info', 'cp_spline_plan_columns', 'cp_spline_rows_plan_info', 'cp_geospline_plan_info', 'cp_interp_table_law',
          'cp_splice_plan_scheme', 'cp_splice_plan_set_scheme', 'cp_splice_plan_info', 'cp_fftlog_plan_destroy', 'cp_rfft_plan_destroy', 'cp_dst_plan_destroy', 'cp_spline_plan_destroy',
          'cp_spline_rows_plan_destroy', 'cp_splice_plan_destroy', 'cp_interp_table_destroy', 'cp_geospline_plan_destroy']
GARBAGE = 0x5a5a5a50      # what the plan pointer holds before a constructor is called


def wallish_knots():
    """(knots, piece_src, piece_start, piece_count, queries) of the spliced spline of the wallish2018 filter: 3 051 of 3 666 knots on a uniform grid."""
    k, klin = np.geomspace(1e-7, 1e2, 1024), np.linspace(1e-7, 2., 4096)
    mask, left, right = (klin > 1e-2) & (klin < 1.5), k < 5e-4, k > 2.
    knots = np.concatenate([k[left], klin[mask], k[right]])
    return knots, [0, 1, 0], [0, int(np.flatnonzero(mask)[0]), int(np.flatnonzero(right)[0])], [int(left.sum()), int(mask.sum()), int(right.sum())], k


NAMED = {'wallish_knots': lambda: wallish_knots()[0], 'wallish_src': lambda: wallish_knots()[1], 'wallish_start': lambda: wallish_knots()[2],
         'wallish_count': lambda: wallish_knots()[3], 'wallish_queries': lambda: wallish_knots()[4],
         'irregular': lambda: np.cumsum(1. + 0.5 * np.sin(np.arange(64.)))}


def convert(arg, keep):
    """An argument as the fixture writes it -> ctypes: 'out' a plan pointer holding GARBAGE, None a null pointer, {'linspace' / 'geomspace': [first,
    last, n]}, {'ones': n}, {'doubles': [...]}, {'named': name of NAMED} host arrays of doubles, {'ints': [...]} (or a named list of integers) a host
    array of int, the rest integers."""
    if arg == 'out':
        keep.append(ctypes.c_void_p(GARBAGE))
        return ctypes.byref(keep[-1])
    if isinstance(arg, dict):
        (kind, value), = arg.items()
        if kind == 'named':
            value = NAMED[value]()
            kind = 'ints' if isinstance(value, list) else 'doubles'
        if kind == 'ints':
            keep.append((ctypes.c_int * len(value))(*value))
            return keep[-1]
        array = {'linspace': lambda: np.linspace(*value), 'geomspace': lambda: np.geomspace(*value), 'ones': lambda: np.ones(value),
                 'doubles': lambda: np.array(value, dtype='f8')}[kind]()
        keep.append(np.ascontiguousarray(array, dtype='f8'))
        return keep[-1].ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return arg


def call(lib, entry, args):
    """(status, message, what a constructor left in the plan pointer: None for null) of ``entry`` on ``args``.  The message is that of a refusal; '' for CP_OK."""
    keep = []
    converted = [convert(a, keep) for a in args]
    status = getattr(lib, entry)(*converted)
    out = keep[0].value if args and args[0] == 'out' else None
    return status, lib.cp_last_error().decode('utf-8') if status else '', out


@pytest.fixture(scope='module')
def cases():
    from cosmoprimo_amd import _lib
    with open(FIXTURE) as file:
        cases = json.load(file)
    assert sorted({case['entry'] for case in cases}) == sorted(CONSTRUCTORS + OTHERS)
    # no call of the file may reach a device unless it is marked valid: a refusal, or CP_OK from an entry that builds nothing
    late = [case for case in cases if not case.get('valid') and not (case['status'] in (_lib.CP_EINVAL, _lib.CP_EUNSUPPORTED) or
                                                                    (case['status'] == _lib.CP_OK and case['entry'] in OTHERS))]
    assert not late, late
    for case in cases:
        if case.get('valid'):
            assert (case['status'], case['entry'] in CONSTRUCTORS) == (_lib.CP_EDEVICE, True) and case['message'].endswith(': cannot select device 0'), case
    if _lib.load().cp_device_count() > 0:      # a good call would build a plan here
        cases = [case for case in cases if not case.get('valid')]
    return cases


@pytest.mark.parametrize('entry', CONSTRUCTORS + OTHERS)
def test_status_and_message_of_every_answer(cases, entry):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    with open(FIXTURE) as file:
        recorded = [case for case in json.load(file) if case['entry'] == entry]
    if entry in CONSTRUCTORS:
        assert len(recorded) >= 8 and any(case.get('valid') for case in recorded)
    wrong = []
    for case in [case for case in cases if case['entry'] == entry]:
        status, message, out = call(lib, entry, case['args'])
        if (status, message) != (case['status'], case['message']) or (entry in CONSTRUCTORS and case['args'][0] == 'out' and out is not None):
            wrong.append((case['what'], (status, message, out), (case['status'], case['message'])))
    assert not wrong, wrong
