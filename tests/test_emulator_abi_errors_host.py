"""CPU: every refusal of the eight emulator entry points (cp_mlp_predict, cp_mlp_predict_columns, cp_mlp_jacobian, cp_mlp_vjp and their cp_taylor_*
counterparts) against tests/golden/emulator_abi_errors.json: status AND message of each bad call as the library answered before its entry points were
given one shared front (tools/gen_emulator_abi_errors.py holds the table of calls and wrote the file).  The calls with two faults at once pin the order of
the checks.  Every call passes fake non-null pointers and must come back before any device call, so the fixture may hold CP_EINVAL, CP_EUNSUPPORTED, or
CP_OK for an empty batch, and nothing else: that is asserted of the whole file before the first call is made."""
import ctypes
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'emulator_abi_errors.json')
ENTRIES = ['cp_mlp_predict', 'cp_mlp_predict_columns', 'cp_mlp_jacobian', 'cp_mlp_vjp', 'cp_taylor_predict', 'cp_taylor_predict_columns', 'cp_taylor_jacobian',
           'cp_taylor_vjp']
FAKE = 8      # a non-null pointer nobody reads


def call(lib, entry, args):
    """(status, message) of ``entry`` on ``args`` as the fixture writes them: 'ptr' a fake non-null pointer, None a null one, a list an int array, the
    rest integers.  The message is that of a refusal; '' for CP_OK."""
    status = getattr(lib, entry)(*[ctypes.c_void_p(FAKE) if a == 'ptr' else (ctypes.c_int * max(len(a), 1))(*a) if isinstance(a, list) else a for a in args])
    return status, lib.cp_last_error().decode('utf-8') if status else ''


def comes_back_early(case):
    """Is the recorded answer one that a call gives before it touches a device?  (args[1] is B for every entry.)"""
    from cosmoprimo_amd import _lib
    return case['status'] in (_lib.CP_EINVAL, _lib.CP_EUNSUPPORTED) or (case['status'] == _lib.CP_OK and case['args'][1] == 0)


@pytest.fixture(scope='module')
def cases():
    with open(FIXTURE) as file:
        cases = json.load(file)
    assert sorted({case['entry'] for case in cases}) == sorted(ENTRIES)
    late = [case for case in cases if not comes_back_early(case)]
    assert not late, late      # such a call would launch on fake pointers
    return cases


@pytest.mark.parametrize('entry', ENTRIES)
def test_status_and_message_of_every_refusal(cases, entry):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    mine = [case for case in cases if case['entry'] == entry]
    assert len(mine) >= 10
    wrong = []
    for case in mine:
        status, message = call(lib, entry, case['args'])
        if (status, message) != (case['status'], case['message']):
            wrong.append((case['what'], (status, message), (case['status'], case['message'])))
    assert not wrong, wrong
