"""CPU: every refusal of cp_mlp_vjp2 and cp_taylor_vjp2 against tests/golden/vjp2_abi_errors.json: status AND message of each bad call as the library
answered when the entry points were written (tools/gen_vjp2_abi_errors.py holds the table of calls and wrote the file): null pointers, B < 0, B = 0 with
null pointers, ndim 0 / 33, column ranges, strides, a short workspace, the row cap, and calls with two faults at once, which pin the order of the checks --
that of the engine's vjp.  Every call passes fake non-null pointers and must come back before any device call, so the fixture may hold CP_EINVAL,
CP_EUNSUPPORTED, or CP_OK for an empty batch, and nothing else: that is asserted of the whole file before the first call is made.  The workspace sizes are
pinned here as well."""
import ctypes
import json
import os

import pytest

from test_emulator_abi_errors_host import call, comes_back_early

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'vjp2_abi_errors.json')
ENTRIES = ['cp_mlp_vjp2', 'cp_taylor_vjp2']


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
    assert len(mine) >= 25
    wrong = []
    for case in mine:
        status, message = call(lib, entry, case['args'])
        if (status, message) != (case['status'], case['message']):
            wrong.append((case['what'], (status, message), (case['status'], case['message'])))
    assert not wrong, wrong


def test_workspace_sizes():
    """cp_mlp_vjp2_workspace_doubles: that of cp_mlp_vjp, and with a y function the Gauss-Newton workspace, its result (B, ndim, ndim) and omega (B, ncols) on
    top; cp_taylor_vjp2_workspace_doubles = B T; minus the status on an error."""
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    widths = (ctypes.c_int * 2)(5, 17)
    for B, ncols in ((4, 8), (4, 2), (70, 8), (0, 8)):
        plain = lib.cp_mlp_vjp_workspace_doubles(B, 3, 2, widths, 8, ncols)
        assert lib.cp_mlp_vjp2_workspace_doubles(B, 3, 2, widths, 8, ncols, 0) == plain
        for yfunction in (1, 2):
            assert lib.cp_mlp_vjp2_workspace_doubles(B, 3, 2, widths, 8, ncols, yfunction) == \
                plain + lib.cp_mlp_gauss_newton_workspace_doubles(B, 3, 2, widths, 8, ncols) + B * 9 + B * ncols
    for bad in ((-1, 3, 8, 8, 0), (4, 0, 8, 8, 0), (4, 33, 8, 8, 0), (4, 3, 0, 8, 0), (4, 3, 8, 0, 0), (4, 3, 8, 9, 0), (4, 3, 8, 8, -1), (4, 3, 8, 8, 3)):
        assert lib.cp_mlp_vjp2_workspace_doubles(bad[0], bad[1], 2, widths, bad[2], bad[3], bad[4]) < 0
    assert lib.cp_mlp_vjp2_workspace_doubles((2**31 - 1) * 64 // 6 + 1, 3, 2, widths, 8, 8, 0) == -_lib.CP_EUNSUPPORTED
    assert lib.cp_taylor_vjp2_workspace_doubles(4, 20) == 80 and lib.cp_taylor_vjp2_workspace_doubles(-1, 20) == -_lib.CP_EINVAL
    assert lib.cp_taylor_vjp2_workspace_doubles(4, 0) == -_lib.CP_EINVAL
