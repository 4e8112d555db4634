"""CPU: every refusal of the entry points that take a batch of cosmologies of an analytic engine (the eleven of ENTRIES[:11]), of cp_wallish_tail and of
the two background entries that share their massive-neutrino argument, against tests/golden/analytic_abi_errors.json: status AND message of each bad
call as the library answered before these entry points were given one shared front (tools/gen_analytic_abi_errors.py holds the table of calls and wrote
the file).  The calls with two faults at once pin the order of the checks.  Cases marked ``by_hand`` are the ones the library before that change could
not answer without a device (it looked at the neutrino tables, at cp_power_eval's workspace and launch size and, on the fused sigma(r, z) routes, at the
engine only behind the device selection; in cp_sigma_rz_analytic / _prefiltered the tables are now looked at in front of the plans): their answers
were written from its strings, with the public entry's name in front.

Every device pointer is a fake non-null one, so a call that got past the checks would launch on it; ``bg_params`` / ``pk_params`` / ``cp_ncdm`` are
real host arrays and structs, because a front may read them before it selects a device.  The fixture may hold CP_EINVAL, CP_EUNSUPPORTED, or CP_OK for an
empty batch, and nothing else: that is asserted of the whole file before the first call is made.  On a machine WITH a device a lost check would launch
on the fake pointers instead of ending in CP_EDEVICE, so the replay skips itself there."""
import ctypes
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'analytic_abi_errors.json')
ENTRIES = ['cp_power_eval', 'cp_power_eval_variants', 'cp_variants_scalars', 'cp_eh_scalars', 'cp_sigma_rz_analytic', 'cp_sigma_rz_analytic_prefiltered',
           'cp_sigma_rz_functional', 'cp_sigma8_normalise', 'cp_dst_forward_analytic', 'cp_dst_forward_analytic_box', 'cp_wallish_full', 'cp_wallish_tail',
           'cp_growth_ode_tables', 'cp_background_eval']
FAKE = 64      # a non-null pointer nobody reads
# position of the sizes of which a zero makes the call an empty one (CP_OK with every pointer null)
EMPTY_AT = {'cp_power_eval': (2, 7), 'cp_power_eval_variants': (2, 7, 9), 'cp_variants_scalars': (0,), 'cp_eh_scalars': (0,), 'cp_sigma_rz_analytic': (1,),
            'cp_sigma_rz_analytic_prefiltered': (1,), 'cp_sigma_rz_functional': (1,), 'cp_sigma8_normalise': (1,), 'cp_dst_forward_analytic': (2,),
            'cp_dst_forward_analytic_box': (2,), 'cp_wallish_full': (3,), 'cp_wallish_tail': (5,), 'cp_growth_ode_tables': (0,), 'cp_background_eval': (0, 1)}


class DstPlan(ctypes.Structure):
    """The head of cp_dst_plan (csrc/cp_dst.hip), which the transform's entries look at before they select a device: length, device, four device tables."""
    _fields_ = [('n', ctypes.c_int), ('device', ctypes.c_int)] + [(name, ctypes.c_void_p) for name in ('d_tw', 'd_rot', 'd_kx', 'd_ln_kx')]


def convert(arg, keep):
    """An argument as the fixture writes it -> ctypes: 'ptr' a fake non-null pointer, None a null one, 'bg' / 'pk' host arrays of cp_param,
    {'ncdm': [nspecies, species, 'ptr' or None]} a host cp_ncdm, {'dst_plan': [n, with abscissa]} a host DstPlan, {'param': value} a cp_param by
    value, the rest integers."""
    from cosmoprimo_amd import _lib
    if arg == 'ptr':
        return ctypes.c_void_p(FAKE)
    if arg in ('bg', 'pk'):
        values = [0.7, 0.25, 0.05, 0., 2.7255, 3.044, -1., 0.] if arg == 'bg' else [2e-9, 0.96, 0., 0., 0.05]
        keep.append((_lib.cp_param * len(values))(*[_lib.cp_param(None, v) for v in values]))
        return ctypes.cast(keep[-1], ctypes.c_void_p)
    if isinstance(arg, dict) and 'ncdm' in arg:
        nspecies, species, tab = arg['ncdm']
        keep.append(_lib.cp_ncdm(nspecies, species, FAKE if tab else None))
        return ctypes.cast(ctypes.pointer(keep[-1]), ctypes.c_void_p)
    if isinstance(arg, dict) and 'dst_plan' in arg:
        n, kx = arg['dst_plan']
        keep.append(DstPlan(n, 0, FAKE, FAKE, FAKE if kx else None, FAKE if kx else None))
        return ctypes.cast(ctypes.pointer(keep[-1]), ctypes.c_void_p)
    if isinstance(arg, dict):
        return _lib.cp_param(None, arg['param'])
    return arg


def call(lib, entry, args):
    """(status, message) of ``entry`` on ``args``.  The message is that of a refusal; '' for CP_OK."""
    keep = []
    status = getattr(lib, entry)(*[convert(a, keep) for a in args])
    return status, lib.cp_last_error().decode('utf-8') if status else ''


def comes_back_early(case):
    """Is the recorded answer one that a call gives before it touches a device?  (CP_OK: only where a size of the call is zero.)"""
    from cosmoprimo_amd import _lib
    empty = any(case['args'][i] == 0 for i in EMPTY_AT[case['entry']])
    return case['status'] in (_lib.CP_EINVAL, _lib.CP_EUNSUPPORTED) or (case['status'] == _lib.CP_OK and empty)


@pytest.fixture(scope='module')
def cases():
    from cosmoprimo_amd import _lib
    if _lib.load().cp_device_count() > 0:
        pytest.skip('with a device a lost check would launch on fake pointers: this replay is for machines without one')
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
