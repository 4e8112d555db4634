"""CPU: the host half of the emulated engine -- the planning of column ranges (``column_runs``), ``EmulatedEngine.read`` (which loads nothing), and the
declarations of the two column-range entry points in the header and the bindings."""
import os
import re

import pytest

from conftest import ROOT
from cosmoprimo_amd import _lib
from cosmoprimo_amd.emulators import EmulatedEngine
from cosmoprimo_amd.emulators.tools import column_runs

KEYS = ['fourier.pk.delta_m.delta_m', 'fourier.pk.delta_m.theta_m', 'fourier.kz', 'primordial.n_eff', 'thermodynamics.rs_drag', 'thermodynamics.z_drag',
        'background.rho_ncdm', 'background.time', 'background.comoving_radial_distance']
SHAPES = [(4, 3), (4, 3), (2,), (), (), (), (0, 5), (5,), (5,)]      # columns 0-12, 12-24, 24-26, 26, 27, 28, none, 29-34, 34-39


def test_column_runs_of_one_section():
    assert column_runs(KEYS, SHAPES, 'background') == [(29, 39)]      # ('background.rho_ncdm' has no column)
    assert column_runs(KEYS, SHAPES, ['background']) == [(29, 39)]
    assert column_runs(KEYS, SHAPES, 'thermodynamics') == [(27, 29)]
    assert column_runs(KEYS, SHAPES, 'fourier') == [(0, 26)]
    assert column_runs(KEYS, SHAPES, ['fourier', 'primordial', 'thermodynamics', 'background']) == [(0, 39)]      # adjacent sections join
    assert column_runs(KEYS, SHAPES, 'primordial.n_eff') == [(26, 27)]


def test_column_runs_of_keys_that_are_not_adjacent():
    assert column_runs(KEYS, SHAPES, ['fourier.pk.delta_m.delta_m', 'background.time']) == [(0, 12), (29, 34)]
    assert column_runs(KEYS, SHAPES, ['background.time', 'fourier.pk.delta_m.delta_m']) == [(0, 12), (29, 34)]      # in the order of the columns
    assert column_runs(KEYS, SHAPES, ['fourier.pk.delta_m.delta_m', 'fourier.kz']) == [(0, 12), (24, 26)]
    assert column_runs(KEYS, SHAPES, ['fourier.pk.delta_m.theta_m', 'fourier.kz', 'fourier.pk']) == [(0, 26)]      # a key asked for twice counts once


def test_column_runs_unknown_and_empty():
    for keys in ('harmonic', ['background', 'harmonic'], ['background.age'], 'back', 'background.', ''):
        with pytest.raises(KeyError):
            column_runs(KEYS, SHAPES, keys)
    assert column_runs(KEYS, SHAPES, []) == []
    assert column_runs([], [], []) == []
    assert column_runs(KEYS, SHAPES, ['background.rho_ncdm']) == []      # known, without columns


def test_column_runs_prefix_stops_at_a_dot():
    keys, shapes = ['fourier.k', 'fourier.kz', 'fourier.k.z', 'fourierx.k'], [(2,), (3,), (4,), (5,)]
    assert column_runs(keys, shapes, 'fourier.k') == [(0, 2), (5, 9)]      # itself and 'fourier.k.z', not 'fourier.kz'
    assert column_runs(keys, shapes, 'fourier') == [(0, 9)]                # not 'fourierx.k'
    assert column_runs(keys, shapes, ['fourier.kz']) == [(2, 5)]


def test_read_returns_a_subclass_that_loads_nothing(tmp_path):
    fn = str(tmp_path / 'no_such_emulator.npy')
    Engine = EmulatedEngine.read(fn)
    assert issubclass(Engine, EmulatedEngine) and Engine is not EmulatedEngine
    assert Engine.path == fn and Engine.name == 'emulated' and EmulatedEngine.path is None
    assert getattr(Engine, '_emulator', None) is None      # nothing is loaded (the file does not even exist) until an engine is made
    assert EmulatedEngine.read(fn) is not Engine           # one class, and later one loaded emulator, per call
    with pytest.warns(DeprecationWarning):
        Deprecated = EmulatedEngine.load(fn)
    assert issubclass(Deprecated, EmulatedEngine) and Deprecated.path == fn
    from cosmoprimo_amd.cosmology import get_engine
    assert get_engine('emulated') is EmulatedEngine      # reading a file does not take the registered name over


def header_declarations():
    """{name: number of arguments} of the functions include/cosmoprimo_amd.h declares (the parsing of tests/test_lib_abi.py, with the argument lists)."""
    text = open(os.path.join(ROOT, 'include', 'cosmoprimo_amd.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {name: (0 if args.strip() == 'void' else args.count(',') + 1) for name, args in re.findall(r'\b(cp_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', text)}


def test_column_entry_points_are_declared_and_bound():
    declared = header_declarations()
    lib = _lib.load()
    for name, base in (('cp_mlp_predict_columns', 'cp_mlp_predict'), ('cp_taylor_predict_columns', 'cp_taylor_predict')):
        assert name in declared and hasattr(lib, name), name
        assert name in _lib.SIGNATURES, 'binding missing for {}'.format(name)
        assert len(_lib.SIGNATURES[name][1]) == declared[name] == declared[base] + 3      # col0, ncols, ldo
        assert len(_lib.SIGNATURES[base][1]) == declared[base]
    assert lib.cp_abi_version() == _lib.ABI_VERSION      # an added entry point does not move it
    # the ranges are judged before any device call: no device here
    for col0, ncols, ldo in ((-1, 4, 4), (0, 0, 4), (6, 3, 3), (0, 4, 3)):
        assert lib.cp_taylor_predict_columns(None, 4, None, None, 3, 5, 2, None, 8, col0, ncols, None, ldo, 0, None) == _lib.CP_EINVAL
        assert b'cp_taylor_predict_columns' in lib.cp_last_error()
    assert lib.cp_taylor_predict_columns(None, 0, None, None, 3, 5, 2, None, 8, 2, 4, None, 4, 0, None) == _lib.CP_OK
    import ctypes
    widths, acts = (ctypes.c_int * 1)(4), (ctypes.c_int * 1)(0)
    for col0, ncols, ldo in ((-1, 4, 4), (0, 0, 4), (6, 3, 3), (0, 4, 3)):
        assert lib.cp_mlp_predict_columns(None, 4, 3, 1, widths, acts, 8, None, None, None, None, None, 0, col0, ncols, None, ldo, 0, None) == _lib.CP_EINVAL
        assert b'cp_mlp_predict_columns' in lib.cp_last_error()
    assert lib.cp_mlp_predict_columns(None, 0, 3, 1, widths, acts, 8, None, None, None, None, None, 0, 2, 4, None, 4, 0, None) == _lib.CP_OK
