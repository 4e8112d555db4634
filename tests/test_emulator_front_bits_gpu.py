"""GPU: the results of the emulator entry points, bit for bit, against tests/golden/emulator_front_bits.npz -- what the library and the engines gave before
the entry points were put behind one shared front (recorded on an MI355X by tools/gen_emulator_front_bits.py, every call run twice there and refused if
its two runs differed).  That change touched no kernel and no launch argument, and the kernels use no atomics and sum in a fixed order, so every output
must be EQUAL: a tolerance would not see a dispatch that picks sinh for 10^v on a near-linear range, or one that passes ldo where ncols belongs.

The inputs come from seeded numpy (tests/vjp_reference.py), so the file holds outputs only.  The shapes are the smallest that cross each boundary the host
code steers: B = 65 is two row tiles of 64, M = 260 two column tiles of 256, the range (250, 260) crosses that edge, the last hidden widths 16, 17, 33, 49
are the four instances of the dh kernel, the y functions none / log10 / arcsinh / log10 across them every instance of the forward and tangent kernels.
A value is stored once: the range (250, 260) as cp_*_predict_columns writes it (into rows of stride 12), the full (65, 260) predict (135 KB) of the
width-17 network and of the polynomial only.  The values that jacobian and vjp return beside their results -- on (250, 260), and for vjp on (0, 260) too,
in every case -- must equal those arrays and are compared with them here, not stored again; where the full predict is not stored, the value of the vjp
on (0, 260) is compared with ``predict(X)`` of this run, whose columns (250, 260) are the pinned ones.  Likewise Emulator.jacobian and Emulator.vjp
return their values, which must equal Emulator.predict's.  The file holds one flat float64 array per test and the names and shapes of the entries in it."""
import ctypes
import os

import numpy as np
import pytest

import mlp_reference as mr
import vjp_reference as vr
from test_emulator_jacobian_gpu import NAMES, XGRID, batch, emulators  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'emulator_front_bits.npz')
B, M, RANGE, PAD = 65, 260, (250, 260), -7.
MLP_CASES = [(16, ''), (17, 'log10'), (33, 'arcsinh'), (49, 'log10')]      # last hidden width (one per NJ of the dh kernel), y function


def _device():
    import torch
    return torch.device('cuda', 0)


def _up(array):
    import torch
    return torch.as_tensor(np.ascontiguousarray(array), device=_device())


def _stream():
    import torch
    return torch.cuda.current_stream(_device()).cuda_stream


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _padded(cot, extra=3):
    """``cot`` as a view of a buffer whose rows are ``extra`` longer."""
    import torch
    big = torch.full((cot.shape[0], cot.shape[1] + extra), PAD, dtype=torch.float64, device=_device())
    big[:, :cot.shape[1]] = _up(cot)
    return big[:, :cot.shape[1]]


def _same(a, b):
    return np.array_equal(np.asarray(a.cpu() if hasattr(a, 'cpu') else a), np.asarray(b.cpu() if hasattr(b, 'cpu') else b))


def _engine_entries(engine, X, cot, ranged, store_predict):
    """jacobian and vjp on RANGE, each with its value, which is ``ranged`` (B, 10), what cp_*_predict_columns wrote; vjp on (0, M) with its value, which is
    ``predict(X)`` (stored where ``store_predict``; its columns RANGE are ``ranged``), and once more without a value (a null d_value: a path of its own in
    the MLP's kernel), which gives the same gradient; the cotangents have a row stride of ncols + 3."""
    out = {}
    value, out['jacobian'] = engine.jacobian(X, columns=RANGE, return_value=True)
    assert _same(value, ranged)
    value, out['vjp'] = engine.vjp(X, _padded(cot[:, RANGE[0]:RANGE[1]]), columns=RANGE, return_value=True)
    assert _same(value, ranged)
    predict = engine.predict(X)
    assert tuple(predict.shape) == (B, M) and _same(predict[:, RANGE[0]:RANGE[1]], ranged)
    value, out['vjp_full'] = engine.vjp(X, _padded(cot), columns=(0, M), return_value=True)
    assert _same(value, predict)
    assert _same(engine.vjp(X, _padded(cot), columns=(0, M)), out['vjp_full'])
    if store_predict:
        out['predict'] = predict
    return out


def mlp_entries(H, yfunction):
    import torch
    from cosmoprimo_amd import _lib
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    lib = _lib.load()
    cfg = vr.mlp_config(B=B, widths=(5, H), M=M, activations=['tanh', 'silu'], yfunction=yfunction, seed=H)
    engine = MLPEmulatorEngine.from_state(mr.engine_state(cfg), device=_device())
    X = _up(cfg['X'])
    # cp_mlp_predict_columns itself, with a row stride that is not the count of columns
    dev = {name: _up(cfg[name]) for name in ('packed', 'xoffset', 'xscale', 'yoffset', 'yscale')}
    buf = torch.full((B, 12), PAD, dtype=torch.float64, device=_device())
    _lib.check(lib.cp_mlp_predict_columns(X.data_ptr(), B, 3, 2, _ints([5, H]), _ints([_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']]), M, dev['packed'].data_ptr(),
                                          dev['xoffset'].data_ptr(), dev['xscale'].data_ptr(), dev['yoffset'].data_ptr(), dev['yscale'].data_ptr(),
                                          _lib.MLP_YFUNCTIONS[yfunction or None], RANGE[0], RANGE[1] - RANGE[0], buf.data_ptr(), 12, 0, _stream()))
    out = _engine_entries(engine, X, cfg['cot'], buf[:, :10], store_predict=H == 17)
    out['predict_columns_ldo12'] = buf
    # cp_mlp_loss_grad at M = 65: its dh launch is the vjp's
    dims, acts = (3, 5, H, 65), ['silu', 'identity-silu']
    rng = np.random.default_rng(H)
    packed, Xs, Ys = _up(vr.draw_network(rng, dims)), _up(rng.uniform(0., 1., (B, 3))), _up(rng.normal(0., 1., (B, 65)))
    need = int(lib.cp_mlp_workspace_doubles(B, 3, 2, _ints([5, H]), 65))
    work = torch.empty(need, dtype=torch.float64, device=_device())
    loss, grad = torch.zeros(1, dtype=torch.float64, device=_device()), torch.full_like(packed, PAD)
    _lib.check(lib.cp_mlp_loss_grad(Xs.data_ptr(), Ys.data_ptr(), B, 3, 2, _ints([5, H]), _ints([_lib.MLP_ACTIVATIONS[a] for a in acts]), 65, packed.data_ptr(),
                                    work.data_ptr(), need, loss.data_ptr(), grad.data_ptr(), 0, _stream()))
    out['loss'], out['loss_grad'] = loss, grad
    return {name: value.cpu().numpy() for name, value in out.items()}


def taylor_entries():
    import torch
    from cosmoprimo_amd import _lib
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    lib = _lib.load()
    rng = np.random.default_rng(260)
    powers = np.array([(i, j, k) for i in range(4) for j in range(4) for k in range(4) if i + j + k <= 3], dtype='i4')      # all 20 terms of order 3
    center, derivatives = rng.uniform(-0.5, 0.5, 3), rng.normal(0., 1., (len(powers), M))
    engine = TaylorEmulatorEngine.from_state({'center': center, 'powers': powers, 'derivatives': derivatives}, device=_device())
    X = _up(rng.uniform(-1., 1., (B, 3)))
    cot = rng.normal(0., 1., (B, M))
    dev = {'center': _up(center), 'powers': _up(powers), 'derivatives': _up(derivatives)}
    buf = torch.full((B, 12), PAD, dtype=torch.float64, device=_device())
    _lib.check(lib.cp_taylor_predict_columns(X.data_ptr(), B, dev['center'].data_ptr(), dev['powers'].data_ptr(), 3, len(powers), 3, dev['derivatives'].data_ptr(), M,
                                             RANGE[0], RANGE[1] - RANGE[0], buf.data_ptr(), 12, 0, _stream()))
    out = _engine_entries(engine, X, cot, buf[:, :10], store_predict=True)
    out['predict_columns_ldo12'] = buf
    # cp_taylor_fit: derivatives (T, 10) = S (T, 65) . Y (65, 10)
    S, Y = _up(rng.normal(0., 1., (len(powers), 65))), _up(rng.normal(0., 1., (65, 10)))
    fitted = torch.full((len(powers), 10), PAD, dtype=torch.float64, device=_device())
    _lib.check(lib.cp_taylor_fit(S.data_ptr(), len(powers), 65, Y.data_ptr(), 10, fitted.data_ptr(), 0, _stream()))
    out['fit'] = fitted
    return {name: value.cpu().numpy() for name, value in out.items()}


def emulator_entries(emulator):
    """Emulator.predict, jacobian and vjp over three varied keys on the engine's 8 columns -- 'head.a' (3,), 'head.b' (2, 2), 'tail' () -- for every key
    (one run, ``columns=None``), the section 'head' (one run) and 'head.a' with 'tail' (two runs), at B = 33 and at one point of scalar parameters."""
    from cosmoprimo_amd.emulators import Emulator
    split = Emulator.__new__(Emulator)
    split.calculator, split.samples, split.params, split.fixed, split.engine = None, None, dict(emulator.params), {'x': XGRID}, emulator.engine
    split.varied_keys, split.varied_shapes = ['head.a', 'head.b', 'tail'], [(3,), (2, 2), ()]
    params = batch()
    rng = np.random.default_rng(33)
    cots = {'head.a': rng.normal(0., 1., (33, 3)), 'head.b': rng.normal(0., 1., (33, 2, 2)), 'tail': rng.normal(0., 1., 33)}
    out = {}
    for label, p, c in (('batch', params, cots), ('point', {name: float(params[name][5]) for name in NAMES}, {key: cot[5] for key, cot in cots.items()})):
        for what, keys, wanted in (('all', None, split.varied_keys), ('section', 'head', ['head.a', 'head.b']), ('two_runs', ['head.a', 'tail'], ['head.a', 'tail'])):
            results = {'predict': split.predict(p, keys=keys)}
            values, results['jacobian'] = split.jacobian(p, keys=keys, return_value=True)
            assert list(values) == list(results['predict']) and all(_same(values[key], value) for key, value in results['predict'].items())
            values, results['vjp'] = split.vjp(p, {key: c[key] for key in wanted}, return_value=True)
            assert [key for key in values if key != 'x'] == wanted and all(_same(values[key], results['predict'][key]) for key in wanted)
            for name, result in results.items():
                varied = wanted if name != 'vjp' else NAMES
                assert [key for key in result if key != 'x'] == varied, (label, what, name, list(result))
                for key in varied:
                    out['%s.%s.%s.%s' % (label, what, name, key)] = np.asarray(result[key])
    return out


@pytest.fixture(scope='module')
def recorded():
    return dict(np.load(FIXTURE))


def flatten(entries):
    """(labels 'name shape', one flat array) of a dictionary of float64 arrays, in the order of the names: what the fixture holds per test."""
    names = sorted(entries)
    assert all(entries[name].dtype == np.float64 for name in names)
    return np.array(['%s %s' % (name, entries[name].shape) for name in names]), np.concatenate([np.ravel(entries[name]) for name in names])


def assert_equal_bits(got, recorded, group):
    labels, flat = flatten(got)
    assert list(labels) == list(recorded[group + '.entries']) and flat.shape == recorded[group].shape
    offset = 0
    for label, name in zip(labels, sorted(got)):
        assert np.array_equal(flat[offset:offset + got[name].size], recorded[group][offset:offset + got[name].size]), '%s: %s' % (group, label)
        offset += got[name].size


@pytest.mark.parametrize('H,yfunction', MLP_CASES)
def test_mlp(recorded, H, yfunction):
    assert_equal_bits(mlp_entries(H, yfunction), recorded, 'mlp%d' % H)


def test_taylor(recorded):
    assert_equal_bits(taylor_entries(), recorded, 'taylor')


@pytest.mark.parametrize('which', ['taylor', 'mlp'])
def test_emulator(recorded, emulators, which):  # noqa: F811
    assert_equal_bits(emulator_entries(emulators[which]), recorded, 'emulator_%s' % which)
