"""GPU: cp_mlp_predict (csrc/cp_mlp.hip) at the edges of its tiles -- 64 rows x 256 columns per workgroup, 64 columns per wave, hidden neurons four at a
time per wave, MFMA steps of 4 taken in pairs over the last hidden width -- on synthetic weights, all distinct, one dimension at a time from a small base.

Truth and tolerance: the longdouble forward pass and the running bound of tests/mlp_reference.py (derived, not measured)."""
import numpy as np
import pytest

import mlp_reference as mr

pytestmark = pytest.mark.gpu
BASE = dict(B=65, M=257, widths=(5, 17), ndim=3)


def config(B, M, widths, ndim, seed, activations=None, yfunction=''):
    rng = np.random.default_rng(seed)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = list(activations or [mr.ACTIVATIONS[(seed + l) % 4] for l in range(len(widths))])
    packed = np.zeros(mr.nparams(dims))
    for name, sl in mr.blocks(dims).items():
        l = int(name[-1])
        packed[sl] = rng.uniform(0.3, 1.2, 2) if name.startswith('alphabeta') else rng.normal(0., 1. / np.sqrt(dims[l]) if name.startswith('kernel') else 0.3, sl.stop - sl.start)
    lo = rng.uniform(-1., 1., ndim)
    cfg = dict(dims=dims, activations=activations, packed=packed, yfunction=yfunction, xoffset=lo, xscale=rng.uniform(0.5, 2., ndim),
               yoffset=rng.normal(0., 1., M), yscale=rng.uniform(0.5, 2., M))
    cfg['X'] = lo + cfg['xscale'] * rng.uniform(0., 1., (B, ndim))
    assert np.unique(cfg['X']).size == cfg['X'].size and np.unique(packed).size == packed.size
    return cfg


def engine_of(cfg):
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    return MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0')


def fraction_of(cfg):
    got = engine_of(cfg).predict(cfg['X']).cpu().numpy()
    truth, bound = mr.predict_bound(*[cfg[name] for name in ('packed', 'dims', 'activations', 'X', 'xoffset', 'xscale', 'yoffset', 'yscale', 'yfunction')])
    assert got.shape == truth.shape == (len(cfg['X']), cfg['dims'][-1]) and np.isfinite(got).all()
    return float((np.abs(got - truth) / bound).max())


SWEEP = ([('B', v) for v in (1, 63, 64, 65, 129)] + [('M', v) for v in (1, 63, 64, 65, 255, 256, 257)] + [('ndim', v) for v in (1, 32)]
         + [('width', v) for v in (1, 4, 5, 31, 32, 33, 64)] + [('layers', v) for v in (1, 8)])


@pytest.mark.parametrize('name,value', SWEEP, ids=['%s%d' % item for item in SWEEP])
def test_predict_one_dimension_at_a_time(name, value):
    """Around B = 65, M = 257, widths (5, 17), ndim = 3: the ends of the row tile, of a wave's and the workgroup's columns, of the input staging, of the
    neurons a wave takes (width mod 16, mod 4) and of the MFMA pairs (last width mod 8; 'width' sets BOTH hidden widths), one hidden layer and eight
    (every activation twice)."""
    shape = dict(BASE)
    if name == 'width':
        shape['widths'] = (value, value)
    elif name == 'layers':
        shape['widths'] = (7, 17, 33, 4, 64, 1, 9, 12)[:value]
    else:
        shape[name] = value
    fraction = fraction_of(config(seed=100 * len(name) + value, **shape))
    print('predict %s: %.3g of the bound' % (shape, fraction))
    assert fraction <= 1.


@pytest.mark.parametrize('yfunction', ['log10', 'arcsinh'])
def test_predict_epilogue_functions(yfunction):
    fraction = fraction_of(config(129, 300, (32, 32, 32), 3, seed=7, yfunction=yfunction))
    print('predict with %s: %.3g of the bound' % (yfunction, fraction))
    assert fraction <= 1.


@pytest.mark.parametrize('B', [63, 65])
def test_nothing_is_stored_past_the_end(B):
    """The result allocated with one row more than asked for, holding a sentinel (M = 257: the second column tile holds one column, whose neighbours in
    memory are the next row)."""
    import ctypes
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    cfg = config(B, 257, (5, 17), 3, seed=300 + B)
    device = torch.device('cuda', 0)
    t = {name: torch.as_tensor(np.ascontiguousarray(cfg[name]), device=device) for name in ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale')}
    out = torch.full((B + 1, 257), -7.25, dtype=torch.float64, device=device)
    widths, acts = (ctypes.c_int * 2)(5, 17), (ctypes.c_int * 2)(*[_lib.MLP_ACTIVATIONS[a] for a in cfg['activations']])
    _lib.check(_lib.load().cp_mlp_predict(t['X'].data_ptr(), B, 3, 2, widths, acts, 257, t['packed'].data_ptr(), t['xoffset'].data_ptr(), t['xscale'].data_ptr(),
                                          t['yoffset'].data_ptr(), t['yscale'].data_ptr(), 0, out.data_ptr(), 0, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    out = out.cpu().numpy()
    assert (out[B] == -7.25).all() and (out[:B] != -7.25).all()
    assert np.array_equal(out[:B], engine_of(cfg).predict(cfg['X']).cpu().numpy())


def test_containment():
    """A NaN in row r of x stays in row r (r at both sides of the row tiles' border); a NaN in column m of the output kernel stays in column m (m at the
    borders of the lane groups, the waves and the workgroups)."""
    cfg = config(130, 513, (5, 17), 3, seed=41, activations=['silu', 'tanh'])
    clean = engine_of(cfg).predict(cfg['X']).cpu().numpy()
    rows = [0, 63, 64, 129]
    bad = dict(cfg, X=cfg['X'].copy())
    bad['X'][rows, 1] = np.nan
    got = engine_of(bad).predict(bad['X']).cpu().numpy()
    others = np.ones(130, dtype=bool)
    others[rows] = False
    assert np.isnan(got[rows]).all() and np.array_equal(got[others], clean[others])
    columns = [0, 15, 16, 63, 64, 255, 256, 512]
    packed = cfg['packed'].copy()
    kernel = packed[mr.blocks(cfg['dims'])['kernel2']].reshape(17, 513)      # (a view into packed)
    kernel[np.arange(len(columns)) * 2, columns] = np.nan
    got = engine_of(dict(cfg, packed=packed)).predict(cfg['X']).cpu().numpy()
    others = np.ones(513, dtype=bool)
    others[columns] = False
    assert np.isnan(got[:, columns]).all() and np.array_equal(got[:, others], clean[:, others])


def test_caps():
    from cosmoprimo_amd.emulators import MLPEmulatorEngine
    for widths, ndim in (((65,), 3), ((4,) * 9, 3), ((8,), 33)):
        dims = (ndim,) + widths + (8,)
        cfg = dict(dims=dims, activations=['silu'] * len(widths), packed=np.zeros(mr.nparams(dims)), yfunction='', xoffset=np.zeros(ndim), xscale=np.ones(ndim),
                   yoffset=np.zeros(8), yscale=np.ones(8))
        with pytest.raises(NotImplementedError, match='at most'):
            MLPEmulatorEngine.from_state(mr.engine_state(cfg), device='cuda:0').predict(np.zeros((4, ndim)))
    with pytest.raises(NotImplementedError):
        MLPEmulatorEngine(nhidden=(65,), device='cuda:0').fit(np.zeros((8, 2)), np.zeros((8, 3)))
