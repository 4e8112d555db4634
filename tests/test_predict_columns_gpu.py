"""GPU: cp_mlp_predict_columns / cp_taylor_predict_columns (csrc/cp_mlp.hip, csrc/cp_taylor.hip): a range [col0, col0 + ncols) of the columns of the
batched prediction, the column tiles (256 per workgroup, 64 per wave, 16 per lane group) starting at col0.

What is asserted is exact.  The sum behind an output element runs over its inner index in one order whatever tile the element falls in, so a range equals
the same columns of the full call BIT FOR BIT (``torch.equal``); the full call itself is held to its truth by tests/test_mlp_edges_gpu.py and
tests/test_taylor_edges_gpu.py.  Nothing outside the range is read: with every entry of the output kernel, the bias, yoffset and yscale (Taylor: the
derivatives) outside the range set to NaN the result keeps its bits.  Nothing outside the result is written: it is allocated with three columns more
(``ldo = ncols + 3``) and one row more, filled with a sentinel that the pad must keep.

Shapes: M = 600 (three column tiles from col0 = 0, the last ragged); every col0 of {0, 1, 15, 16, 17, 255, 256, 257, 599} -- aligned, odd (the 128 bytes
that 16 lanes fetch per k then start 8-byte aligned only), at the edges of a lane group and of the workgroup's columns, the last column -- with every ncols
of {1, 2, 16, 255, 256, 257} clipped to fit, for each configuration; configurations and B one at a time from MLP (32, 33), ndim 3, B = 65 and Taylor B = 65."""
import ctypes

import numpy as np
import pytest

import mlp_reference as mr

pytestmark = pytest.mark.gpu
M = 600
COL0 = (0, 1, 15, 16, 17, 255, 256, 257, 599)
NCOLS = (1, 2, 16, 255, 256, 257)
SENTINEL = -7.25


def ranges():
    return sorted({(col0, min(ncols, M - col0)) for col0 in COL0 for ncols in NCOLS})


def tensors(device, **arrays):
    import torch
    return {name: torch.as_tensor(np.ascontiguousarray(a), device=device) for name, a in arrays.items()}


def mlp_config(B, widths, ndim, seed, yfunction=''):
    """Synthetic weights, all distinct, as ``config`` of tests/test_mlp_edges_gpu.py."""
    rng = np.random.default_rng(seed)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = [mr.ACTIVATIONS[(seed + l) % 4] for l in range(len(widths))]
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


def mlp_outside_nan(cfg, col0, ncols):
    """The configuration with everything that belongs to the columns outside the range set to NaN."""
    outside = np.ones(M, dtype=bool)
    outside[col0:col0 + ncols] = False
    L = len(cfg['dims']) - 2
    sl = mr.blocks(cfg['dims'])
    packed, yoffset, yscale = cfg['packed'].copy(), cfg['yoffset'].copy(), cfg['yscale'].copy()
    packed[sl['kernel%d' % L]].reshape(cfg['dims'][-2], M)[:, outside] = np.nan      # (views into packed)
    packed[sl['bias%d' % L]][outside] = np.nan
    yoffset[outside] = yscale[outside] = np.nan
    return dict(cfg, packed=packed, yoffset=yoffset, yscale=yscale)


class MLPCase(object):

    def __init__(self, B, widths=(32, 33), ndim=3, yfunction=''):
        import torch
        from cosmoprimo_amd import _lib
        self.cfg = mlp_config(B, widths, ndim, seed=1000 * B + 10 * sum(widths) + ndim, yfunction=yfunction)
        self.B, self.device = B, torch.device('cuda', 0)
        self.widths = (ctypes.c_int * len(widths))(*widths)
        self.acts = (ctypes.c_int * len(widths))(*[_lib.MLP_ACTIVATIONS[a] for a in self.cfg['activations']])
        self.yfunction = _lib.MLP_YFUNCTIONS[{'': None}.get(yfunction, yfunction)]
        self.t = self.upload(self.cfg)
        self.full = torch.empty((B, M), dtype=torch.float64, device=self.device)
        t = self.t
        _lib.check(_lib.load().cp_mlp_predict(t['X'].data_ptr(), B, ndim, len(widths), self.widths, self.acts, M, t['packed'].data_ptr(), t['xoffset'].data_ptr(),
                                              t['xscale'].data_ptr(), t['yoffset'].data_ptr(), t['yscale'].data_ptr(), self.yfunction, self.full.data_ptr(), 0, self.stream()))

    def stream(self):
        from cosmoprimo_amd import _device as dv
        return dv.stream_of(self.device)

    def upload(self, cfg):
        return tensors(self.device, **{name: cfg[name] for name in ('X', 'packed', 'xoffset', 'xscale', 'yoffset', 'yscale')})

    def status(self, col0, ncols, out, ldo, t=None):
        from cosmoprimo_amd import _lib
        t = t or self.t
        return _lib.load().cp_mlp_predict_columns(t['X'].data_ptr(), self.B, self.cfg['dims'][0], len(self.widths), self.widths, self.acts, M, t['packed'].data_ptr(),
                                                  t['xoffset'].data_ptr(), t['xscale'].data_ptr(), t['yoffset'].data_ptr(), t['yscale'].data_ptr(), self.yfunction,
                                                  col0, ncols, out.data_ptr(), ldo, 0, self.stream())

    def poisoned(self, col0, ncols):
        return self.upload(mlp_outside_nan(self.cfg, col0, ncols))

    def engine(self):
        from cosmoprimo_amd.emulators import MLPEmulatorEngine
        return MLPEmulatorEngine.from_state(mr.engine_state(self.cfg), device='cuda:0')


class TaylorCase(object):

    """The first configuration of the ``taylor`` golden (20 terms of 3 parameters, 8 outputs) widened to M = 600: its derivatives repeated along the
    columns, column j times 1 + j / 1024 (so that no two columns agree); its query points repeated to B rows, each repeat shifted."""

    def __init__(self, golden, B):
        import torch
        from cosmoprimo_amd import _lib
        g = golden('taylor')
        self.center, self.powers = np.asarray(g['c0_center'], dtype='f8'), np.asarray(g['c0_powers'], dtype='i4')
        self.derivatives = np.tile(g['c0_derivatives'], (1, M // 8)) * (1. + np.arange(M) / 1024.)
        Xq = g['c0_Xq']
        self.X = np.concatenate([Xq + 1e-3 * i for i in range(B // len(Xq) + 1)])[:B]
        assert self.derivatives.shape == (20, M) and np.unique(self.derivatives, axis=1).shape[1] == M
        self.B, self.device = B, torch.device('cuda', 0)
        self.t = self.upload(self.derivatives)
        self.full = torch.empty((B, M), dtype=torch.float64, device=self.device)
        t = self.t
        _lib.check(_lib.load().cp_taylor_predict(t['X'].data_ptr(), B, t['center'].data_ptr(), t['powers'].data_ptr(), 3, 20, int(self.powers.max()),
                                                 t['derivatives'].data_ptr(), M, self.full.data_ptr(), 0, self.stream()))

    stream = MLPCase.stream

    def upload(self, derivatives):
        import torch
        t = tensors(self.device, X=self.X, center=self.center, powers=self.powers, derivatives=derivatives)
        assert t['powers'].dtype == torch.int32
        return t

    def status(self, col0, ncols, out, ldo, t=None):
        from cosmoprimo_amd import _lib
        t = t or self.t
        return _lib.load().cp_taylor_predict_columns(t['X'].data_ptr(), self.B, t['center'].data_ptr(), t['powers'].data_ptr(), 3, 20, int(self.powers.max()),
                                                     t['derivatives'].data_ptr(), M, col0, ncols, out.data_ptr(), ldo, 0, self.stream())

    def poisoned(self, col0, ncols):
        derivatives = self.derivatives.copy()
        derivatives[:, :col0] = np.nan
        derivatives[:, col0 + ncols:] = np.nan
        return self.upload(derivatives)

    def engine(self):
        from cosmoprimo_amd.emulators import TaylorEmulatorEngine
        return TaylorEmulatorEngine.from_state({'center': self.center, 'powers': self.powers, 'derivatives': self.derivatives}, device='cuda:0')


def check_ranges(case):
    import torch
    from cosmoprimo_amd import _lib
    B = case.B
    assert bool(torch.isfinite(case.full).all())
    for col0, ncols in ranges():
        want = case.full[:, col0:col0 + ncols]
        for t in (None, case.poisoned(col0, ncols)):
            out = torch.full((B + 1, ncols + 3), SENTINEL, dtype=torch.float64, device=case.device)
            _lib.check(case.status(col0, ncols, out, ncols + 3, t=t))
            what = 'columns [%d, %d)%s' % (col0, col0 + ncols, ', NaN outside them' if t is not None else '')
            assert torch.equal(out[:B, :ncols], want), what
            assert bool((out[:B, ncols:] == SENTINEL).all()) and bool((out[B] == SENTINEL).all()), what + ': pad overwritten'


MLP_CASES = [dict(widths=(3,)), dict(widths=(32, 33)), dict(widths=(64,)), dict(ndim=1), dict(ndim=32), dict(yfunction='log10'), dict(yfunction='arcsinh'),
             dict(B=1), dict(B=63), dict(B=64)]


@pytest.mark.parametrize('options', MLP_CASES, ids=['-'.join('%s=%s' % item for item in case.items()).replace(' ', '') for case in MLP_CASES])
def test_mlp_ranges(options):
    """One dimension at a time from widths (32, 33), ndim 3, B = 65, no y function: the widths (3,) -- one MFMA pair, five of its eight k masked --, (32, 33)
    and (64,) -- 80 KB of LDS --, ndim 1 and 32, the three y functions, B in {1, 63, 64, 65}; every range each."""
    check_ranges(MLPCase(**{'B': 65, **options}))


@pytest.mark.parametrize('B', [1, 63, 64, 65])
def test_taylor_ranges(golden, B):
    check_ranges(TaylorCase(golden, B))


@pytest.mark.parametrize('which', ['mlp', 'taylor'])
def test_bad_ranges_are_refused_and_the_device_answers(golden, which):
    """col0 < 0, ncols < 1, col0 + ncols > M and ldo < ncols raise ValueError (CP_EINVAL, before any launch: the result keeps its sentinel); the next call
    gives the right columns."""
    import torch
    from cosmoprimo_amd import _lib
    case = MLPCase(65) if which == 'mlp' else TaylorCase(golden, 65)
    out = torch.full((65, 16), SENTINEL, dtype=torch.float64, device=case.device)
    for col0, ncols, ldo in ((-1, 8, 16), (0, 0, 16), (0, -3, 16), (M - 7, 8, 16), (M, 1, 16), (0, M + 1, M + 1), (8, 16, 15), (2**31, 8, 16)):
        with pytest.raises(ValueError, match='columns|row stride'):
            _lib.check(case.status(col0, ncols, out, ldo))
    torch.cuda.synchronize(case.device)
    assert bool((out == SENTINEL).all())
    _lib.check(case.status(M - 16, 16, out, 16))
    assert torch.equal(out, case.full[:, M - 16:])


@pytest.mark.parametrize('which', ['mlp', 'taylor'])
def test_engine_columns(golden, which):
    """``engine.predict(X, columns=(a, b))`` is ``engine.predict(X)[:, a:b]``, and refuses what the entry point refuses."""
    import torch
    case = MLPCase(65) if which == 'mlp' else TaylorCase(golden, 65)
    engine = case.engine()
    X = case.cfg['X'] if which == 'mlp' else case.X
    full = engine.predict(X)
    assert torch.equal(full, case.full)
    for a, b in ((0, M), (17, 274), (599, 600), (1, 2)):
        got = engine.predict(X, columns=(a, b))
        assert tuple(got.shape) == (65, b - a) and got.is_contiguous() and torch.equal(got, full[:, a:b])
    for a, b in ((5, 5), (-1, 4), (590, 601)):
        with pytest.raises(ValueError):
            engine.predict(X, columns=(a, b))
