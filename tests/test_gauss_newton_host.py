"""CPU: (a) the truth of tests/gauss_newton_reference.py -- ``contract`` against the plain ``einsum`` of the longdouble Jacobian and value of
tests/jacobian_reference.py, a zero weight dropping its column whatever it holds -- and the level of the tolerance rule, at most 32 for every case the
device tests use (a case above it is redrawn, the cap stays); (b) the argument checks of cp_mlp_gauss_newton and cp_taylor_gauss_newton, which come back by
status with the entry point's name in cp_last_error() before any device call (this test runs without a device); (c) the key handling of
Emulator.gauss_newton on a stub engine."""
import ctypes

import numpy as np
import pytest

import gauss_newton_reference as gr
import jacobian_reference as jr

LD = np.longdouble


@pytest.mark.parametrize('options', gr.MLP_CASES, ids=[gr.case_id(case) for case in gr.MLP_CASES])
def test_mlp_level(options):
    cfg = gr.mlp_config(**options)
    truth, restated, value = gr.mlp_truth(cfg)
    assert all(r.dtype == LD for r in truth) and truth[0].shape == (len(cfg['X']),) + 2 * cfg['X'].shape[1:]
    level = gr.worst_level(truth, restated)
    print('%s: level at most %.3g' % (options, level))
    assert level <= 32.
    assert (cfg['weights'] > 0).all() and cfg['weights'].max() / cfg['weights'].min() > (30. if cfg['weights'].size > 4 else 1.)


@pytest.mark.parametrize('options', gr.TAYLOR_CASES, ids=[gr.case_id(case) for case in gr.TAYLOR_CASES])
def test_taylor_level(options):
    cfg = gr.taylor_config(**options)
    truth, restated, value = gr.taylor_truth(cfg)
    assert all(r.dtype == LD for r in truth)
    level = gr.worst_level(truth, restated)
    print('%s: level at most %.3g' % (options, level))
    assert level <= 32.
    args = (cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'])      # the dyadic polynomial is exact in float64
    assert np.array_equal(jr.taylor_jacobian(*args, dtype='f8'), jr.taylor_jacobian(*args, dtype=LD))
    assert np.array_equal(jr.taylor_predict(*args, dtype='f8'), jr.taylor_predict(*args, dtype=LD))


def test_level_of_the_other_tests():
    """The configurations of the zero-weight, NaN and engine tests of the two device files."""
    for options in (dict(B=22, ncols=65), dict(B=22, ncols=65, yfunction='log10'), dict(B=22, yfunction='arcsinh')):
        cfg = gr.mlp_config(**options)
        gr.mlp_truth(cfg)
        cfg['weights'][:, [0, 15, 16]] = 0.
        assert gr.worst_level(*gr.mlp_truth(cfg)[:2]) <= 32., options
    for options in (dict(B=22, ncols=65), dict(B=22)):
        assert gr.worst_level(*gr.taylor_truth(gr.taylor_config(**options))[:2]) <= 32., options


@pytest.mark.parametrize('kind', ['mlp', 'taylor'])
def test_contract_is_the_einsum_of_the_longdouble_jacobian(kind):
    if kind == 'mlp':
        cfg = gr.mlp_config(B=5, ncols=9, yfunction='log10')
        truth, restated, value = gr.mlp_truth(cfg)
        full, J = jr.mlp_jacobian(*gr.mlp_args(cfg), dtype=LD)
    else:
        cfg = gr.taylor_config(B=5, ncols=9)
        truth, restated, value = gr.taylor_truth(cfg)
        args = (cfg['center'], cfg['powers'], cfg['derivatives'], cfg['X'])
        full, J = jr.taylor_predict(*args, dtype=LD), jr.taylor_jacobian(*args, dtype=LD)
    a, b = cfg['columns']
    J, w, r = J[:, :, a:b], cfg['weights'].astype(LD), cfg['data'].astype(LD) - full[:, a:b]
    assert np.array_equal(value, full[:, a:b])
    scale = lambda x: np.abs(x).max()      # noqa: E731
    assert scale(truth[0] - np.einsum('bic,bc,bjc->bij', J, w, J)) <= 1e-17 * scale(truth[0])
    assert scale(truth[1] - np.einsum('bic,bc->bi', J, w * r)) <= 1e-17 * scale(truth[1])
    assert scale(truth[2] - (w * r * r).sum(axis=1)) <= 1e-17 * scale(truth[2])
    # a zero weight drops its column whatever it holds
    w0, Jbad, data = cfg['weights'].copy(), J.copy(), cfg['data'].copy()
    w0[:, 2] = 0.
    Jbad[:, :, 2], data[:, 2] = np.inf, np.nan
    dropped = gr.contract(Jbad, full[:, a:b], w0, data, LD)
    kept = gr.contract(np.delete(J, 2, axis=2), np.delete(full[:, a:b], 2, axis=1), np.delete(cfg['weights'], 2, axis=1), np.delete(cfg['data'], 2, axis=1), LD)
    assert all(np.array_equal(x, y) for x, y in zip(dropped, kept))
    assert gr.contract(J, full[:, a:b], cfg['weights'], None, LD)[1:] == (None, None)


FAKE = ctypes.c_void_p(8)      # a non-null pointer nobody reads: every call here returns before its first device call
MLP_POINTERS = 13              # d_x, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, d_weights, d_data, d_value, d_fisher, d_grad, d_chi2, d_work
TAYLOR_POINTERS = 11           # d_x, d_center, d_powers, d_derivatives, d_weights, d_data, d_value, d_fisher, d_grad, d_chi2, d_work


def mlp_call(B=4, ndim=3, widths=(5, 17), M=8, col0=0, ncols=8, ldw=8, ldd=8, ldv=8, work=None, pointers=None, yfunction=0):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    L = len(widths)
    p = [FAKE] * MLP_POINTERS if pointers is None else pointers
    w = (ctypes.c_int * L)(*widths)
    if work is None:
        work = max(int(lib.cp_mlp_gauss_newton_workspace_doubles(max(B, 0), ndim, L, w, M, ncols)), 0)
    return lib.cp_mlp_gauss_newton(p[0], B, ndim, L, w, (ctypes.c_int * L)(*([0] * L)), M, p[1], p[2], p[3], p[4], p[5], yfunction, col0, ncols, p[6], ldw, p[7], ldd,
                                   p[8], ldv, p[9], p[10], p[11], p[12], work, 0, None)


def taylor_call(B=4, ndim=3, T=20, max_power=3, M=8, col0=0, ncols=8, ldw=8, ldd=8, ldv=8, work=None, pointers=None):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    p = [FAKE] * TAYLOR_POINTERS if pointers is None else pointers
    if work is None:
        work = max(int(lib.cp_taylor_gauss_newton_workspace_doubles(max(B, 0), ndim, T, M, ncols)), 0)
    return lib.cp_taylor_gauss_newton(p[0], B, p[1], p[2], ndim, T, max_power, p[3], M, col0, ncols, p[4], ldw, p[5], ldd, p[6], ldv, p[7], p[8], p[9], p[10], work, 0, None)


@pytest.mark.parametrize('call,npointers,name', [(mlp_call, MLP_POINTERS, b'cp_mlp_gauss_newton'), (taylor_call, TAYLOR_POINTERS, b'cp_taylor_gauss_newton')], ids=['mlp', 'taylor'])
def test_argument_checks_come_before_any_device_call(call, npointers, name):
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    named = lambda words: name in lib.cp_last_error() and words in lib.cp_last_error()      # noqa: E731
    data, value, grad, chi2 = npointers - 6, npointers - 5, npointers - 3, npointers - 2
    some = lambda *null: [None if j in null else FAKE for j in range(npointers)]      # noqa: E731
    for k in range(npointers):      # each null pointer on its own is refused, but for the value, which is optional
        if k == value:
            continue
        assert call(pointers=some(k)) == _lib.CP_EINVAL and name in lib.cp_last_error(), k
    assert call(pointers=some(data)) == _lib.CP_EINVAL and named(b'without data')      # d_grad and d_chi2 given without d_data
    assert call(pointers=some(data, chi2)) == _lib.CP_EINVAL and named(b'without data')      # d_grad alone
    assert call(pointers=some(data, grad)) == _lib.CP_EINVAL and named(b'without data')
    assert call(pointers=some(grad)) == _lib.CP_EINVAL and named(b'null pointer') and call(pointers=some(chi2)) == _lib.CP_EINVAL and named(b'null pointer')
    # the strides: 0 (one shared row) or at least ncols for the weights and the data, at least ncols for the value; those of absent operands are not read
    for bad in (dict(ldw=7), dict(ldw=-1), dict(ldd=7), dict(ldd=1), dict(ldv=7), dict(ldv=0)):
        assert call(**bad) == _lib.CP_EINVAL and named(b'row stride'), bad
    # a workspace that is too small
    assert call(work=0) == _lib.CP_EINVAL and named(b'workspace') and named(b'_workspace_doubles')
    for col0, ncols in ((-1, 4), (0, 0), (0, -3), (4, 5), (8, 1), (0, 9), (2**31, 4)):
        assert call(col0=col0, ncols=ncols, ldw=16, ldd=16, ldv=16, work=2**40) == _lib.CP_EINVAL and named(b'columns')
    assert call(B=-1, work=2**40) == _lib.CP_EINVAL
    assert call(B=0) == _lib.CP_OK and call(B=0, pointers=[None] * npointers) == _lib.CP_OK
    assert call(ndim=33, work=2**40) == _lib.CP_EUNSUPPORTED and name in lib.cp_last_error()
    # the B cap: 2^31 - 1 row tiles of floor(64 / ndim) points and 2^31 - 1 workgroups of 256 sums B (ndim^2 + ndim + 1); the largest count below is refused only
    # for its null pointers
    for ndim in (1, 3, 8, 32):
        most = min((2**31 - 1) * (64 // ndim), (2**31 - 1) * 256 // (ndim * ndim + ndim + 1))
        assert call(B=most + 1, ndim=ndim, work=2**62) == _lib.CP_EUNSUPPORTED and named(b'points')
        assert call(B=most, ndim=ndim, work=2**62, pointers=[None] * npointers) == _lib.CP_EINVAL and named(b'null pointer')
    assert call(B=2**62, work=2**62) == _lib.CP_EUNSUPPORTED and name in lib.cp_last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(B=2**40, work=2**62))


def test_argument_checks_of_the_network_the_polynomial_and_the_sizers():
    from cosmoprimo_amd import _lib
    lib = _lib.load()
    assert mlp_call(widths=(5, 65), work=2**40) == _lib.CP_EUNSUPPORTED and b'width 65' in lib.cp_last_error() and b'cp_mlp_gauss_newton' in lib.cp_last_error()
    assert mlp_call(widths=(5, 0), work=2**40) == _lib.CP_EINVAL and mlp_call(widths=(8,) * 9, work=2**40) == _lib.CP_EUNSUPPORTED
    assert mlp_call(yfunction=3) == _lib.CP_EINVAL
    assert taylor_call(max_power=16) == _lib.CP_EUNSUPPORTED and b'cp_taylor_gauss_newton' in lib.cp_last_error()
    assert taylor_call(max_power=-1) == _lib.CP_EINVAL and taylor_call(T=0, work=2**40) == _lib.CP_EINVAL
    # the order of the fronts: the range of columns before the strides, the strides before the caps of the entry point
    assert mlp_call(ncols=0, ldw=-1, work=2**40) == _lib.CP_EINVAL and b'columns' in lib.cp_last_error()
    assert mlp_call(ldw=7, B=2**62, work=2**62) == _lib.CP_EINVAL and taylor_call(ldd=7, B=2**62, work=2**62) == _lib.CP_EINVAL
    # the sizers: the value (B, ncols) and per column tile B (ndim^2 + ndim + 1) partial sums; minus the status on an error
    w = (ctypes.c_int * 2)(5, 17)
    for B, ndim, ncols in ((4, 3, 8), (100, 8, 257), (7, 32, 1024)):
        want = B * ncols + -(-ncols // 256) * B * (ndim * ndim + ndim + 1)
        assert lib.cp_mlp_gauss_newton_workspace_doubles(B, ndim, 2, w, 2000, ncols) == want
        assert lib.cp_taylor_gauss_newton_workspace_doubles(B, ndim, 20, 2000, ncols) == want
    assert lib.cp_mlp_gauss_newton_workspace_doubles(-1, 3, 2, w, 8, 8) == -_lib.CP_EINVAL and lib.cp_mlp_gauss_newton_workspace_doubles(4, 3, 2, w, 8, 9) == -_lib.CP_EINVAL
    assert lib.cp_mlp_gauss_newton_workspace_doubles(2**62, 3, 2, w, 8, 8) == -_lib.CP_EUNSUPPORTED and b'cp_mlp_gauss_newton_workspace_doubles' in lib.cp_last_error()
    assert lib.cp_taylor_gauss_newton_workspace_doubles(-1, 3, 20, 8, 8) == -_lib.CP_EINVAL and lib.cp_taylor_gauss_newton_workspace_doubles(4, 3, 20, 8, 9) == -_lib.CP_EINVAL
    assert lib.cp_taylor_gauss_newton_workspace_doubles(2**62, 3, 20, 8, 8) == -_lib.CP_EUNSUPPORTED and b'cp_taylor_gauss_newton_workspace_doubles' in lib.cp_last_error()


class StubEngine(object):
    """What Emulator.gauss_newton uses of an engine, on host tensors: fisher = sum of the weights times the identity, grad = sum of weights x data in every parameter,
    chi2 = sum of the data, the value the column numbers."""
    name, device, _dev = 'stub', None, {'device': None}

    def __init__(self):
        self.calls = []

    def gauss_newton(self, X, weights, data=None, columns=None, return_value=False):
        import torch
        self.calls.append((np.asarray(X), weights.numpy().copy(), None if data is None else data.numpy().copy(), columns))
        B, ndim = np.shape(X)
        out = (weights.sum(dim=1)[:, None, None] * torch.eye(ndim, dtype=torch.float64),)
        if data is not None:
            out += ((weights * data).sum(dim=1)[:, None].expand(B, ndim).clone(), data.sum(dim=1))
        if return_value:
            out = (torch.arange(columns[0], columns[1], dtype=torch.float64).expand(B, columns[1] - columns[0]),) + out
        return out[0] if len(out) == 1 else out

    def predict(self, X, columns=None):
        import torch
        return torch.arange(columns[0], columns[1], dtype=torch.float64).expand(len(X), columns[1] - columns[0])


def stub_emulator():
    from cosmoprimo_amd.emulators import Emulator
    emulator = Emulator(None, params={'a': (0., 1.), 'b': (0., 1.), 'c': (0., 1.)}, engine=StubEngine())
    emulator.varied_keys, emulator.varied_shapes, emulator.fixed = ['curve', 'middle', 'product', 'grid'], [(4,), (2,), (), (2, 3)], {'x': np.arange(3.)}
    return emulator      # columns: curve [0, 4), middle [4, 6), product [6, 7), grid [7, 13)


def test_emulator_keys_on_a_stub_engine():
    import torch
    emulator = stub_emulator()
    engine = emulator.engine
    real = emulator.gauss_newton

    def gauss_newton(params, weights, data=None, **kwargs):      # the operands as host tensors: without a device nothing can be uploaded
        t = lambda d: None if d is None else {key: torch.as_tensor(value, dtype=torch.float64) for key, value in d.items()}      # noqa: E731
        return real(params, t(weights), data=t(data), **kwargs)
    params = {'a': np.linspace(0., 1., 5), 'b': 0.5, 'c': np.linspace(1., 0., 5)}
    with pytest.raises(KeyError):      # an unknown key of weights
        gauss_newton(params, {'curve': 1., 'nothing': 1.})
    with pytest.raises(KeyError):      # a key of data that holds no weights
        gauss_newton(params, {'curve': 1.}, data={'curve': 1., 'product': 2.})
    with pytest.raises(ValueError):      # a varied key of weights without data
        gauss_newton(params, {'curve': 1., 'product': 1.}, data={'curve': 1.})
    with pytest.raises(ValueError):      # a missing parameter
        gauss_newton({'a': 1.}, {'curve': 1.})
    assert not engine.calls
    # two non-adjacent keys: two runs, added in run order; a fixed key is accepted and contributes nothing (with or without data)
    weights = {'grid': np.arange(1., 7.).reshape(2, 3), 'curve': np.array([1., 2., 3., 4.]), 'x': 5.}
    fisher = gauss_newton(params, weights)
    assert [call[3] for call in engine.calls] == [(0, 4), (7, 13)] and all(call[2] is None for call in engine.calls)
    assert engine.calls[0][1].shape == (5, 4) and np.array_equal(engine.calls[1][1], np.tile(np.arange(1., 7.), (5, 1))) and engine.calls[0][0].shape == (5, 3)
    assert isinstance(fisher, np.ndarray) and fisher.shape == (5, 3, 3) and np.array_equal(fisher, np.tile(31. * np.eye(3), (5, 1, 1)))
    del engine.calls[:]
    data = {'curve': np.ones((5, 4)), 'grid': 2.}
    fisher2, gradient, chi2 = gauss_newton(params, weights, data=data)
    assert np.array_equal(fisher2, fisher) and list(gradient) == ['a', 'b', 'c'] and all(g.shape == (5,) and (g == 10. + 42.).all() for g in gradient.values())
    assert chi2.shape == (5,) and (chi2 == 4. + 12.).all() and [call[3] for call in engine.calls] == [(0, 4), (7, 13)]
    del engine.calls[:]
    # adjacent keys are one run, in the calculator's order whatever the dictionary's
    gauss_newton(params, {'middle': 1., 'curve': 2.}, data={'curve': 0., 'middle': 0.})
    assert [call[3] for call in engine.calls] == [(0, 6)] and np.array_equal(engine.calls[0][1][0], [2., 2., 2., 2., 1., 1.])
    del engine.calls[:]
    # empty weights, and fixed keys only: zeros, no call
    for weights0 in ({}, {'x': 1.}):
        fisher0, gradient0, chi0 = gauss_newton(params, weights0, data={})
        assert fisher0.shape == (5, 3, 3) and not fisher0.any() and not chi0.any() and chi0.shape == (5,) and all(not g.any() for g in gradient0.values())
        assert gauss_newton(params, weights0).shape == (5, 3, 3)
    assert not engine.calls
    # scalar parameters: no leading axis
    point = {'a': 0.1, 'b': 0.2, 'c': 0.3}
    fisher1, gradient1, chi1 = gauss_newton(point, {'product': 2.}, data={'product': 3.})
    assert fisher1.shape == (3, 3) and np.array_equal(fisher1, 2. * np.eye(3)) and all(g.shape == () and g == 6. for g in gradient1.values()) and chi1.shape == () and chi1 == 3.
    assert gauss_newton(point, {}).shape == (3, 3)
    # return_value: what predict gives for the keys of weights, then the results; device=True: tensors
    values, fisherv = gauss_newton(params, {'grid': 1., 'x': 1., 'curve': 1.}, return_value=True)
    assert list(values) == ['curve', 'grid', 'x'] and values['grid'].shape == (5, 2, 3) and np.array_equal(values['grid'][0], np.arange(7., 13.).reshape(2, 3))
    values, fisherd, gradientd, chid = gauss_newton(params, {'curve': 1.}, data={'curve': 1.}, device=True, return_value=True)
    assert all(isinstance(t, torch.Tensor) for t in (values['curve'], fisherd, chid, gradientd['a'])) and tuple(fisherd.shape) == (5, 3, 3)
