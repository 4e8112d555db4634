"""GPU: cp_taylor_vjp2 (csrc/cp_taylor.hip: the GEMM with the front end of the fit on the transposed derivatives, then taylor_curvature_kernel) against the
longdouble contraction of tests/vjp2_reference.py: C[b, i, j] = sum_c q d^2 value / d x_i d x_j with the signed cotangent q = w (data - value).

Tolerance (vjp2_reference.assert_within): the project's rule, per pair (i, j) over the batch 16 x the rounding level of the float64 restatement, floored at
1.1e-16; tests/test_vjp2_host.py holds every case to a level of at most 32 floors.

Every call (``run``) gets derivatives whose columns outside the range are 1e300, reads a cotangent with the row stride ncols + 3 (the padding NaN), writes the
matrices followed by 64 sentinels and gets a workspace of exactly cp_taylor_vjp2_workspace_doubles filled with NaN and followed by 64 sentinels.  Asserted
there: the sentinels survive, a second call gives the same bits, every matrix is symmetric bit for bit.

Cases (vjp2_reference.taylor_cases), one thing at a time from B = 9, ndim = 3, T = 20 of order 3, columns [3, 20) of 25: the rows B ndim (ndim + 1) / 2 against
the tiles of 64, the columns, T in {1, 31, 32, 33, 70} against the chunks of 32 terms, order 1 (exactly 0) and 2."""
import numpy as np
import pytest

import gauss_newton_reference as gn
import vjp2_reference as cr
from mlp_device import same_bits

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
PAD, TAIL = 3, 64
CASES = cr.taylor_cases()


def run(cfg, q, poisoned=True):
    """C (B, ndim, ndim) of one call of cp_taylor_vjp2 on the columns of cfg, with everything the module docstring says asserted."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    lib, device = _lib.load(), torch.device('cuda', 0)
    given = gn.taylor_poisoned(cfg) if poisoned else cfg
    (B, ndim), (T, M) = cfg['X'].shape, cfg['derivatives'].shape
    col0, stop = cfg['columns']
    ncols = stop - col0
    ld = ncols + PAD
    padded = np.full((B, ld), np.nan)
    padded[:, :ncols] = q
    names = ('X', 'center', 'powers', 'derivatives_t', 'cot')
    host = [np.ascontiguousarray(given[name]) for name in names[:3]] + [np.ascontiguousarray(given['derivatives'].T), padded]
    X, center, powers, derivatives_t, cotd = t = [torch.as_tensor(a, device=device) for a in host]
    assert powers.dtype == torch.int32 and X.dtype == torch.float64
    need = int(lib.cp_taylor_vjp2_workspace_doubles(B, T))
    assert need == B * T
    results = []
    for _ in range(2):
        hess = torch.full((B * ndim * ndim + TAIL,), SENTINEL, dtype=torch.float64, device=device)
        work = torch.full((need + TAIL,), np.nan, dtype=torch.float64, device=device)
        work[need:] = SENTINEL
        _lib.check(lib.cp_taylor_vjp2(X.data_ptr(), B, center.data_ptr(), powers.data_ptr(), ndim, T, int(cfg['powers'].max()), derivatives_t.data_ptr(), M, col0, ncols,
                                      cotd.data_ptr(), ld, hess.data_ptr(), work.data_ptr(), need, 0, dv.stream_of(device)))
        torch.cuda.synchronize(device)
        hess, work = hess.cpu().numpy(), work.cpu().numpy()
        assert (hess[B * ndim * ndim:] == SENTINEL).all() and (work[need:] == SENTINEL).all(), 'written past the end'
        results.append(hess[:B * ndim * ndim].reshape(B, ndim, ndim).copy())
    assert same_bits(results[0], results[1]), 'two calls differ'
    assert same_bits(results[0], np.ascontiguousarray(results[0].transpose(0, 2, 1))), 'not symmetric bit for bit'
    for name, before, after in zip(names, host, t):
        assert np.array_equal(before, after.cpu().numpy(), equal_nan=True), name      # the inputs are read only
    return results[0]


@pytest.mark.parametrize('options', CASES, ids=[cr.case_id(case) for case in CASES])
def test_against_truth(options):
    cfg, case = cr.taylor_case(**options)
    C = run(cfg, case['q'])
    cr.assert_within(C, case, str(options))
    if options.get('order') == 1 or options.get('T') == 1:
        assert not C.any(), 'an expansion of order 1 has no second derivative: exactly 0'
    assert same_bits(run(cfg, 2. * case['q']), 2. * C), 'twice the cotangent is not exactly twice the result'


def test_a_range_is_the_polynomial_cut_to_it():
    for options in (dict(), dict(ncols=257), dict(T=70, ncols=65)):
        cfg, case = cr.taylor_case(**options)
        a, b = cfg['columns']
        small = dict(cfg, derivatives=np.ascontiguousarray(cfg['derivatives'][:, a:b]), columns=(0, b - a))
        assert same_bits(run(cfg, case['q']), run(small, case['q'], poisoned=False)), options


def test_a_point_keeps_its_bits():
    for options in (dict(), dict(ndim=7, B=7)):
        cfg, case = cr.taylor_case(**options)
        C = run(cfg, case['q'])
        for keep in (slice(2, 7), slice(3, 4)):
            assert same_bits(run(dict(cfg, X=cfg['X'][keep]), case['q'][keep]), C[keep]), (options, keep)


def test_order_one_is_exactly_zero_whatever_it_holds():
    """No term has a second derivative: every term is skipped, so neither a NaN point nor an infinite cotangent reaches the result."""
    cfg, case = cr.taylor_case(order=1, B=22)
    X, q = cfg['X'].copy(), case['q'].copy()
    X[3] = np.nan
    q[5, 7] = np.inf
    assert not run(dict(cfg, X=X), q).any()


@pytest.mark.parametrize('bad', [np.nan, np.inf])
def test_nan_and_inf_in_a_parameter(bad):
    """Parameter 1 is under power 0 in every term: NaN / Inf in it leaves C what it was, bit for bit, its own row and column exactly 0.  Parameter 2 is under
    powers <= 1: its diagonal entry is exactly 0, and with NaN / Inf in it at point 21 the entries (., 2) drop the factor and stay finite, the other entries
    of the point that hold it take it; no other point is touched."""
    cfg, case = cr.taylor_case(B=22)
    cfg['powers'][:, 1] = 0
    cfg['powers'][:, 2] = np.minimum(cfg['powers'][:, 2], 1)
    clean = run(cfg, case['q'])
    assert not clean[:, 1, :].any() and not clean[:, :, 1].any() and not clean[:, 2, 2].any()
    X = cfg['X'].copy()
    X[7, 1] = bad
    assert same_bits(run(dict(cfg, X=X), case['q']), clean)
    X[21, 2] = bad
    C = run(dict(cfg, X=X), case['q'])
    keep = np.arange(22) != 21
    assert same_bits(C[keep], clean[keep])
    assert np.isfinite(C[21, :, 2]).all() and not C[21, 1].any()


def test_nan_in_the_cotangent():
    cfg, case = cr.taylor_case(B=23)
    clean = run(cfg, case['q'])
    q = case['q'].copy()
    q[10, 3] = np.nan      # (point 10: rows 60 .. 65, across two workgroups)
    C = run(cfg, q)
    keep = np.arange(23) != 10
    used = np.abs(clean[10]) > 0      # (an entry no term reaches is skipped, not multiplied: it stays 0)
    assert np.isnan(C[10][used]).all() and same_bits(C[keep], clean[keep])


def test_engine():
    """TaylorEmulatorEngine.vjp2: the bits of the C entry point, shapes, ``columns``, ``return_value``, a strided cotangent."""
    import torch
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    cfg, case = cr.taylor_case(ndim=7, B=7)
    engine = TaylorEmulatorEngine.from_state({'center': cfg['center'], 'powers': cfg['powers'], 'derivatives': cfg['derivatives']}, device='cuda:0')
    X, (a, b), (ndim, M) = cfg['X'], cfg['columns'], (cfg['X'].shape[1], cfg['derivatives'].shape[1])
    C = run(cfg, case['q'], poisoned=False)
    got = engine.vjp2(X, case['q'], columns=(a, b))
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (len(X), ndim, ndim) and got.is_contiguous()
    assert same_bits(got.cpu().numpy(), C)
    wide = torch.zeros((len(X), M), dtype=torch.float64, device='cuda:0')
    wide[:, a:b] = torch.as_tensor(case['q'], device='cuda:0')
    v, strided = engine.vjp2(torch.as_tensor(X, device='cuda:0'), wide[:, a:b], columns=(a, b), return_value=True)      # (a view with the row stride M)
    assert torch.equal(strided, got) and torch.equal(v, engine.predict(X, columns=(a, b)))
    cr.assert_within(engine.vjp2(X, wide).cpu().numpy(), case, 'every column')
    with pytest.raises(ValueError):
        engine.vjp2(X, case['q'][:, :-1], columns=(a, b))
    with pytest.raises(ValueError):
        engine.vjp2(X[:, :-1], case['q'], columns=(a, b))
