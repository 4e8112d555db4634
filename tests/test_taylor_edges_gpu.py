"""GPU: the GEMM of the Taylor emulator (cp_taylor_predict / cp_taylor_fit, csrc/cp_taylor.hip) at the edges of its tiles -- 64 rows x 256 columns per
workgroup, 64 columns per wave, chunks of 32 inner indices in two alternating LDS buffers, MFMA steps of 4 taken in pairs -- with operands drawn from
``default_rng``, all distinct: a result stored in the wrong tile, row or column cannot pass, as it can with the tiled operands of
tests/test_taylor_gpu.py::test_predict_tiled.

Truth: formed at run time in ``np.longdouble`` (monomials by ``**``, then the product), rounded to float64 once.
Tolerance (derived, not measured): ``dot_bound`` of tests/test_taylor_gpu.py, ``2 (n + degree + 2) eps sum_i |A_ti| |B_im|`` with n the non-zero
entries of the row of A, and in the place of ``ndim`` the largest total degree of a term -- the multiplications that form a monomial by repeated
multiplication -- or 0 for the fit, whose left operand is given.  The factor 2 covers a platform whose longdouble is no wider than double."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = 2.**-53
LD = np.longdouble
BASE = dict(B=65, M=257, T=33, ndim=3)


def dot_bound(A, B, degree):
    n = (A != 0).sum(axis=1)
    return (2 * (n + degree + 2))[:, None] * EPS * (np.abs(A) @ np.abs(B))


def monomials(X, center, powers, dtype='f8'):
    """(B, T), a factor of power 0 being exactly 1 whatever the parameter holds (the reference's ``where``)."""
    d = np.asarray(X, dtype=dtype) - np.asarray(center, dtype=dtype)
    mono = np.ones((len(d), len(powers)), dtype=dtype)
    for t, power in enumerate(powers):
        for j, p in enumerate(power):
            if p > 0:
                mono[:, t] *= d[:, j]**int(p)
    return mono


def operands(B, M, T, ndim, seed, powers=None):
    rng = np.random.default_rng(seed)
    center = rng.uniform(-1., 1., ndim)
    X = center + rng.uniform(-1.5, 1.5, (B, ndim))
    if powers is None:
        powers = rng.integers(0, 4, (T, ndim))
    derivatives = rng.normal(0., 1., (T, M))
    assert np.unique(X).size == X.size and np.unique(derivatives).size == derivatives.size
    return X, center, np.asarray(powers, dtype='i4'), derivatives


def engine_of(center, powers, derivatives):
    from cosmoprimo_amd.emulators import TaylorEmulatorEngine
    return TaylorEmulatorEngine.from_state({'center': center, 'powers': powers, 'derivatives': derivatives}, device='cuda:0')


def predict_fraction(X, center, powers, derivatives):
    """Largest fraction of the bound that ``predict`` uses against the longdouble truth."""
    got = engine_of(center, powers, derivatives).predict(X).cpu().numpy()
    truth = np.asarray(monomials(X, center, powers, dtype=LD) @ derivatives.astype(LD), dtype='f8')
    assert got.shape == truth.shape == (len(X), derivatives.shape[1]) and np.isfinite(got).all()
    bound = dot_bound(monomials(X, center, powers), derivatives, int(powers.sum(axis=1).max()))
    return float((np.abs(got - truth) / bound).max())


SWEEP = ([('B', v) for v in (1, 63, 64, 65, 129)] + [('M', v) for v in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)]
         + [('T', v) for v in (1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 97)])


@pytest.mark.parametrize('name,value', SWEEP, ids=['%s%d' % item for item in SWEEP])
def test_predict_one_dimension_at_a_time(name, value):
    """1. Around B = 65, M = 257, T = 33, ndim = 3 with random powers 0 .. 3: the ends of the row tile (64), of a wave's columns (64) and a lane group's
    (16), of the workgroup's columns (256), of the chunk (32: T = 65 and 97 use a buffer for the second time) and of the MFMA pairs (T mod 8)."""
    shape = dict(BASE, **{name: value})
    fraction = predict_fraction(*operands(seed=1000 * len(name) + value, **shape))
    print('predict %s: %.3g of the bound' % (shape, fraction))
    assert fraction <= 1.


def test_predict_corner():
    """1. Every dimension ragged in its last tile at once: B = 129, M = 513, T = 97."""
    fraction = predict_fraction(*operands(129, 513, 97, 3, seed=11))
    print('predict corner: %.3g of the bound' % fraction)
    assert fraction <= 1.


@pytest.mark.parametrize('ndim', [1, 32])
def test_predict_ndim(ndim):
    """1. One parameter, and the 32 that the LDS tail of x - center holds: one term with all 32 powers equal to 1, one with a power of 15 (ndim = 32: few
    factors per term otherwise, so that the monomials stay within range; x - center in (-1.5, 1.5))."""
    rng = np.random.default_rng(ndim)
    T = BASE['T']
    if ndim == 1:
        powers = rng.integers(0, 4, (T, 1))
        powers[5] = 15
    else:
        powers = np.where(rng.uniform(0., 1., (T, ndim)) < 0.1, rng.integers(1, 4, (T, ndim)), 0)
        powers[3] = 1
        powers[7] = 0
        powers[7, [0, 31]] = 15, 2
        powers[8] = 0
        powers[8, 31] = 3
    fraction = predict_fraction(*operands(BASE['B'], BASE['M'], T, ndim, seed=50 + ndim, powers=powers))
    print('predict ndim = %d: %.3g of the bound' % (ndim, fraction))
    assert fraction <= 1.


def fit_on_device(S, Y, rows_allocated=None):
    """cp_taylor_fit as ``TaylorEmulatorEngine.fit`` calls it; the result buffer may hold more rows than T (filled with a sentinel)."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    device = torch.device('cuda', 0)
    Sd, Yd = (torch.as_tensor(np.ascontiguousarray(a, dtype='f8'), device=device) for a in (S, Y))
    (T, npoints), M = S.shape, Y.shape[1]
    out = torch.full((rows_allocated or T, M), -7.25, dtype=torch.float64, device=device)
    _lib.check(_lib.load().cp_taylor_fit(Sd.data_ptr(), T, npoints, Yd.data_ptr(), M, out.data_ptr(), device.index, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    return out.cpu().numpy()


FIT_BASE = dict(T=65, npoints=33, M=257)
FIT_SWEEP = [('T', v) for v in (1, 63, 64, 65)] + [('npoints', v) for v in (1, 7, 31, 32, 33, 65)] + [('M', v) for v in (1, 255, 257)] + [('sparse', 3)]


@pytest.mark.parametrize('name,value', FIT_SWEEP, ids=['%s%d' % item for item in FIT_SWEEP])
def test_fit_dense(name, value):
    """2. derivatives = S . Y through the staging of a given left operand, on dense random S (the sampler's S has a few non-zeros per row, which is all
    that tests/test_taylor_gpu.py drives it with), one dimension at a time around T = 65, npoints = 33, M = 257; and one S with three non-zeros per row."""
    shape = dict(FIT_BASE)
    if name != 'sparse':
        shape[name] = value
    rng = np.random.default_rng(2000 + 10 * len(name) + value)
    S = rng.normal(0., 1., (shape['T'], shape['npoints']))
    if name == 'sparse':
        keep = np.zeros(S.shape, dtype=bool)
        for row in keep:
            row[rng.choice(shape['npoints'], value, replace=False)] = True
        S[~keep] = 0.
    Y = rng.normal(0., 1., (shape['npoints'], shape['M']))
    got = fit_on_device(S, Y)
    truth = np.asarray(S.astype(LD) @ Y.astype(LD), dtype='f8')
    fraction = float((np.abs(got - truth) / dot_bound(S, Y, 0)).max())
    print('fit %s%s: %.3g of the bound' % (shape, ' (3 non-zeros per row)' if name == 'sparse' else '', fraction))
    assert got.shape == truth.shape and fraction <= 1.


@pytest.mark.parametrize('B', [63, 65])
def test_nothing_is_stored_past_the_end(B):
    """3. The result allocated with one row more than asked for, holding a sentinel: the rows of the last tile past B (and the columns of the last
    column tile past M, which would land in the next row) are not stored.  M = 257: the second column tile holds one column."""
    import torch
    from cosmoprimo_amd import _device as dv, _lib
    X, center, powers, derivatives = operands(B, BASE['M'], BASE['T'], BASE['ndim'], seed=300 + B)
    M, (T, ndim) = derivatives.shape[1], powers.shape
    device = torch.device('cuda', 0)
    Xd, cd, pd, dd = (torch.as_tensor(np.ascontiguousarray(a), device=device) for a in (X, center, powers, derivatives))
    assert pd.dtype == torch.int32
    out = torch.full((B + 1, M), -7.25, dtype=torch.float64, device=device)
    _lib.check(_lib.load().cp_taylor_predict(Xd.data_ptr(), B, cd.data_ptr(), pd.data_ptr(), ndim, T, int(powers.max()), dd.data_ptr(), M, out.data_ptr(),
                                             device.index, dv.stream_of(device)))
    torch.cuda.synchronize(device)
    out = out.cpu().numpy()
    assert (out[B] == -7.25).all()
    assert np.array_equal(out[:B], engine_of(center, powers, derivatives).predict(X).cpu().numpy()) and (out[:B] != -7.25).all()
    # the fit: B rows of a given left operand
    rng = np.random.default_rng(B)
    S, Y = rng.normal(0., 1., (B, 33)), rng.normal(0., 1., (33, M))
    out = fit_on_device(S, Y, rows_allocated=B + 1)
    assert (out[B] == -7.25).all() and np.array_equal(out[:B], fit_on_device(S, Y))


def same_pattern(got, X, center, powers, derivatives):
    """The NaN pattern of numpy's product of the same operands (and the same bits wherever neither is NaN and the truth is finite is not asked: the
    order of the sums differs)."""
    with np.errstate(all='ignore'):
        want = monomials(X, center, powers) @ derivatives
    return np.array_equal(np.isnan(got), np.isnan(want))


def test_containment_rows_of_x():
    """4. NaN and Inf in row r of X change row r alone (r at both sides of the row tiles' border), and only through a parameter with a positive power."""
    X, center, powers, derivatives = operands(130, BASE['M'], BASE['T'], 4, seed=41)
    powers[:, 1] = 0      # no term depends on parameter 1
    engine = engine_of(center, powers, derivatives)
    clean = engine.predict(X).cpu().numpy()
    for value in (np.nan, np.inf, -np.inf):
        for column, touched in ((1, False), (0, True), (3, True)):
            rows = [0, 63, 64, 129]
            Xb = X.copy()
            Xb[rows, column] = value
            got = engine.predict(Xb).cpu().numpy()
            others = np.ones(len(X), dtype=bool)
            others[rows] = False
            assert np.array_equal(got[others], clean[others])
            assert same_pattern(got, Xb, center, powers, derivatives)
            if touched:
                assert not np.isfinite(got[rows]).any()      # every row of ``derivatives`` is dense: a term that is not finite reaches every column
            else:
                assert np.array_equal(got[rows], clean[rows])


def test_containment_columns_of_derivatives():
    """4. NaN in column m of ``derivatives`` changes column m alone (m at the borders of the lane groups, the waves and the workgroups)."""
    X, center, powers, derivatives = operands(BASE['B'], 513, BASE['T'], BASE['ndim'], seed=42)
    clean = engine_of(center, powers, derivatives).predict(X).cpu().numpy()
    columns = [0, 15, 16, 63, 64, 255, 256, 512]
    bad = derivatives.copy()
    bad[np.arange(len(columns)) * 4 % BASE['T'], columns] = np.nan
    got = engine_of(center, powers, bad).predict(X).cpu().numpy()
    others = np.ones(513, dtype=bool)
    others[columns] = False
    assert np.isnan(got[:, columns]).all() and np.array_equal(got[:, others], clean[:, others])
    assert same_pattern(got, X, center, powers, bad)


@pytest.mark.parametrize('T', [33, 37])
def test_last_row_of_derivatives_is_not_padding(T):
    """4. T = 33 and 37 end one and five terms into a chunk whose other rows are masked off: a NaN in the last row of ``derivatives`` reaches the result."""
    X, center, powers, derivatives = operands(BASE['B'], BASE['M'], T, BASE['ndim'], seed=43 + T)
    columns = [0, 100, 256]
    derivatives[T - 1, columns] = np.nan
    got = engine_of(center, powers, derivatives).predict(X).cpu().numpy()
    expect = np.zeros(got.shape, dtype=bool)
    expect[:, columns] = True
    assert np.array_equal(np.isnan(got), expect) and same_pattern(got, X, center, powers, derivatives)
