"""GPU: ``utils.DistanceToRedshift`` over a batch of cosmologies (cp_spline_tables_build / cp_spline_tables_apply, csrc/cp_spline_tables.hip) against
the reference's own ``DistanceToRedshift`` per cosmology (tests/golden/distance_to_redshift_batch.npz, tools/gen_d2z_golden.py): spline parity on the
reference's tables, end to end from the batched cosmology's distances, round trips, isolation of rows that cannot be inverted, and the contracts of
``__call__``."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SETTINGS = [(100., 512, 3), (10., 4096, 3), (100., 512, 1)]
RTOL, ATOL = 1e-11, 1e-13      # what test_many_points_path holds cp_spline_points to against scipy's natural CubicSpline
PNAMES = ['Omega_m', 'h', 'w0_fld', 'wa_fld', 'Omega_k']


@pytest.fixture(scope='module')
def cp():
    import torch
    assert torch.cuda.is_available()
    import cosmoprimo_amd
    warnings.simplefilter('ignore')
    return cosmoprimo_amd


def tag(setting):
    return '%d_%d_%d' % setting


def table_of(g, setting):
    return g['rgrid_%d_%d' % setting[:2]]


def excess(got, ref):
    """max |got - ref| / (ATOL + RTOL |ref|): <= 1 passes the tolerance of (a)"""
    got, ref = np.asarray(got, dtype='f8'), np.asarray(ref, dtype='f8')
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())


def batch_and_singles(cp, g):
    batch = cp.Cosmology(engine='eisenstein_hu', m_ncdm=[g['m_ncdm']], **{name: g[name] for name in PNAMES})
    singles = [cp.Cosmology(engine='eisenstein_hu', m_ncdm=[float(g['m_ncdm'][i])], **{name: float(g[name][i]) for name in PNAMES}) for i in range(g['h'].size)]
    return batch, singles


@pytest.mark.parametrize('setting', SETTINGS, ids=tag)
def test_spline_parity_on_the_reference_tables(cp, golden, setting):
    """(a) The reference's own tables through a callable: the batched object reproduces the reference's redshifts, per-cosmology and shared queries, numpy
    and device-resident input."""
    import torch
    from cosmoprimo_amd.utils import DistanceToRedshift
    g = golden('distance_to_redshift_batch')
    zmax, nz, order = setting
    rgrid = table_of(g, setting)
    d, z, ds, zs = (g[name + tag(setting)] for name in ('d_', 'z_', 'ds_', 'zs_'))
    for table in (rgrid, torch.as_tensor(rgrid, device='cuda')):
        d2z = DistanceToRedshift(lambda zgrid: table, zmax=zmax, nz=nz, interp_order=order)
        got = d2z(d, per_cosmology=True)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
        shared = d2z(ds)
        gpu = d2z(torch.as_tensor(d, device='cuda'), per_cosmology=True)
        gpu_shared = d2z(torch.as_tensor(ds, device='cuda'))
        assert gpu.is_cuda and gpu_shared.is_cuda and gpu.dtype == torch.float64
        errs = [excess(got, z), excess(shared, zs), excess(gpu.cpu().numpy(), z), excess(gpu_shared.cpu().numpy(), zs)]
        print('parity %s: max |dz| / (1e-13 + 1e-11 |z|) = %.3e (per cosmology), %.3e (shared)' % (tag(setting), errs[0], errs[1]))
        assert max(errs) <= 1., errs
        assert np.array_equal(got, gpu.cpu().numpy()) and np.array_equal(shared, gpu_shared.cpu().numpy())


@pytest.mark.parametrize('setting', SETTINGS, ids=tag)
def test_end_to_end_from_the_batched_cosmology(cp, golden, setting):
    """(b) The object built from the batched cosmology's own distances against the fixture.  The yardstick is today's object, one cosmology at a time
    (unchanged): the batch may miss the fixture by 4 times the loop's largest error (another, equally valid order of operations in the solve) and
    agrees with the loop at the tolerance of (a)."""
    from cosmoprimo_amd.utils import DistanceToRedshift
    g = golden('distance_to_redshift_batch')
    zmax, nz, order = setting
    d, z = g['d_' + tag(setting)], g['z_' + tag(setting)]
    # the end knots of the reference's table need not lie inside this package's (distances agree to rounding only): queries strictly inside both
    inside = (d > table_of(g, setting)[:, :1] * (1. + 1e-9) + 1e-9) & (d < table_of(g, setting)[:, -1:] * (1. - 1e-9))
    batch, singles = batch_and_singles(cp, g)
    got = DistanceToRedshift(batch.get_background().comoving_radial_distance, zmax=zmax, nz=nz, interp_order=order)(d, bounds_error=False, per_cosmology=True)
    loop = np.array([DistanceToRedshift(c.get_background().comoving_radial_distance, zmax=zmax, nz=nz, interp_order=order)(d[i], bounds_error=False)
                     for i, c in enumerate(singles)])
    assert inside.sum() > 0.95 * inside.size and np.isfinite(got[inside]).all() and np.isfinite(loop[inside]).all()
    err_loop, err_batch = np.abs(loop - z)[inside].max(), np.abs(got - z)[inside].max()
    mutual = excess(got[inside], loop[inside])
    print('end to end %s: max |dz| loop %.3e, batch %.3e; batch against loop, in units of the tolerance: %.3e' % (tag(setting), err_loop, err_batch, mutual))
    assert err_batch <= 4. * err_loop, (err_batch, err_loop)
    assert mutual <= 1., mutual


def test_round_trip(cp, golden):
    """(c) z -> D_C -> z and z -> D_L -> z for the batch, as test_distance_to_redshift asserts for one cosmology."""
    from cosmoprimo_amd.utils import DistanceToRedshift
    g = golden('distance_to_redshift_batch')
    batch, _ = batch_and_singles(cp, g)
    ba = batch.get_background()
    z = np.random.default_rng(0).uniform(0., 2., 1000)
    for distance in (ba.comoving_radial_distance, ba.luminosity_distance):
        d2z = DistanceToRedshift(distance, zmax=10., nz=4096)
        d = np.asarray(distance(z))
        assert d.shape == (g['h'].size, z.size)
        back = d2z(d, per_cosmology=True)
        print('round trip: max |dz| = %.3e' % np.abs(back - z).max())
        assert np.allclose(back, np.broadcast_to(z, back.shape), atol=1e-6)


def normal_params(n, seed):
    rng = np.random.default_rng(seed)
    return dict(h=rng.uniform(0.6, 0.8, n), Omega_cdm=rng.uniform(0.2, 0.3, n), Omega_b=rng.uniform(0.04, 0.06, n), Omega_k=rng.uniform(-0.05, 0.05, n),
                w0_fld=rng.uniform(-1.2, -0.8, n), wa_fld=rng.uniform(-0.3, 0.3, n))


@pytest.mark.parametrize('n', [65, 256, 3072])
def test_rows_that_cannot_be_inverted_stay_alone(cp, n):
    """(d) A cosmology with NaN distances (the corner wa_overflow: w0 = -1, wa = -300), then a table that is not ascending, at rows 0, 63 and 64: NaN rows,
    and every other row bit for bit as in the batch without them."""
    import torch
    from cosmoprimo_amd import background as bgm
    from cosmoprimo_amd.utils import DistanceToRedshift
    positions = [0, 63, 64]
    zgrid = 1. / np.geomspace(1. / 101., 1., 512)[::-1] - 1.
    p = normal_params(n, n)
    pc = {name: v.copy() for name, v in p.items()}
    pc['w0_fld'][positions], pc['wa_fld'][positions] = -1., -300.
    zt = torch.as_tensor(zgrid, device='cuda')
    clean = bgm.distance('comoving_radial_distance', zt, params=p)
    corner = bgm.distance('comoving_radial_distance', zt, params=pc)
    assert clean.shape == (n, 512) and bool(torch.isnan(corner[positions]).any(dim=1).all())
    swapped = clean.clone()
    swapped[positions, 200], swapped[positions, 201] = clean[positions, 201], clean[positions, 200]
    others = torch.ones(n, dtype=torch.bool, device='cuda')
    others[positions] = False
    rng = np.random.default_rng(n)
    lo, hi = clean[:, :1], clean[:, -1:]
    per_row = lo + torch.as_tensor(rng.uniform(0., 1., (n, 40)), device='cuda') * (hi - lo)
    shared = torch.as_tensor(rng.uniform(0., 1., 5000), device='cuda') * float(hi.min())      # the catalogue regime
    ref = DistanceToRedshift(lambda z: clean)
    want_rows, want_shared = ref(per_row, bounds_error=False, per_cosmology=True), ref(shared, bounds_error=False)
    assert bool(torch.isfinite(want_rows).all())
    for table in (corner, swapped):
        d2z = DistanceToRedshift(lambda z: table)
        for got, want in ((d2z(per_row, bounds_error=False, per_cosmology=True), want_rows), (d2z(shared, bounds_error=False), want_shared)):
            assert bool(torch.isnan(got[positions]).all())
            assert torch.equal(got[others], want[others])
        d2z(shared, bounds_error=True)      # inside every table that can be inverted: the rows that cannot do not count as out of range


def test_contracts(cp, golden):
    """(e) Shapes, dtypes, containers, bounds and the two launch regimes."""
    import torch
    from cosmoprimo_amd.utils import DistanceToRedshift
    g = golden('distance_to_redshift_batch')
    rgrid = g['rgrid_100_512']
    nb, nz = rgrid.shape
    zgrid = 1. / np.geomspace(1. / 101., 1., nz)[::-1] - 1.
    d2z = DistanceToRedshift(lambda z: rgrid)
    ds = g['ds_100_512_3']
    full = d2z(ds)
    # scalar, n-d and empty queries
    assert d2z(float(ds[3])).shape == (nb,) and np.array_equal(d2z(float(ds[3])), full[:, 3])
    assert d2z(ds[:24].reshape(2, 3, 4)).shape == (nb, 2, 3, 4) and np.array_equal(d2z(ds[:24].reshape(2, 3, 4)).reshape(nb, 24), full[:, :24])
    assert d2z(np.zeros((0,))).shape == (nb, 0) and d2z(np.zeros((3, 0))).shape == (nb, 3, 0)
    per = np.broadcast_to(ds[:24], (nb, 24)).reshape(nb, 2, 12).copy()
    assert d2z(per, per_cosmology=True).shape == (nb, 2, 12) and np.array_equal(d2z(per, per_cosmology=True).reshape(nb, 24), full[:, :24])
    assert d2z(ds[:nb].copy(), per_cosmology=True).shape == (nb,)
    assert d2z(np.zeros((nb, 0)), per_cosmology=True).shape == (nb, 0)
    with pytest.raises(ValueError):
        d2z(ds[:nb + 1], per_cosmology=True)
    # B = 1
    one = DistanceToRedshift(lambda z: rgrid[:1])
    assert one(ds).shape == (1, ds.size) and np.array_equal(one(ds)[0], full[0])
    # float32 in, float32 out: the float64 result rounded once
    d32 = ds.astype('f4')
    got32 = d2z(d32)
    assert got32.dtype == np.float32 and np.array_equal(got32, d2z(d32.astype('f8')).astype('f4'))
    t32 = d2z(torch.as_tensor(d32, device='cuda'))
    assert t32.dtype == torch.float32 and t32.is_cuda and np.array_equal(t32.cpu().numpy(), got32)
    t64 = d2z(torch.as_tensor(ds, device='cuda'))
    assert t64.is_cuda and t64.device == torch.device('cuda', torch.cuda.current_device()) and np.array_equal(t64.cpu().numpy(), full)
    # a query outside one row's table and inside another's
    top = np.sort(rgrid[:, -1])
    q = np.array([ds[5], 0.5 * (top[0] + top[-1]), ds[7]])
    with pytest.raises(ValueError):
        d2z(q)
    with pytest.raises(ValueError):
        d2z(q, bounds_error=True)
    soft = d2z(q, bounds_error=False)
    expect_nan = np.zeros((nb, 3), dtype=bool)
    expect_nan[:, 1] = q[1] > rgrid[:, -1]
    assert expect_nan.any() and not expect_nan[:, 1].all() and np.array_equal(np.isnan(soft), expect_nan)
    assert np.isnan(d2z(np.array([np.nan]), bounds_error=False)).all()
    # the end knots are inside
    ends = d2z(rgrid[:, [0, -1]].copy(), bounds_error=True, per_cosmology=True)
    assert np.allclose(ends, zgrid[[0, -1]], rtol=1e-12, atol=1e-14)
    # orders
    with pytest.raises(NotImplementedError):
        DistanceToRedshift(lambda z: rgrid, interp_order=2)
    with pytest.raises(ValueError):      # one cosmology has no per-cosmology queries
        DistanceToRedshift(lambda z: rgrid[0])(ds[:nb], per_cosmology=True)
    # the two launch regimes: 8 rows x 10^6 queries (rows staged in LDS), 2 10^4 rows x 8 queries (bisection in memory); bit for bit on what they share
    rng = np.random.default_rng(5)
    many = torch.as_tensor(ds[0] + rng.uniform(0., 1., 10**6) * (ds[-1] - ds[0]), device='cuda')
    catalogue = d2z(many)
    assert catalogue.shape == (nb, 10**6) and bool(torch.isfinite(catalogue).all())
    nrows = 20000
    scale = 1. + 1e-3 * (np.arange(nrows) // nb)[:, None]
    big = np.tile(rgrid, (nrows // nb, 1)) * scale
    samples = DistanceToRedshift(lambda z: torch.as_tensor(big, device='cuda'))
    queries = (many[:8][None, :] * torch.as_tensor(scale, device='cuda')).contiguous()
    few = samples(queries, per_cosmology=True)
    assert few.shape == (nrows, 8) and torch.equal(few[:nb], catalogue[:, :8])
    # ... and both against scipy on a few rows
    from scipy.interpolate import CubicSpline
    for row in (0, 5, 4003, nrows - 1):
        ref = CubicSpline(big[row], zgrid, bc_type='natural')(queries[row].cpu().numpy())
        assert excess(few[row].cpu().numpy(), ref) <= 1.
    ref = CubicSpline(rgrid[3], zgrid, bc_type='natural')(many[::997].cpu().numpy())
    assert excess(catalogue[3, ::997].cpu().numpy(), ref) <= 1.
