"""
Knot families and queries of the edge cases of ``cp_spline_tables_build`` / ``cp_spline_tables_apply`` (csrc/cp_spline_tables.hip), shared by
``tools/gen_spline_tables_edges_golden.py`` (which computes the truth in extended precision and stores it with the queries in
``tests/golden/spline_tables_edges.npz``) and ``tests/test_spline_tables_edges_gpu.py`` (which rebuilds the knots from here).  numpy only.

A family is a fixed expression for the SPACINGS of n knots (fixed ``default_rng`` seeds where it is random), accumulated with ``cumsum`` and mapped
onto [1, 5000] by one shift and one scale, so that the tables of all families overlap and a batch of them can be asked shared queries:
  uniform    equal spacings
  geom1.05   spacings 1.05^i (i <= 600): a distance table seen through a steep map, ratio of neighbours 1.05
  saw1.5x16  spacings 1.5^(i mod 16): a drop by 1.5^15 = 438 every 16 knots
  saw2x40    spacings 2^(i mod 40): a drop by 2^39 every 40 knots -- the elimination of the build forgets its start by almost 1/2 per knot
             only along such a ramp, longer than the halo of a lane
  alt1e3     spacings alternating 1 and 1e-3
  jitter100  spacings 10^U(-2, 0)
The values are always ``DistanceToRedshift``'s own redshift grid for zmax = 100.
"""
import numpy as np

FAMILIES = ['uniform', 'geom1.05', 'saw1.5x16', 'saw2x40', 'alt1e3', 'jitter100']
SIZES = [2, 3, 4, 5, 33, 34, 65, 66, 129, 130, 193, 512]      # the runs of the build change at 65 / 66 (1 -> 3 intervals per lane), 129 / 130, 193
LARGE_SIZES = [2048, 2049, 4096]                              # apply: rows staged in LDS up to 2048 knots; build: at most 4096
LARGE_FAMILIES = ['uniform', 'jitter100']
ORDERS = [3, 1]
ZMAX = 100.
NQ, NQ_SHARED = 256, 128
RTOL, ATOL = 1e-11, 1e-13      # the tolerance of tests/test_distance_to_redshift_batch_gpu.py


def table_run(n):
    """Intervals per lane of the build (``table_run`` of csrc/cp_spline_tables.hip)."""
    return ((n - 1 + 63) // 64) | 1


def zgrid(n, zmax=ZMAX):
    """The redshift grid of ``DistanceToRedshift(zmax=zmax, nz=n)``."""
    return 1. / np.geomspace(1. / (1. + zmax), 1., n)[::-1] - 1.


def spacings(name, n):
    i = np.arange(n - 1)
    if name == 'uniform':
        return np.ones(n - 1)
    if name == 'geom1.05':
        return 1.05**np.minimum(i, 600)
    if name == 'saw1.5x16':
        return 1.5**(i % 16)
    if name == 'saw2x40':
        return 2.**(i % 40)
    if name == 'alt1e3':
        return np.where(i % 2, 1e-3, 1.)
    if name == 'jitter100':
        return 10.**np.random.default_rng(100 + n).uniform(-2., 0., n - 1)
    raise ValueError('unknown family {}'.format(name))


def knots(name, n):
    """The n knots of family ``name``: strictly ascending, from 1 to (within rounding) 5000."""
    c = np.concatenate([[0.], np.cumsum(spacings(name, n))])
    x = 1. + c * (4999. / c[-1])
    assert x.shape == (n,) and np.isfinite(x).all() and (np.diff(x) > 0.).all(), (name, n)
    return x


def families(n):
    return FAMILIES if n in SIZES else LARGE_FAMILIES


def cases():
    """Every (n, family) of the fixture."""
    return [(n, name) for n in SIZES + LARGE_SIZES for name in families(n)]


def batch(n):
    """(families, n): the tables of one size stacked as the rows of one batch."""
    return np.array([knots(name, n) for name in families(n)])


def _seed(name, n):
    return 7919 * n + FAMILIES.index(name)


def queries(name, n):
    """The NQ queries of one case, all inside the table: both end knots and their neighbours inside the table, every knot at a multiple of
    ``table_run(n)`` (where one lane's intervals end and the next one's begin) with its two neighbours, ``nextafter`` in both directions of a few
    interior knots, the midpoints of the first two and the last two intervals, and random points for the rest -- two in three uniform within an
    interval drawn uniformly (every interval counts alike however short), one in three uniform in the table's range."""
    x = knots(name, n)
    rng = np.random.default_rng(_seed(name, n))
    run = table_run(n)
    q = [x[0], x[-1], np.nextafter(x[0], np.inf), np.nextafter(x[-1], -np.inf)]
    for k in range(0, n, run):
        q += [x[j] for j in (k - 1, k, k + 1) if 0 <= j < n]
    for k in sorted(set(j for j in (1, run, 2 * run, n // 3, n // 2, n - 1 - run, n - 2) if 0 < j < n - 1)):
        q += [np.nextafter(x[k], -np.inf), np.nextafter(x[k], np.inf)]
    for k in sorted(set(j for j in (0, 1, n - 3, n - 2) if 0 <= j < n - 1)):
        q.append(0.5 * (x[k] + x[k + 1]))
    q = np.array(q)
    assert q.size <= NQ, (name, n, q.size)
    nrand = NQ - q.size
    k = rng.integers(0, n - 1, nrand)
    inside = x[k] + rng.uniform(0., 1., nrand) * (x[k + 1] - x[k])
    anywhere = x[0] + rng.uniform(0., 1., nrand) * (x[-1] - x[0])
    q = np.concatenate([q, np.where(np.arange(nrand) % 3 < 2, inside, anywhere)])
    return np.clip(q, x[0], x[-1])


def shared_queries(n):
    """NQ_SHARED queries inside the tables of ALL families of size n: a strided pick from every family's own queries (its knots among them), moved
    into the range that the tables share (their last knots differ by rounding)."""
    names = families(n)
    x = batch(n)
    lo, hi = x[:, 0].max(), x[:, -1].min()
    per = NQ_SHARED // len(names)
    q = np.concatenate([queries(name, n)[i::len(names)][:per] for i, name in enumerate(names)])
    rng = np.random.default_rng(_seed('uniform', n) + 1)
    q = np.concatenate([q, lo + rng.uniform(0., 1., NQ_SHARED - q.size) * (hi - lo)])
    return np.clip(q, lo, hi)


def excess(got, truth):
    """max |got - truth| / (ATOL + RTOL |truth|): <= 1 passes."""
    got, truth = np.asarray(got, dtype='f8'), np.asarray(truth, dtype='f8')
    assert got.shape == truth.shape, (got.shape, truth.shape)
    assert np.isfinite(got).all()
    return float((np.abs(got - truth) / (ATOL + RTOL * np.abs(truth))).max())
