"""
Finite-difference sampler under the reference's name (cosmoprimo/emulators/tools/samples.py:574-669): ``DiffSampler`` lays out the grid of parameter
points a Taylor expansion of given order and accuracy needs, and evaluates the calculator on it.  The reference evaluates one clone per grid point;
here the whole grid is ONE call of the calculator, every parameter an array of ``npoints`` values -- what ``get_calculator`` is made for.

``QMCSampler`` (reference samples.py:672-714) draws quasi-random points over the box of the limits for the MLP engine and evaluates them the same way.

No MPI, no ``save_fn`` / resume, no ``InputSampler`` / ``GridSampler``.
"""
import fnmatch

import numpy as np


def deriv_ncoeffs(order, acc=2):
    """Number of nodes of the central stencil of a derivative of given order and accuracy (reference taylor.py:9-11)."""
    return 2 * ((order + 1) // 2) - 1 + acc


class Samples(dict):

    """Parameter name -> (npoints,) array, with ``attrs`` (``cidx``, ``order``, ``accuracy``); after :meth:`DiffSampler.run` also ``varied``
    (output key -> (npoints,) + shape array) and ``fixed`` (output key -> the calculator's value, the same for every point)."""

    def __init__(self, *args, attrs=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.attrs = dict(attrs or {})
        self.varied, self.fixed = {}, {}

    def matrix(self):
        """(npoints, ndim) array of the parameter points."""
        return np.column_stack([np.asarray(v, dtype='f8') for v in self.values()])


def _expand(item, names):
    """A value per parameter name from a single value or a dictionary (names or wildcards; parameters it does not name get ``None``)."""
    if not isinstance(item, dict):
        return {name: item for name in names}
    toret = {name: None for name in names}
    for pattern, value in item.items():
        for name in fnmatch.filter(names, pattern):
            toret[name] = value
    return toret


def _pruned_grid(axes, used=0):
    """Points of the tensor grid of ``axes`` = [(coordinates, tag per node, maximum order)], a node kept only if its tag (the least derivative order whose
    stencil reaches it) and the tags already ``used`` along the later axes can be orders of one term.  The last axis varies slowest, tags descending
    (the reference's order, taylor.py:153-177)."""
    coords, tags, maxorder = axes[-1]
    points = []
    for tag in sorted(set(tags.tolist()), reverse=True):
        if tag and tag + used > maxorder:
            continue
        heads = _pruned_grid(axes[:-1], used + tag) if len(axes) > 1 else [()]
        nodes = coords[tags == tag]
        points += [head + (x,) for head in heads for x in nodes]
    return points


def rqrs_points(ndim, n, seed=0.5):
    """First ``n`` points of the R quasi-random sequence in ``ndim`` dimensions, (n, ndim) in [0, 1): point i = 1 .. n has the coordinates
    ``(seed + i g^-k) mod 1``, k = 1 .. ndim, with g > 1 the root of ``g^(ndim + 1) = g + 1`` (the generalised golden ratio), found by Newton's method
    from 1 until the residual is below 1e-12.  Same operations in the same order as the reference's ``RQuasiRandomSequence`` (samples.py:286-311), because
    the points have to equal its points bit for bit (tests/test_mlp_host.py::test_qmc_points)."""
    def residual(g):
        return g**(ndim + 1) - g - 1

    root = 1.
    while abs(residual(root)) > 1e-12:
        slope = (ndim + 1) * root**ndim - 1
        root = root - residual(root) / slope
    steps = [root**(-k) for k in range(1, ndim + 1)]
    index = np.arange(1, n + 1).reshape(n, 1)
    return np.mod(float(seed) + index * steps, 1.)


class QMCSampler(object):

    """Quasi Monte-Carlo samples over the box of the parameters' limits (reference samples.py:672-714; engine :class:`MLPEmulatorEngine`): 'sobol',
    'halton', 'lhs' of :mod:`scipy.stats.qmc` or 'rqrs', the R quasi-random sequence.  The calculator is evaluated on all points in one batched call."""

    def __init__(self, calculator, params, engine='rqrs', **kwargs):
        """``kwargs``: arguments of the engine, e.g. ``seed`` (for 'rqrs' the offset of the sequence, 0.5 by default)."""
        self.calculator = calculator
        self.params = {name: tuple(float(v) for v in limits) for name, limits in params.items()}
        if not self.params:
            raise ValueError('Provide at least one parameter')
        if engine not in ('sobol', 'halton', 'lhs', 'rqrs'):
            raise ValueError("engine must be one of 'sobol', 'halton', 'lhs', 'rqrs', got {!r}".format(engine))
        self.engine, self.engine_options = engine, dict(kwargs)
        self.samples = None

    def points(self, niterations=300):
        """``niterations`` points scaled to the limits, as :class:`Samples`."""
        from scipy.stats import qmc
        ndim = len(self.params)
        if self.engine == 'rqrs':
            unit = rqrs_points(ndim, int(niterations), **self.engine_options)
        else:
            cls = {'sobol': qmc.Sobol, 'halton': qmc.Halton, 'lhs': qmc.LatinHypercube}[self.engine]
            unit = cls(d=ndim, **self.engine_options).random(n=int(niterations))
        X = qmc.scale(unit, [limits[0] for limits in self.params.values()], [limits[1] for limits in self.params.values()])
        return Samples({name: X[:, i].copy() for i, name in enumerate(self.params)}, attrs={'params': dict(self.params)})

    def run(self, niterations=300, batch_size=None):
        """Evaluate the calculator on all points in one batched call (or in chunks of ``batch_size`` points) and once at the centre of the box (scalars:
        the unbatched shapes, which tell *varied* from *fixed* outputs as in :meth:`DiffSampler.run`).  Points with a non-finite varied output are
        dropped from parameters and outputs alike (the reference masks failed samples); ``attrs['ndropped']`` counts them."""
        samples = self.points(niterations)
        npoints = int(niterations)
        center = self.calculator(**{name: float(np.mean(limits)) for name, limits in self.params.items()})
        batch_size = npoints if not batch_size else int(batch_size)
        chunks = []
        for start in range(0, npoints, batch_size):
            chunks.append(self.calculator(**{name: np.array(value[start:start + batch_size]) for name, value in samples.items()}))
        good = np.ones(npoints, dtype=bool)
        for key, first in (chunks[0] if chunks else {}).items():
            sizes = [min(batch_size, npoints - start) for start in range(0, npoints, batch_size)]
            if key in center and all(np.shape(chunk[key]) == (size,) + np.shape(center[key]) for chunk, size in zip(chunks, sizes)):
                value = np.concatenate([np.asarray(chunk[key]) for chunk in chunks], axis=0)
                good &= np.isfinite(value.reshape(npoints, -1)).all(axis=1)
                samples.varied[key] = value
            else:
                samples.fixed[key] = np.asarray(first)
        for key in samples.varied:
            samples.varied[key] = samples.varied[key][good]
        for name in list(samples):
            samples[name] = samples[name][good]
        samples.attrs['ndropped'] = int(npoints - good.sum())
        self.samples = samples
        return samples


class DiffSampler(object):

    """Sample points for finite differentiation (engine :class:`TaylorEmulatorEngine`)."""

    def __init__(self, calculator, params, order=1, accuracy=2):
        """
        Parameters
        ----------
        calculator : callable
            ``**params -> dict of arrays``; must accept arrays (one value per grid point) for every parameter, as ``get_calculator``'s does.

        params : dict
            {parameter name: (lower limit, upper limit)}.

        order : int, dict, default=1
            Maximum derivative order, for all parameters or per parameter (names or wildcards).  0 or ``None``: the parameter is held at the centre
            of its limits.

        accuracy : int, dict, default=2
            Accuracy of the finite differences, a positive even integer, for all parameters or per parameter.
        """
        self.calculator = calculator
        self.params = {name: tuple(float(v) for v in limits) for name, limits in params.items()}
        names = list(self.params)
        self.order = {name: int(value or 0) for name, value in _expand(order, names).items()}
        self.accuracy = _expand(accuracy, names)
        for name in names:
            if not self.order[name]:
                continue
            value = self.accuracy[name]
            if value is None:
                raise ValueError('accuracy not specified for parameter {}'.format(name))
            value = int(value)
            if value < 1:
                raise ValueError('accuracy is {} < 1 for parameter {}'.format(value, name))
            if value % 2:
                raise ValueError('accuracy is {} for parameter {}, but it must be a positive EVEN integer'.format(value, name))
            self.accuracy[name] = value
        self.grid_center, self.grids = {}, []
        for name, limits in self.params.items():
            maxorder = self.order[name]
            if maxorder:
                coords = np.linspace(*limits, deriv_ncoeffs(maxorder, acc=self.accuracy[name]))
                c = len(coords) // 2
                reach = np.abs(np.arange(len(coords)) - c)
                tags = np.zeros(len(coords), dtype='i4')
                for o in range(maxorder, 0, -1):      # the least order whose stencil reaches the node; the centre belongs to order 0
                    tags[reach <= deriv_ncoeffs(o, acc=self.accuracy[name]) // 2] = o
                tags[c] = 0
                center = coords[c]
            else:
                center = np.mean(limits)
                coords, tags = np.array([center]), np.array([0], dtype='i4')
            self.grid_center[name] = center
            self.grids.append((coords, tags, maxorder))
        self.samples = None

    def points(self):
        """The grid points, as :class:`Samples` with ``attrs['cidx']`` (index of the centre, a 1-tuple as in the reference), ``'order'``, ``'accuracy'``."""
        X = np.array(_pruned_grid(self.grids), dtype='f8').reshape(-1, len(self.params))
        center = np.array([self.grid_center[name] for name in self.params])
        cidx = tuple(np.flatnonzero((X == center).all(axis=1)))
        assert len(cidx) == 1
        return Samples({name: X[:, i].copy() for i, name in enumerate(self.params)}, attrs={'cidx': cidx, 'order': dict(self.order), 'accuracy': dict(self.accuracy)})

    def run(self):
        """Evaluate the calculator once on the whole grid (arrays of ``npoints`` values) and once at the centre (scalars: the unbatched shapes).  An output
        is *varied* if its batched shape is ``(npoints,)`` + its shape at the centre, *fixed* (grids such as 'fourier.k') otherwise."""
        from .. import CalculatorComputationError
        samples = self.points()
        npoints = len(next(iter(samples.values())))
        center = self.calculator(**{name: float(value) for name, value in self.grid_center.items()})
        batch = self.calculator(**{name: np.array(value) for name, value in samples.items()})
        for key, value in batch.items():
            value = np.asarray(value)
            if key in center and value.shape == (npoints,) + np.shape(center[key]):
                bad = ~np.isfinite(value.reshape(npoints, -1)).all(axis=1)
                if bad.any():      # a Taylor fit cannot drop a node
                    i = int(np.flatnonzero(bad)[0])
                    raise CalculatorComputationError('{} is not finite at grid point {:d}: {}'.format(key, i, {name: float(v[i]) for name, v in samples.items()}))
                samples.varied[key] = value
            else:
                samples.fixed[key] = value
        self.samples = samples
        return samples
