"""
Taylor-expansion emulator under the reference's names (cosmoprimo/emulators/tools/taylor.py:180-254 ``TaylorEmulatorEngine``, with the ``Emulator``
front end of emulators/tools/base.py reduced to what the Taylor engine needs): finite differences on a grid of parameter points, then a polynomial.

Fit: the derivative of every term is linear in the samples, ``derivatives (T, M) = S (T, npoints) . Y (npoints, M)``.  ``S`` -- products of 1-D
finite-difference weights, times the 1 / alpha! of the term -- is built here on the host (T x npoints numbers); the product is one GEMM on the device
(``cp_taylor_fit``), and ``derivatives`` stay there.  Predict: ``out (B, M) = monomials (B, T) . derivatives`` for B parameter points at once
(``cp_taylor_predict``: the monomials are formed inside the kernel), where the reference evaluates one point per call.  Jacobian: the derivative of the
polynomial with respect to the parameters, ``(B ndim, M) = d monomials / d x_i . derivatives`` by the same kernel (``cp_taylor_jacobian``);
``Emulator.jacobian`` returns it by output key for either engine.

No x / y operations (log10, PCA, ...), no other engines.
"""
import itertools
import math

import numpy as np

from .samples import DiffSampler, deriv_ncoeffs


def fd_weights(order, acc, coords, idx):
    """Finite-difference weights of the derivative of given ``order`` and accuracy ``acc`` at node ``idx`` of the (non-uniform) 1-D grid ``coords``,
    and the offsets of the nodes they apply to: the solution of ``sum_j w_j (x_j - x_c)^i = order! delta_{i, order}`` by ``numpy.linalg.solve``, the
    system the reference solves (taylor.py:53-88), so that the weights are bit-identical to its weights on the same coordinates.  Central where the
    grid reaches far enough on both sides, one-sided at its ends."""
    order, acc = int(order), int(acc)
    if acc % 2 or acc <= 0:
        raise ValueError('Accuracy order acc must be positive EVEN integer')
    if order < 0:
        raise ValueError('Derive degree must be positive integer')
    ncoeffs = deriv_ncoeffs(order, acc=acc)
    nside = ncoeffs // 2
    ncoeffs += order % 2 == 0      # one-sided stencils of even derivatives take one node more
    if idx < nside:
        offsets = np.arange(ncoeffs)
    elif idx >= len(coords) - nside:
        offsets = np.arange(-ncoeffs + 1, 1)
    else:
        offsets = np.arange(-nside, nside + 1)
    matrix = np.array([[1] * len(offsets)] + [[(coords[idx + j] - coords[idx])**i for j in offsets] for i in range(1, len(offsets))], dtype='f8')
    rhs = np.zeros(len(offsets), dtype='f8')
    rhs[order] = math.factorial(order)
    return np.linalg.solve(matrix, rhs), offsets


def _stencil(X, index, orders, center):
    """Weights w (npoints,) with ``w @ Y`` the derivative of orders ``orders`` = [(axis, order, accuracy)] at ``center``, from the samples ``index`` of X:
    the last axis is differentiated first, each of its nodes standing for the derivative along the remaining axes on the samples that share it."""
    w = np.zeros(len(X), dtype='f8')
    if not orders:
        match = index[(X[index] == center).all(axis=1)]
        if not match.size:
            raise ValueError('Global center point not found')
        w[match[0]] = 1.
        return w
    axis, order, acc = orders[-1]
    coord = np.unique(X[index, axis])
    if coord.size < deriv_ncoeffs(order, acc=acc):
        raise ValueError('Grid is not large enough ({:d} < {:d}) to estimate {:d}-th order derivative'.format(coord.size, deriv_ncoeffs(order, acc=acc), order))
    c = np.flatnonzero(coord == center[axis])
    if not c.size:
        raise ValueError('Global center point not found')
    c = c[0]
    for weight, offset in zip(*fd_weights(order, acc, coord, c)):
        node = center.copy()
        node[axis] = coord[c + offset]
        w += weight * _stencil(X, index[X[index, axis] == node[axis]], orders[:-1], node)
    return w


def taylor_operator(X, cidx, order, accuracy):
    """``center`` (ndim,), ``powers`` (T, ndim) and ``S`` (T, npoints) of the expansion fitted to samples at ``X`` (npoints, ndim), a grid of
    :class:`DiffSampler` with centre ``X[cidx]`` and per-parameter maximum ``order`` and ``accuracy``: coefficient t of the expansion is ``S[t] @ Y``.

    Terms in the reference's order (taylor.py:221-236): the constant, then total order 1, 2, ...; within an order, multi-indices as their first
    appearance in ``itertools.product(range(ndim), repeat=order)``, which is the order of ``itertools.combinations_with_replacement``.  A term is skipped
    when its total order exceeds the maximum order of any parameter it involves.  The reference adds 1 / order! once per permutation of the indices;
    that is order! / alpha! times, i.e. the coefficient D^alpha f / alpha!."""
    X = np.asarray(X, dtype='f8')
    npoints, ndim = X.shape
    cidx = int(np.ravel(cidx)[0])
    order, accuracy = [int(o or 0) for o in order], list(accuracy)
    center = X[cidx].copy()
    unit = np.zeros(npoints, dtype='f8')
    unit[cidx] = 1.
    powers, S = [(0,) * ndim], [unit]
    index = np.arange(npoints)
    for total in range(1, max(order + [0]) + 1):
        for indices in itertools.combinations_with_replacement(range(ndim), total):
            power = tuple(np.bincount(indices, minlength=ndim).tolist())
            if total > min(o for p, o in zip(power, order) if p):
                continue
            alpha = 1
            for p in power:
                alpha *= math.factorial(p)
            powers.append(power)
            S.append(_stencil(X, index, [(i, p, accuracy[i]) for i, p in enumerate(power) if p > 0], center) / alpha)
    return center, np.array(powers, dtype='i4'), np.array(S, dtype='f8')


class TaylorEmulatorEngine(object):

    """Taylor expansion emulator engine.  State (the reference's names): ``center`` (ndim,), ``powers`` (T, ndim) int, ``derivatives`` (T, M),
    ``sampler_options``; ``derivatives`` is the host copy of the coefficients the device holds."""
    name = 'taylor'

    def __init__(self, order=3, accuracy=2, device=None):
        self.sampler_options = dict(order=order, accuracy=accuracy)
        self.device = device
        self._dev = None

    def get_default_samples(self, calculator, params, **kwargs):
        """Samples of a :class:`DiffSampler` with this engine's order and accuracy (``kwargs`` override them)."""
        sampler = DiffSampler(calculator, params, **{**self.sampler_options, **kwargs})
        return sampler.run()

    def fit(self, X, Y, attrs, params=None):
        """Fit to samples ``X`` (npoints, ndim), ``Y`` (npoints, M) of a :class:`DiffSampler`, ``attrs`` its ``cidx`` / ``order`` / ``accuracy`` (dictionaries
        by parameter name, in the order of ``params``, or sequences in the order of the columns of X)."""
        from ... import _device as dv, _lib
        if attrs.get('cidx', None) is None:
            raise ValueError('provide samples that are obtained with DiffSampler')
        order, accuracy = ([item[name] for name in params] if isinstance(item, dict) else list(item) for item in (attrs['order'], attrs['accuracy']))
        self.center, self.powers, S = taylor_operator(X, attrs['cidx'], order, accuracy)
        torch = dv.torch()
        device = dv.resolve_device(self.device)
        Yd = dv.to_device(np.ascontiguousarray(Y, dtype='f8'), device, cache=False)
        Sd = dv.to_device(S, device, cache=False)
        (T, npoints), M = S.shape, int(Yd.shape[1])
        if tuple(Yd.shape) != (npoints, M):
            raise ValueError('Y must be of shape (npoints, M) = ({:d}, M), got {}'.format(npoints, tuple(Yd.shape)))
        derivatives = torch.empty((T, M), dtype=torch.float64, device=device)
        _lib.check(_lib.load().cp_taylor_fit(Sd.data_ptr(), T, npoints, Yd.data_ptr(), M, derivatives.data_ptr(), device.index, dv.stream_of(device)))
        self.derivatives = dv.to_host(derivatives)
        self._set_device(device, derivatives)
        return self

    def _set_device(self, device, derivatives=None):
        from ... import _device as dv
        torch = dv.torch()
        if derivatives is None:
            derivatives = dv.to_device(np.ascontiguousarray(self.derivatives, dtype='f8'), device, cache=False)
        powers = np.ascontiguousarray(self.powers, dtype='i4')
        # derivatives_t: the (M, T) transpose, the right operand of the first GEMM of vjp (contiguous along the terms), made once
        self._dev = dict(device=device, derivatives=derivatives, derivatives_t=derivatives.t().contiguous(), center=dv.to_device(np.asarray(self.center, dtype='f8'), device, cache=False),
                         powers=dv.upload(powers, device, cache=False), max_power=int(powers.max(initial=0)), min_power=int(powers.min(initial=0)))
        assert self._dev['powers'].dtype == torch.int32

    def predict(self, X, columns=None):
        """Expansion at the points ``X`` (B, ndim), a device tensor (or host array, uploaded): device tensor (B, M).  Nothing is read back and the call
        does not wait for the device.  ``columns = (start, stop)``: those columns of it only, a (B, stop - start) tensor, bit for bit the same numbers
        (``cp_taylor_predict_columns``: no other column of the derivatives is read, nothing else is allocated)."""
        from ... import _device as dv, _lib
        if self._dev is None:
            self._set_device(dv.resolve_device(self.device, X))
        d = self._dev
        torch = dv.torch()
        X = dv.to_device(X, d['device'], cache=False)
        T, ndim = (int(n) for n in np.shape(self.powers))
        if X.ndim != 2 or int(X.shape[1]) != ndim:
            raise ValueError('X must be of shape (B, {:d}), got {}'.format(ndim, tuple(X.shape)))
        if d['min_power'] < 0:
            raise ValueError('powers must be non-negative')
        B, M = int(X.shape[0]), int(d['derivatives'].shape[1])
        if columns is not None:
            start, stop = (int(c) for c in columns)
            out = torch.empty((B, max(stop - start, 0)), dtype=torch.float64, device=d['device'])
            _lib.check(_lib.load().cp_taylor_predict_columns(X.data_ptr(), B, d['center'].data_ptr(), d['powers'].data_ptr(), ndim, T, d['max_power'],
                                                             d['derivatives'].data_ptr(), M, start, stop - start, out.data_ptr(), stop - start, d['device'].index,
                                                             dv.stream_of(d['device'])))
            return out
        out = torch.empty((B, M), dtype=torch.float64, device=d['device'])
        _lib.check(_lib.load().cp_taylor_predict(X.data_ptr(), B, d['center'].data_ptr(), d['powers'].data_ptr(), ndim, T, d['max_power'], d['derivatives'].data_ptr(),
                                                 M, out.data_ptr(), d['device'].index, dv.stream_of(d['device'])))
        return out

    def jacobian(self, X, columns=None, return_value=False):
        """Derivative of :meth:`predict` with respect to the parameters at the points ``X`` (B, ndim): device tensor ``J`` (B, ndim, M),
        ``J[b, i, :] = sum_t derivatives[t, :] p_ti (x_i - c_i)^(p_ti - 1) prod_{j != i} (x_j - c_j)^p_tj``, one launch (``cp_taylor_jacobian``: the
        derivatives of the monomials are formed inside the kernel).  ``columns = (start, stop)``: those output columns only, (B, ndim, stop - start), bit
        for bit the same numbers.  ``return_value=True``: ``(predict(X, columns=columns), J)``, one more launch.  Nothing is read back and the call does
        not wait for the device."""
        from ... import _device as dv, _lib
        if self._dev is None:
            self._set_device(dv.resolve_device(self.device, X))
        d = self._dev
        torch = dv.torch()
        X = dv.to_device(X, d['device'], cache=False)
        T, ndim = (int(n) for n in np.shape(self.powers))
        if X.ndim != 2 or int(X.shape[1]) != ndim:
            raise ValueError('X must be of shape (B, {:d}), got {}'.format(ndim, tuple(X.shape)))
        if d['min_power'] < 0:
            raise ValueError('powers must be non-negative')
        B, M = int(X.shape[0]), int(d['derivatives'].shape[1])
        start, stop = (int(c) for c in columns) if columns is not None else (0, M)
        ncols = max(stop - start, 0)
        jac = torch.empty((B, ndim, ncols), dtype=torch.float64, device=d['device'])
        _lib.check(_lib.load().cp_taylor_jacobian(X.data_ptr(), B, d['center'].data_ptr(), d['powers'].data_ptr(), ndim, T, d['max_power'], d['derivatives'].data_ptr(),
                                                  M, start, stop - start, jac.data_ptr(), ncols, d['device'].index, dv.stream_of(d['device'])))
        return (self.predict(X, columns=columns), jac) if return_value else jac

    def vjp(self, X, cotangent, columns=None, return_value=False):
        """Vector-Jacobian product of :meth:`predict` at the points ``X`` (B, ndim): device tensor ``G`` (B, ndim),
        ``G[b, i] = sum_c cotangent[b, c] d predict(X)[b, c] / d X[b, i]`` (``cp_taylor_vjp``: the cotangent times the transposed derivatives on the matrix
        cores, (B, T), then its contraction with the derivatives of the monomials; no (B, ndim, M) array anywhere).  ``cotangent``: (B, M) device tensor
        (or host array, uploaded), rows of any stride.  ``columns = (start, stop)``: the sum over those output columns only, ``cotangent``
        (B, stop - start).  ``return_value=True``: ``(predict(X, columns=columns), G)``, one more launch.  Nothing is read back and the call does not wait
        for the device."""
        from ... import _device as dv, _lib
        if self._dev is None:
            self._set_device(dv.resolve_device(self.device, X))
        d = self._dev
        torch = dv.torch()
        X = dv.to_device(X, d['device'], cache=False)
        T, ndim = (int(n) for n in np.shape(self.powers))
        if X.ndim != 2 or int(X.shape[1]) != ndim:
            raise ValueError('X must be of shape (B, {:d}), got {}'.format(ndim, tuple(X.shape)))
        if d['min_power'] < 0:
            raise ValueError('powers must be non-negative')
        B, M = int(X.shape[0]), int(d['derivatives'].shape[1])
        start, stop = (int(c) for c in columns) if columns is not None else (0, M)
        ncols = max(stop - start, 0)
        cotangent = dv.to_device(cotangent, d['device'], cache=False)
        if tuple(cotangent.shape) != (B, ncols):
            raise ValueError('cotangent must be of shape ({:d}, {:d}), got {}'.format(B, ncols, tuple(cotangent.shape)))
        if cotangent.dtype != torch.float64 or (ncols > 1 and cotangent.stride(1) != 1) or (B > 1 and cotangent.stride(0) < ncols):
            cotangent = cotangent.to(torch.float64).contiguous()
        ldc = int(cotangent.stride(0)) if B > 1 else ncols
        lib = _lib.load()
        need = int(lib.cp_taylor_vjp_workspace_doubles(B, T))
        if need < 0:
            _lib.check(-need)
        work = torch.empty((need,), dtype=torch.float64, device=d['device'])
        grad = torch.empty((B, ndim), dtype=torch.float64, device=d['device'])
        _lib.check(lib.cp_taylor_vjp(X.data_ptr(), B, d['center'].data_ptr(), d['powers'].data_ptr(), ndim, T, d['max_power'], d['derivatives_t'].data_ptr(), M, start,
                                     stop - start, cotangent.data_ptr(), ldc, grad.data_ptr(), work.data_ptr(), need, d['device'].index, dv.stream_of(d['device'])))
        return (self.predict(X, columns=columns), grad) if return_value else grad

    def __getstate__(self):
        state = {'sampler_options': self.sampler_options}
        for name in ['center', 'derivatives', 'powers']:
            if hasattr(self, name):
                state[name] = getattr(self, name)
        return state

    def __setstate__(self, state):
        self.sampler_options = dict(state.get('sampler_options', {}))
        self.device, self._dev = None, None
        for name in ['center', 'derivatives', 'powers']:
            if name in state:
                setattr(self, name, np.asarray(state[name]))

    @classmethod
    def from_state(cls, state, device=None):
        new = cls.__new__(cls)
        new.__setstate__(state)
        new.device = device
        return new


def _requested(key, keys):
    """Is ``key`` asked for by ``keys``, a section prefix ('fourier' takes 'fourier.k', never 'fourierx.k'; 'fourier.k' takes itself, never 'fourier.kz')
    or a list of such?"""
    return any(key == name or key.startswith(name + '.') for name in ([keys] if isinstance(keys, str) else keys))


def _key_columns(varied_keys, varied_shapes):
    """(key, shape, start, stop) of every varied key in the concatenation the engine is fitted on."""
    toret, start = [], 0
    for key, shape in zip(varied_keys, varied_shapes):
        size = int(np.prod(shape, dtype='i8'))
        toret.append((key, tuple(shape), start, start + size))
        start += size
    return toret


def column_runs(varied_keys, varied_shapes, keys):
    """The maximal contiguous runs ``[(start, stop), ...]`` of columns of the (B, M) prediction that hold the varied outputs ``keys`` asks for: a list of
    output names or section prefixes, or one such string ('background': every 'background.*').  A name matches itself and what it prefixes at a dot
    ('fourier.k' does not take 'fourier.kz').  A name that matches no varied output raises ``KeyError``; an empty list gives no run.  Outputs without
    columns (size 0) join no run.  The keys of one section are adjacent in the calculator's order, so a section is normally one run."""
    names = [keys] if isinstance(keys, str) else list(keys)
    for name in names:
        if not any(_requested(key, [name]) for key in varied_keys):
            raise KeyError('no varied output {}'.format(name))
    runs = []
    for key, shape, start, stop in _key_columns(varied_keys, varied_shapes):
        if stop == start or not _requested(key, names):
            continue
        if runs and runs[-1][1] == start:
            runs[-1] = (runs[-1][0], stop)
        else:
            runs.append((start, stop))
    return runs


class Emulator(object):

    """Emulate a calculator ``**params -> dict of arrays``: sample it (:meth:`set_samples`), :meth:`fit`, then :meth:`predict` at B parameter points at once.

    .. code-block:: python

        calculator = get_calculator(Cosmology(engine='eisenstein_hu'))
        emulator = Emulator(calculator, params={'Omega_m': (0.25, 0.35), 'h': (0.6, 0.8)}, engine='taylor', order=3)
        emulator.set_samples()       # the whole finite-difference grid in one call of the calculator
        emulator.fit()
        emulator.predict({'Omega_m': np.linspace(0.28, 0.32, 10000), 'h': 0.7})   # {'fourier.pk.delta_m.delta_m': (10000, 422, 30) array, ...}
    """

    def __init__(self, calculator, params=None, engine='taylor', device=None, **engine_options):
        if isinstance(engine, str):
            if engine == 'mlp':
                from .mlp import MLPEmulatorEngine
                engine = MLPEmulatorEngine(device=device, **engine_options)
            elif engine == 'taylor':
                engine = TaylorEmulatorEngine(device=device, **engine_options)
            else:
                raise NotImplementedError('engine {} (only the Taylor and MLP engines are built)'.format(engine))
        self.calculator = calculator
        self.params = {name: tuple(limits) for name, limits in (params or {}).items()}
        self.engine = engine
        self.samples = None
        self.varied_keys, self.varied_shapes, self.fixed = [], [], {}

    def set_samples(self, samples=None, **kwargs):
        """Set the samples to fit: those given, else the engine's default (Taylor: :class:`DiffSampler` run on the calculator, ``kwargs`` override order /
        accuracy; MLP: :class:`QMCSampler`, ``kwargs`` its ``engine``, ``niterations``, ``batch_size``)."""
        self.samples = samples if samples is not None else self.engine.get_default_samples(self.calculator, self.params, **kwargs)
        return self.samples

    def fit(self, **kwargs):
        """Concatenate the flattened varied outputs into Y (npoints, M), upload it once and fit the engine on the device.  ``kwargs``: training options of
        the engine (:meth:`MLPEmulatorEngine.fit`; the Taylor engine takes none)."""
        if self.samples is None:
            self.set_samples()
        samples = self.samples
        self.varied_keys = list(samples.varied)
        if not self.varied_keys:
            raise ValueError('the calculator returns nothing that varies with the parameters')
        self.varied_shapes = [tuple(samples.varied[key].shape[1:]) for key in self.varied_keys]
        self.fixed = dict(samples.fixed)
        Y = np.concatenate([np.asarray(samples.varied[key], dtype='f8').reshape(len(samples.varied[key]), -1) for key in self.varied_keys], axis=1)
        self.engine.fit(samples.matrix(), Y, samples.attrs, params=list(self.params), **kwargs)
        return self

    def _points(self, params):
        """(X (B, ndim) in the order of ``self.params``, a host array unless a parameter is a device tensor; B; whether every parameter is a scalar)."""
        from ... import _device as dv
        missing = [name for name in self.params if name not in params]
        if missing:
            raise ValueError('missing parameters {}'.format(missing))
        values = [params[name] for name in self.params]
        dev = self.engine._dev['device'] if self.engine._dev is not None else dv.resolve_device(self.engine.device, *values)
        torch = dv.torch()
        sizes = {int(np.prod(np.shape(v))) for v in values if np.ndim(v) > 0}
        if len(sizes) > 1:
            raise ValueError('parameter arrays must share one length, got {}'.format(sorted(sizes)))
        scalar = not sizes
        B = 1 if scalar else sizes.pop()
        if all(not dv.is_torch(v) for v in values):
            X = np.empty((B, len(values)), dtype='f8')
            for i, v in enumerate(values):
                X[:, i] = np.ravel(v)
        else:
            X = torch.stack([dv.to_device(v, dev, cache=False).reshape(-1).expand(B) for v in values], dim=1)
        return X, B, scalar

    def predict(self, params, device=False, keys=None):
        """Outputs at ``params``, a dictionary of scalars or arrays of B values (host arrays or device tensors): the calculator's keys, varied ones of shape
        ``(B,) + shape`` (no leading axis if every parameter is a scalar), fixed ones as they are.  Host arrays by default; ``device=True``: torch tensors,
        views into one (B, M) buffer, and no synchronisation with the device.

        ``keys``: a list of output names, or a section prefix such as 'background' (every 'background.*' key): these outputs only.  Their columns are
        planned by :func:`column_runs`; each maximal contiguous run of them is one launch of the engine on that range (B, ncols) -- the keys of a section
        are adjacent, so normally one -- and no other column is computed or stored.  The varied keys asked for and the fixed ones under the prefix (or
        among the names) are returned."""
        from ... import _device as dv
        X, B, scalar = self._points(params)
        if keys is not None:
            names = [keys] if isinstance(keys, str) else list(keys)
            unknown = [name for name in names if not any(_requested(key, [name]) for key in list(self.varied_keys) + list(self.fixed))]
            if unknown:
                raise KeyError('no output {}'.format(unknown))
            # names that match fixed outputs only need no column
            runs = column_runs(self.varied_keys, self.varied_shapes, [name for name in names if any(_requested(key, [name]) for key in self.varied_keys)])
            toret = {}
            for start, stop in runs:
                out = self.engine.predict(X, columns=(start, stop))
                if not device:
                    out = dv.to_host(out)
                for key, shape, lo, hi in _key_columns(self.varied_keys, self.varied_shapes):
                    if start <= lo and hi <= stop and _requested(key, keys):
                        value = out[:, lo - start:hi - start].reshape((B,) + shape)
                        toret[key] = value[0] if scalar else value
            toret.update({key: value for key, value in self.fixed.items() if _requested(key, keys)})
            return toret
        out = self.engine.predict(X)
        if not device:
            out = dv.to_host(out)
        toret, start = {}, 0
        for key, shape in zip(self.varied_keys, self.varied_shapes):
            size = int(np.prod(shape, dtype='i8'))
            value = out[:, start:start + size].reshape((B,) + shape)
            toret[key] = value[0] if scalar else value
            start += size
        toret.update(self.fixed)
        return toret

    def jacobian(self, params, device=False, keys=None, return_value=False):
        """Derivatives of the varied outputs with respect to the parameters at ``params`` (as in :meth:`predict`: scalars or arrays of B values, host or
        device), computed analytically on the device (:meth:`MLPEmulatorEngine.jacobian`, :meth:`TaylorEmulatorEngine.jacobian`):
        ``{key: array (B, ndim) + shape}``, the ``ndim`` axis in the order of ``Emulator.params``, without the leading ``B`` axis if every parameter is a
        scalar.  Fixed outputs are not returned: their derivative is identically zero.  Host arrays by default; ``device=True``: torch tensors, views
        into the (B, ndim, ncols) buffer(s), and no synchronisation with the device.

        ``keys``: as in :meth:`predict` -- the columns are planned by :func:`column_runs`, one call of the engine per maximal contiguous run, and no other
        column is computed.  ``return_value=True``: ``(values, jacobian)``, ``values`` what ``predict(params, device=device, keys=keys)`` returns."""
        from ... import _device as dv
        X, B, scalar = self._points(params)
        ndim = len(self.params)
        if keys is not None:
            names = [keys] if isinstance(keys, str) else list(keys)
            unknown = [name for name in names if not any(_requested(key, [name]) for key in list(self.varied_keys) + list(self.fixed))]
            if unknown:
                raise KeyError('no output {}'.format(unknown))
            runs = column_runs(self.varied_keys, self.varied_shapes, [name for name in names if any(_requested(key, [name]) for key in self.varied_keys)])
        else:
            runs = [(0, sum(int(np.prod(shape, dtype='i8')) for shape in self.varied_shapes))]
        values, toret = {}, {}
        for start, stop in runs:
            out = self.engine.jacobian(X, columns=None if keys is None else (start, stop), return_value=return_value)
            value, jac = out if return_value else (None, out)
            if not device:
                value, jac = (dv.to_host(a) if a is not None else None for a in (value, jac))
            for key, shape, lo, hi in _key_columns(self.varied_keys, self.varied_shapes):
                if not (start <= lo and hi <= stop) or (keys is not None and not _requested(key, keys)):
                    continue
                block = jac[:, :, lo - start:hi - start].reshape((B, ndim) + shape)
                toret[key] = block[0] if scalar else block
                if return_value:
                    block = value[:, lo - start:hi - start].reshape((B,) + shape)
                    values[key] = block[0] if scalar else block
        if not return_value:
            return toret
        values.update({key: value for key, value in self.fixed.items() if keys is None or _requested(key, keys)})
        return values, toret

    def vjp(self, params, cotangents, device=False, return_value=False):
        """Vector-Jacobian product: the gradient with respect to the parameters of a scalar function of the outputs whose derivative with respect to
        them is ``cotangents``, for every point of a batch -- what ``jax.vjp`` / ``jax.grad`` of the reference's ``predict`` give, and what a
        gradient-based sampler wants of a log-likelihood.  ``params`` as in :meth:`predict`.  ``cotangents``: ``{varied key: array or tensor}``, each
        broadcastable to ``(B,) + shape`` of that output (``shape`` alone with scalar parameters).  A fixed key is accepted and contributes nothing (its
        derivative is zero), an unknown key raises ``KeyError``, an empty dictionary gives zeros.

        Returns ``{parameter name: (B,) array}`` in the order of ``Emulator.params``, ``sum over keys and entries of cotangent * d output / d parameter``
        (scalars if every parameter is a scalar).  Computed by reverse mode on the device (:meth:`MLPEmulatorEngine.vjp`,
        :meth:`TaylorEmulatorEngine.vjp`) without forming the Jacobian: the columns are planned by :func:`column_runs` over the cotangents' varied keys,
        one call of the engine per maximal contiguous run on that range only, the runs' results added in run order.  Host arrays by default;
        ``device=True``: the views ``G[:, i]`` of one (B, ndim) tensor, and no synchronisation with the device.  ``return_value=True``:
        ``(values, gradients)``, ``values`` what ``predict(params, device=device, keys=list(cotangents))`` returns."""
        from ... import _device as dv
        X, B, scalar = self._points(params)
        torch = dv.torch()
        names = list(cotangents)
        unknown = [name for name in names if name not in self.varied_keys and name not in self.fixed]
        if unknown:
            raise KeyError('no output {}'.format(unknown))
        runs = column_runs(self.varied_keys, self.varied_shapes, [name for name in names if name in self.varied_keys])
        dev = self.engine._dev['device'] if self.engine._dev is not None else dv.resolve_device(self.engine.device, X, *cotangents.values())
        total, values = None, {}
        for start, stop in runs:
            blocks = []
            for key, shape, lo, hi in _key_columns(self.varied_keys, self.varied_shapes):
                if start <= lo and hi <= stop and hi > lo:      # (a run holds requested keys only)
                    cot = dv.to_device(cotangents[key], dev, cache=False).to(torch.float64)
                    blocks.append(torch.broadcast_to(cot, (B,) + shape).reshape(B, hi - lo))
            out = self.engine.vjp(X, blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1), columns=(start, stop), return_value=return_value)
            value, grad = out if return_value else (None, out)
            total = grad if total is None else total + grad
            if return_value:
                if not device:
                    value = dv.to_host(value)
                for key, shape, lo, hi in _key_columns(self.varied_keys, self.varied_shapes):
                    if start <= lo and hi <= stop and key in cotangents:
                        block = value[:, lo - start:hi - start].reshape((B,) + shape)
                        values[key] = block[0] if scalar else block
        if total is None:
            total = torch.zeros((B, len(self.params)), dtype=torch.float64, device=dev)
        if not device:
            total = dv.to_host(total)
        grads = {name: (total[0, i] if scalar else total[:, i]) for i, name in enumerate(self.params)}
        if not return_value:
            return grads
        for key in self.varied_keys:      # empty outputs hold no column and join no run
            if key in cotangents and key not in values:
                values[key] = self.predict(params, device=device, keys=[key])[key]
        values = {key: values[key] for key in self.varied_keys if key in values}      # predict's order: the calculator's, then the fixed outputs
        values.update({key: value for key, value in self.fixed.items() if key in cotangents})
        return values, grads

    def to_calculator(self, device=False):
        """Callable ``**params -> dict`` with the contract of ``get_calculator``'s."""
        def calculator(**params):
            return self.predict(params, device=device)

        return calculator

    def __getstate__(self):
        return {'name': self.engine.name, 'engine': self.engine.__getstate__(), 'params': dict(self.params), 'varied_keys': list(self.varied_keys), 'varied_shapes': [tuple(s) for s in self.varied_shapes],
                'fixed': dict(self.fixed)}

    def save(self, fn):
        """Save the state (the engine's ``name`` and state -- Taylor: ``center``, ``powers``, ``derivatives``, ``sampler_options`` -- key names, shapes, fixed
        values) as one ``.npy`` dictionary."""
        np.save(fn, self.__getstate__(), allow_pickle=True)

    @classmethod
    def load(cls, fn, device=None):
        state = np.load(fn, allow_pickle=True)[()]
        new = cls.__new__(cls)
        new.calculator, new.samples = None, None
        new.params = dict(state['params'])
        name = state.get('name', 'taylor')      # a file without a name is a Taylor file
        if name == 'mlp':
            from .mlp import MLPEmulatorEngine
            new.engine = MLPEmulatorEngine.from_state(state['engine'], device=device)
        elif name == 'taylor':
            new.engine = TaylorEmulatorEngine.from_state(state['engine'], device=device)
        else:
            raise NotImplementedError('engine {} (only the Taylor and MLP engines are built)'.format(name))
        new.varied_keys, new.varied_shapes, new.fixed = list(state['varied_keys']), [tuple(s) for s in state['varied_shapes']], dict(state['fixed'])
        return new
