"""
Taylor-expansion emulator engine under the reference's name (cosmoprimo/emulators/tools/taylor.py:180-254 ``TaylorEmulatorEngine``) and its fitting helpers:
finite differences on a grid of parameter points, then a polynomial.  The ``Emulator`` front end that serves this engine and the MLP one is in base.py.

Fit: the derivative of every term is linear in the samples, ``derivatives (T, M) = S (T, npoints) . Y (npoints, M)``.  ``S`` -- products of 1-D
finite-difference weights, times the 1 / alpha! of the term -- is built here on the host (T x npoints numbers); the product is one GEMM on the device
(``cp_taylor_fit``), and ``derivatives`` stay there.  Predict: ``out (B, M) = monomials (B, T) . derivatives`` for B parameter points at once
(``cp_taylor_predict_columns``: the monomials are formed inside the kernel), where the reference evaluates one point per call.  Jacobian: the derivative
of the polynomial with respect to the parameters, ``(B ndim, M) = d monomials / d x_i . derivatives`` by the same kernel (``cp_taylor_jacobian``).  Vjp: its
product with a cotangent, without forming it (``cp_taylor_vjp``).  Jvp: its product with tangents, without forming it (``cp_taylor_jvp``).  Jvp2: second
directional derivatives along pairs of tangents, the second derivatives of the monomials formed inside the kernel (``cp_taylor_jvp2``).  They open
with one prologue (``_enter``: device state, upload and check of ``X``, the nine leading C arguments).

No x / y operations (log10, PCA, ...).
"""
import itertools
import math

import numpy as np

from ... import _device as dv, _lib
from .base import _columns, _cotangent, _empty, _gauss_newton, _jacobian_out, _tangent
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
        torch = dv.torch()
        if derivatives is None:
            derivatives = dv.to_device(np.ascontiguousarray(self.derivatives, dtype='f8'), device, cache=False)
        powers = np.ascontiguousarray(self.powers, dtype='i4')
        # derivatives_t: the (M, T) transpose, the right operand of the first GEMM of vjp (contiguous along the terms), made once
        self._dev = dict(device=device, torch=torch, derivatives=derivatives, derivatives_t=derivatives.t().contiguous(), center=dv.to_device(np.asarray(self.center, dtype='f8'), device, cache=False),
                         powers=dv.upload(powers, device, cache=False), max_power=int(powers.max(initial=0)), min_power=int(powers.min(initial=0)),
                         sizes=tuple(int(n) for n in powers.shape) + (int(derivatives.shape[1]),))      # (T, ndim, M)
        assert self._dev['powers'].dtype == torch.int32

    def _enter(self, X, derivatives='derivatives'):
        """The opening of :meth:`predict`, :meth:`jacobian` and :meth:`vjp`: the device state (set at the first call), ``X`` (B, ndim) on its device, the sizes
        (B, ndim, T, M), the nine leading arguments of the C entry points (the points, the polynomial, and the derivatives
        under the name ``derivatives``: (T, M), or for ``vjp`` its transpose)
        and their last two (device, stream)."""
        if self._dev is None:
            self._set_device(dv.resolve_device(self.device, X))
        d = self._dev
        X = dv.to_device(X, d['device'], cache=False)
        T, ndim, M = d['sizes']
        if X.ndim != 2 or int(X.shape[1]) != ndim:
            raise ValueError('X must be of shape (B, {:d}), got {}'.format(ndim, tuple(X.shape)))
        if d['min_power'] < 0:
            raise ValueError('powers must be non-negative')
        B = int(X.shape[0])
        head = (X.data_ptr(), B, d['center'].data_ptr(), d['powers'].data_ptr(), ndim, T, d['max_power'], d[derivatives].data_ptr(), M)
        return d, X, (B, ndim, T, M), head, (d['device'].index, dv.stream_of(d['device']))

    def predict(self, X, columns=None):
        """Expansion at the points ``X`` (B, ndim), a device tensor (or host array, uploaded): device tensor (B, M).  Nothing is read back and the call
        does not wait for the device.  ``columns = (start, stop)``: those columns of it only, a (B, stop - start) tensor, bit for bit the same numbers
        (``cp_taylor_predict_columns``: no other column of the derivatives is read, nothing else is allocated; every column is the range (0, M) of the
        same call, so a refusal names that entry point; ``cp_taylor_predict`` itself is there for C callers)."""
        d, X, (B, ndim, T, M), head, where = self._enter(X)
        start, ncols = _columns(columns, M)
        out = _empty(d, B, max(ncols, 0))
        _lib.check(_lib.load().cp_taylor_predict_columns(*head, start, ncols, out.data_ptr(), ncols, *where))
        return out

    def jacobian(self, X, columns=None, return_value=False, out=None):
        """Derivative of :meth:`predict` with respect to the parameters at the points ``X`` (B, ndim): device tensor ``J`` (B, ndim, M),
        ``J[b, i, :] = sum_t derivatives[t, :] p_ti (x_i - c_i)^(p_ti - 1) prod_{j != i} (x_j - c_j)^p_tj``, one launch (``cp_taylor_jacobian``: the
        derivatives of the monomials are formed inside the kernel).  ``columns = (start, stop)``: those output columns only, (B, ndim, stop - start), bit
        for bit the same numbers.  ``return_value=True``: ``(predict(X, columns=columns), J)``, one more launch.  Nothing is read back and the call does
        not wait for the device.  ``out = (value or None, J)``: device tensors to write instead of new ones, views into wider buffers with rows of any
        stride (:func:`base._jacobian_out`); the value is written where ``return_value`` asks for it."""
        d, X, (B, ndim, T, M), head, where = self._enter(X)
        start, ncols = _columns(columns, M)
        value, ldv, jac, ldj = _jacobian_out(d, out, B, ndim, max(ncols, 0), return_value and out is not None)
        _lib.check(_lib.load().cp_taylor_jacobian(*head, start, ncols, jac.data_ptr(), ldj, *where))
        if out is None:
            return (self.predict(X, columns=columns), jac) if return_value else jac
        if return_value:
            _lib.check(_lib.load().cp_taylor_predict_columns(*head, start, ncols, value.data_ptr(), ldv, *where))
        return (value, jac) if return_value else jac

    def vjp(self, X, cotangent, columns=None, return_value=False):
        """Vector-Jacobian product of :meth:`predict` at the points ``X`` (B, ndim): device tensor ``G`` (B, ndim),
        ``G[b, i] = sum_c cotangent[b, c] d predict(X)[b, c] / d X[b, i]`` (``cp_taylor_vjp``: the cotangent times the transposed derivatives on the matrix
        cores, (B, T), then its contraction with the derivatives of the monomials; no (B, ndim, M) array anywhere).  ``cotangent``: (B, M) device tensor
        (or host array, uploaded), rows of any stride.  ``columns = (start, stop)``: the sum over those output columns only, ``cotangent``
        (B, stop - start).  ``return_value=True``: ``(predict(X, columns=columns), G)``, one more launch.  Nothing is read back and the call does not wait
        for the device."""
        d, X, (B, ndim, T, M), head, where = self._enter(X, derivatives='derivatives_t')
        start, ncols = _columns(columns, M)
        cotangent, ldc = _cotangent(cotangent, B, max(ncols, 0), d['device'])
        lib = _lib.load()
        need = int(lib.cp_taylor_vjp_workspace_doubles(B, T))
        if need < 0:
            _lib.check(-need)
        work, grad = _empty(d, need), _empty(d, B, ndim)
        _lib.check(lib.cp_taylor_vjp(*head, start, ncols, cotangent.data_ptr(), ldc, grad.data_ptr(), work.data_ptr(), need, *where))
        return (self.predict(X, columns=columns), grad) if return_value else grad

    def vjp2(self, X, cotangent, columns=None, return_value=False):
        """Second derivatives of :meth:`predict` contracted with a cotangent at the points ``X`` (B, ndim): device tensor ``C`` (B, ndim, ndim),
        ``C[b, i, j] = sum_c cotangent[b, c] d^2 predict(X)[b, c] / d X[b, i] d X[b, j]``, symmetric bit for bit (``cp_taylor_vjp2``: the first GEMM of
        :meth:`vjp`, (B, T), then its contraction with the second derivatives of the monomials, a row per (point, pair i <= j); no
        (B, ndim (ndim + 1) / 2, M) array anywhere).  ``cotangent``, ``columns`` and ``return_value`` as in :meth:`vjp`.  Nothing is read back and the
        call does not wait for the device."""
        d, X, (B, ndim, T, M), head, where = self._enter(X, derivatives='derivatives_t')
        start, ncols = _columns(columns, M)
        cotangent, ldc = _cotangent(cotangent, B, max(ncols, 0), d['device'])
        lib = _lib.load()
        need = int(lib.cp_taylor_vjp2_workspace_doubles(B, T))
        if need < 0:
            _lib.check(-need)
        work, hess = _empty(d, need), _empty(d, B, ndim, ndim)
        _lib.check(lib.cp_taylor_vjp2(*head, start, ncols, cotangent.data_ptr(), ldc, hess.data_ptr(), work.data_ptr(), need, *where))
        return (self.predict(X, columns=columns), hess) if return_value else hess

    def jvp(self, X, tangents, columns=None, return_value=False):
        """Jacobian-vector product of :meth:`predict` at the points ``X`` (B, ndim) along ``tangents`` (B, ndim) -- device tensor (B, M),
        ``out[b, c] = sum_i tangents[b, i] d predict(X)[b, c] / d X[b, i]`` -- or (B, K, ndim), K directions per point -- (B, K, M) --, a device tensor or
        host array (uploaded); one launch (``cp_taylor_jvp``: the derivatives of the monomials contracted with the tangent inside the kernel, a parameter
        that a term does not hold skipped; no (B, ndim, M) array anywhere, and ndim identity tangents give the bits of :meth:`jacobian`).
        ``columns = (start, stop)``: those output columns only, bit for bit the same numbers.  ``return_value=True``:
        ``(predict(X, columns=columns), out)``, one more launch.  Nothing is read back and the call does not wait for the device."""
        d, X, (B, ndim, T, M), head, where = self._enter(X)
        start, ncols = _columns(columns, M)
        width = max(ncols, 0)
        tangents, K, single = _tangent(tangents, B, ndim, d['device'])
        out = _empty(d, B, K, width)
        _lib.check(_lib.load().cp_taylor_jvp(*head, start, ncols, tangents.data_ptr(), K, out.data_ptr(), width, *where))
        out = out[:, 0] if single else out
        return (self.predict(X, columns=columns), out) if return_value else out

    def jvp2(self, X, tangents, tangents2=None, columns=None, return_value=False, return_first=False):
        """Second directional derivatives of :meth:`predict` at the points ``X`` (B, ndim) along the pairs of directions ``tangents``, ``tangents2``, both
        (B, ndim) -- device tensor (B, M), ``out[b, c] = sum_ij tangents[b, i] tangents2[b, j] d^2 predict(X)[b, c] / d X[b, i] d X[b, j]`` -- or
        (B, K, ndim), K pairs per point -- (B, K, M) --, device tensors or host arrays (uploaded); ``tangents2=None``: the second directional derivative
        along ``tangents``.  One launch (``cp_taylor_jvp2``: the second derivatives of the monomials contracted with the pair inside the kernel, a
        parameter that a term does not hold skipped; no (B, ndim, ndim, M) array anywhere; exchanging the two sets gives the same bits).
        ``columns = (start, stop)``: those output columns only, bit for bit the same numbers.  ``return_value=True``: ``predict(X, columns=columns)`` is
        prepended, one more launch; ``return_first=True``: what :meth:`jvp` gives along ``tangents`` (and along ``tangents2``, where given) is inserted
        before the result, a call of :meth:`jvp` each.  Nothing is read back and the call does not wait for the device."""
        d, X, (B, ndim, T, M), head, where = self._enter(X)
        start, ncols = _columns(columns, M)
        width = max(ncols, 0)
        sets = [tangents] if tangents2 is None else [tangents, tangents2]
        tangents, K, single = _tangent(tangents, B, ndim, d['device'])
        mixed = tangents2 is not None
        if mixed:
            tangents2, K2, single2 = _tangent(tangents2, B, ndim, d['device'])
            if (K2, single2) != (K, single):
                raise ValueError('tangents and tangents2 must share one shape')
        out = _empty(d, B, K, width)
        _lib.check(_lib.load().cp_taylor_jvp2(*head, start, ncols, tangents.data_ptr(), tangents2.data_ptr() if mixed else None, K, out.data_ptr(), width, *where))
        toret = ([self.predict(X, columns=columns)] if return_value else []) + ([self.jvp(X, t, columns=columns) for t in sets] if return_first else [])
        toret.append(out[:, 0] if single else out)
        return tuple(toret) if len(toret) > 1 else toret[0]

    def gauss_newton(self, X, weights, data=None, columns=None, return_value=False):
        """Fisher matrices and Gauss-Newton normal equations of :meth:`predict` at the points ``X`` (B, ndim), with ``J`` the Jacobian of :meth:`jacobian`:
        device tensors ``fisher`` (B, ndim, ndim), ``fisher[b, i, j] = sum_c weights[b, c] J[b, i, c] J[b, j, c]`` (symmetric bit for bit), and with
        ``data`` ``(fisher, grad, chi2)``, ``grad[b, i] = sum_c weights[b, c] (data[b, c] - predict(X)[b, c]) J[b, i, c]`` (B, ndim) and
        ``chi2[b] = sum_c weights[b, c] (data[b, c] - predict(X)[b, c])^2`` (B,) (``cp_taylor_gauss_newton``: the tile of ``J`` the jacobian GEMM would
        store is contracted over its columns in registers and LDS; no (B, ndim, M) array anywhere).  ``weights``, ``data``: (M,) shared by all points or
        (B, M), device tensors or host arrays (uploaded), rows of any stride.  A weight of exactly 0 drops its column, whatever it holds.
        ``columns = (start, stop)``: the sums over those output columns only, ``weights`` and ``data`` (stop - start,) or (B, stop - start).
        ``return_value=True``: ``predict(X, columns=columns)`` is prepended.  Nothing is read back and the call does not wait for the device."""
        d, X, (B, ndim, T, M), head, where = self._enter(X)
        start, ncols = _columns(columns, M)
        lib = _lib.load()
        need = int(lib.cp_taylor_gauss_newton_workspace_doubles(B, ndim, T, M, ncols))
        return _gauss_newton(d, _lib.check, lib.cp_taylor_gauss_newton, need, head, where, B, ndim, start, ncols, weights, data, return_value)

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
