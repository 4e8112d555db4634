"""
Multi-layer perceptron emulator under the reference's name (cosmoprimo/emulators/tools/mlp.py ``MLPEmulatorEngine``): a network trained on quasi-random
samples over the whole prior box, predicted for B parameter points at once.

Predict is ONE launch (``cp_mlp_predict_columns``): the affine x operation, the hidden layers in LDS, the output layer on the matrix cores, the inverse of the
y operations in its epilogue -- where the reference evaluates one point per call in Python.  Fit is written here (the reference's is jax / flax / optax,
which this project does not depend on): the reference's procedure (mlp.py:142-147, 256-346: one stage per batch fraction, a fresh validation /
training split per stage from one ``RandomState(seed)``, whole batches only, validation loss after each epoch, the best state kept, early stopping,
the next stage from the best parameters with fresh Adam moments), a training step being ``cp_mlp_loss_grad`` then ``cp_mlp_adam`` with no host
synchronisation; the one read-back is the validation loss of an epoch.

``jacobian`` is the derivative of ``predict`` with respect to the raw parameters (what ``jax.jacfwd`` gives a user of the reference), analytic, by forward
mode through the network on the device (``cp_mlp_jacobian``).  ``vjp`` is its product with a cotangent, ``sum_c cotangent[b, c] J[b, i, c]`` (what
``jax.vjp`` / ``jax.grad`` give: the gradient of a scalar function of the outputs for every point of a batch), by reverse mode (``cp_mlp_vjp``): one
forward pass, one product with the transposed output kernel, one walk back through the hidden layers; the Jacobian is never formed.
``jvp`` is its product with tangents, ``sum_i tangent[b, k, i] J[b, i, c]`` (what ``jax.jvp`` / ``jax.linearize`` give), by forward mode with a row per
(point, direction) pair (``cp_mlp_jvp``).  ``jvp2`` is the second directional derivative ``sum_ij u[b, k, i] v[b, k, j] d^2 predict / d x_i d x_j`` (what
``jax.jvp`` of ``jax.jvp`` gives), by second-order forward mode with a row per (point, pair of directions) (``cp_mlp_jvp2``).
``predict``, ``jacobian``, ``vjp``, ``jvp`` and ``jvp2`` open with one prologue (``_enter``: fitted?, device state, upload and check of ``X``, the leading and the
last arguments of the C entry points); the full prediction is the column range (0, M) of ``cp_mlp_predict_columns``.

Operations are held as numbers, not as expressions: x a chain of affine maps ('scale', 'norm') folded into one (offset, scale) per parameter, y
optionally 'log10' or 'arcsinh' first, then affine maps.  Not built: 'pca', 'chebyshev', ``model_yoperation``, batch normalisation, learning-rate
schedules, callable losses, optimizers other than Adam (each raises ``NotImplementedError``), MPI, reading the reference's saved emulators.
"""
import ctypes

import numpy as np

from ... import _device as dv, _lib
from .base import _columns, _cotangent, _empty, _gauss_newton, _jacobian_out, _tangent

ACTIVATIONS = ('silu', 'relu', 'tanh', 'identity-silu')
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.999, 1e-8      # optax.adam's defaults
_TRUNCATED_STD = 0.87962566103423978               # standard deviation of a standard normal truncated at +-2 (flax divides by it)


def _per_stage(value, count):
    """``value`` as a tuple: a single number or name repeated ``count`` times, a sequence as it is."""
    return tuple(value) if np.ndim(value) else (value,) * count


def _make_list(obj):
    if obj is None:
        return []
    if isinstance(obj, (str, dict)):
        return [obj]
    return list(obj)


def _operation(operation):
    """{'name': ..., ['limits': ...]} from a name or such a dictionary."""
    if isinstance(operation, str):
        operation = {'name': operation}
    if not isinstance(operation, dict) or 'name' not in operation:
        raise ValueError('an operation is a name or a dictionary with a name, got {!r}'.format(operation))
    operation = dict(operation)
    operation['name'] = name = str(operation['name']).lower()
    if name in ('pca', 'chebyshev'):
        raise NotImplementedError("operation '{}' is not built (only 'scale', 'norm' and, for y, 'log10' / 'arcsinh' first)".format(name))
    if name not in ('scale', 'norm', 'log10', 'arcsinh'):
        raise ValueError('Unknown operation {}.'.format(name))
    return operation


def _operations(operation, allow_function):
    """List of operations with 'scale' appended unless the last one is 'scale' or 'norm' (reference mlp.py:65-67)."""
    operations = [_operation(op) for op in _make_list(operation)]
    for i, op in enumerate(operations):
        if op['name'] in ('log10', 'arcsinh') and not (allow_function and i == 0):
            raise NotImplementedError("operation '{}' is built as the first y operation only".format(op['name']))
    if not operations or operations[-1]['name'] not in ('scale', 'norm'):
        operations.append({'name': 'scale'})
    return operations


def initialize_affine(operation, values):
    """(offset, scale) of 'scale' / 'norm' on ``values`` (npoints, n), as the reference's ``ScaleOperation`` / ``NormOperation`` (base.py:849-879):
    limits given or min / max, or mean / standard deviation (ddof = 1); columns with zero spread get offset 0 (scale) and scale 1."""
    values = np.asarray(values, dtype='f8')
    if operation['name'] == 'scale':
        limits = list(operation.get('limits', None) or [None, None])
        lo = np.min(values, axis=0) if limits[0] is None else np.broadcast_to(np.asarray(limits[0], dtype='f8'), values.shape[1:]).copy()
        hi = np.max(values, axis=0) if limits[1] is None else np.broadcast_to(np.asarray(limits[1], dtype='f8'), values.shape[1:]).copy()
        mask = hi == lo
        lo, hi = np.where(mask, 0., lo), np.where(mask, 1., hi)
        return lo, hi - lo
    mean, sigma = np.mean(values, axis=0), np.std(values, ddof=1, axis=0)
    return mean, np.where(sigma == 0., 1., sigma)


def apply_operations(operations, values):
    """Forward operations (with their 'offset' / 'scale' set) on ``values``, one after the other as the reference applies them."""
    values = np.asarray(values, dtype='f8')
    for op in operations:
        if op['name'] == 'log10':
            values = np.log10(values)
        elif op['name'] == 'arcsinh':
            values = np.arcsinh(values)
        else:
            values = (values - op['offset']) / op['scale']
    return values


def invert_operations(operations, values):
    values = np.asarray(values, dtype='f8')
    for op in operations[::-1]:
        if op['name'] == 'log10':
            values = 10**values
        elif op['name'] == 'arcsinh':
            values = np.sinh(values)
        else:
            values = values * op['scale'] + op['offset']
    return values


def folded_affine(operations):
    """One (offset, scale) with ``(v - offset) / scale`` the chain of the affine operations."""
    offset, scale = 0., 1.
    for op in operations:
        if op['name'] in ('scale', 'norm'):      # ((v - o) / s - o') / s' = (v - (o + s o')) / (s s')
            offset, scale = offset + scale * op['offset'], scale * op['scale']
    return np.asarray(offset, dtype='f8'), np.asarray(scale, dtype='f8')


def split_indices(rng, nsamples, validation_frac):
    """(validation, training) indices of one stage: the three lines of the reference (mlp.py:260-262), drawn from ``rng``."""
    nvalidation = int(nsamples * float(validation_frac) + 0.5)
    if nvalidation >= nsamples:
        raise ValueError('validation_frac = {:g} leaves no training sample: {:d} of {:d} samples would be held out'.format(float(validation_frac), nvalidation, nsamples))
    index1 = rng.choice(nsamples, size=nvalidation, replace=False)
    index2 = rng.choice(nsamples, size=nsamples, replace=False)
    index2 = index2[~np.isin(index2, index1)]
    return index1, index2


def batch_slices(ntraining, batch_frac):
    """The whole batches of an epoch (mlp.py:269-276): the remainder is dropped."""
    batch_size = max(int(ntraining * min(batch_frac, 1.) + 0.5), 1)
    return [slice(i * batch_size, (i + 1) * batch_size) for i in range(ntraining // batch_size)]


def layer_sizes(ndim, nhidden, M):
    """[(offset, n_in, n_out)] of the layers in the packed buffer, and its length: per layer kernel (n_in, n_out), bias (n_out), and for a hidden layer
    alpha, beta."""
    dims = [int(ndim)] + [int(n) for n in nhidden] + [int(M)]
    layers, offset = [], 0
    for l in range(len(dims) - 1):
        layers.append((offset, dims[l], dims[l + 1]))
        offset += (dims[l] + 1) * dims[l + 1] + (2 if l < len(dims) - 2 else 0)
    return layers, offset


def pack_parameters(layers):
    """Packed buffer from [{'kernel', 'bias', ['alpha', 'beta']}] per layer."""
    chunks = []
    for i, layer in enumerate(layers):
        chunks += [np.ravel(np.asarray(layer['kernel'], dtype='f8')), np.ravel(np.asarray(layer['bias'], dtype='f8'))]
        if i < len(layers) - 1:
            chunks.append(np.array([layer.get('alpha', 0.), layer.get('beta', 0.)], dtype='f8'))
    return np.concatenate(chunks)


def unpack_parameters(packed, ndim, nhidden, M):
    sizes, total = layer_sizes(ndim, nhidden, M)
    packed = np.asarray(packed, dtype='f8')
    if packed.shape != (total,):
        raise ValueError('packed parameters must be of shape ({:d},), got {}'.format(total, packed.shape))
    layers = []
    for l, (offset, nin, nout) in enumerate(sizes):
        layer = {'kernel': packed[offset:offset + nin * nout].reshape(nin, nout), 'bias': packed[offset + nin * nout:offset + (nin + 1) * nout]}
        if l < len(sizes) - 1:
            layer['alpha'], layer['beta'] = packed[offset + (nin + 1) * nout], packed[offset + (nin + 1) * nout + 1]
        layers.append(layer)
    return layers


class MLPEmulatorEngine(object):

    """Multi-layer perceptron emulator engine.  State: ``nhidden``, ``activation``, ``parameters`` (the packed buffer: per layer kernel, bias and, for a
    hidden layer, alpha and beta), ``xoperations`` / ``yoperations`` (names with their offsets and scales), ``params``, ``name``."""
    name = 'mlp'

    def __init__(self, nhidden=(32, 32, 32), activation='silu', loss='mse', xoperation=None, yoperation=None, device=None, model_yoperation=None, **kwargs):
        if model_yoperation is not None:
            raise NotImplementedError('model_yoperation is not built')
        if kwargs:
            raise TypeError('unexpected arguments {}'.format(sorted(kwargs)))
        if not (isinstance(loss, str) and loss == 'mse'):
            raise NotImplementedError("loss {!r} is not built (only 'mse')".format(loss))
        self.nhidden = tuple(int(n) for n in nhidden)
        self.activation = tuple(str(a) for a in _per_stage(activation, len(self.nhidden)))
        if len(self.activation) != len(self.nhidden):
            raise ValueError('provide one activation, or one per hidden layer ({:d}), got {}'.format(len(self.nhidden), self.activation))
        for name in self.activation:
            if name not in ACTIVATIONS:
                raise ValueError('unknown activation {}'.format(name))
        self.loss = loss
        self.xoperations = _operations(xoperation, allow_function=False)
        self.yoperations = _operations(yoperation, allow_function=True)
        self.device = device
        self.params = None
        self.parameters = None
        self.history = []
        self._dev = None

    def get_default_samples(self, calculator, params, engine='rqrs', niterations=10**4, **kwargs):
        """Samples of a :class:`QMCSampler` (``kwargs``: its ``batch_size``, or arguments of the scipy engine such as ``seed``)."""
        from .samples import QMCSampler
        batch_size = kwargs.pop('batch_size', None)
        sampler = QMCSampler(calculator, params, engine=engine, **kwargs)
        return sampler.run(niterations=niterations, batch_size=batch_size)

    def initial_parameters(self, ndim, M, seed=42):
        """Packed initial parameters: kernels as flax's ``Dense`` default (LeCun normal: variance 1 / n_in, a normal truncated at two standard deviations),
        biases, alpha and beta zero.  Drawn on the host from ``np.random.RandomState(seed)``: they cannot equal the reference's draws, which come from
        jax's generator."""
        rng = np.random.RandomState(seed=seed)
        sizes, total = layer_sizes(ndim, self.nhidden, M)
        packed = np.zeros(total, dtype='f8')
        for offset, nin, nout in sizes:
            draws = rng.standard_normal(nin * nout)
            while True:      # redraw what falls outside +-2
                bad = np.abs(draws) > 2.
                if not bad.any():
                    break
                draws[bad] = rng.standard_normal(int(bad.sum()))
            packed[offset:offset + nin * nout] = draws * (np.sqrt(1. / nin) / _TRUNCATED_STD)
        return packed

    def _net(self, ndim, M):
        """The ctypes view of the network (host arrays the C ABI reads at every call), checked against the kernels' caps."""
        L = len(self.nhidden)
        widths = (ctypes.c_int * max(L, 1))(*self.nhidden)
        acts = (ctypes.c_int * max(L, 1))(*[_lib.MLP_ACTIVATIONS[name] for name in self.activation])
        total = _lib.load().cp_mlp_param_count(int(ndim), L, widths, int(M))
        if total < 0:      # minus the status: a cap is NotImplementedError, a bad count ValueError
            _lib.check(-int(total))
        return dict(ndim=int(ndim), M=int(M), L=L, widths=widths, acts=acts, total=int(total))

    def fit(self, X, Y, attrs=None, params=None, validation_frac=0.1, batch_frac=(0.1, 0.3, 1.), epochs=1000, learning_rate=(1e-2, 1e-3, 1e-5), patience=100, seed=42,
            optimizer='adam', loss=None, learning_rate_scheduling=False, batch_norm=False):
        """Fit to samples ``X`` (npoints, ndim), ``Y`` (npoints, M) by the reference's procedure (module docstring).  ``attrs``: the samples' attributes,
        which :class:`Emulator` hands every engine; this one reads none of them.  ``epochs``, ``learning_rate``,
        ``patience``: one value, or one per entry of ``batch_frac``.  Initial weights: :meth:`initial_parameters` -- not jax's draws, so a fit does not
        reproduce the reference's weights, only its procedure.  ``history``: per stage ``batch_size``, ``epochs`` run, ``best_loss``, ``losses``."""
        if optimizer != 'adam':
            raise NotImplementedError("optimizer {!r} is not built (only 'adam')".format(optimizer))
        if loss is not None and not (isinstance(loss, str) and loss == 'mse'):
            raise NotImplementedError("loss {!r} is not built (only 'mse')".format(loss))
        if learning_rate_scheduling:
            raise NotImplementedError('learning_rate_scheduling is not built')
        if batch_norm:
            raise NotImplementedError('batch_norm=True is not built')
        X, Y = np.asarray(X, dtype='f8'), np.asarray(Y, dtype='f8')
        if X.ndim != 2 or Y.ndim != 2 or len(X) != len(Y):
            raise ValueError('X (npoints, ndim) and Y (npoints, M) must share npoints, got {} and {}'.format(X.shape, Y.shape))
        self.params = list(params) if params is not None else None
        nsamples, ndim = X.shape
        M = Y.shape[1]
        net = self._net(ndim, M)
        # the operations, initialised one after the other on what the previous ones give (reference base.py:610-618), y first
        for operations, values in ((self.yoperations, Y), (self.xoperations, X)):
            for i, op in enumerate(operations):
                if op['name'] in ('scale', 'norm'):
                    op['offset'], op['scale'] = initialize_affine(op, apply_operations(operations[:i], values))
        Xs, Ys = apply_operations(self.xoperations, X), apply_operations(self.yoperations, Y)
        if not (np.isfinite(Xs).all() and np.isfinite(Ys).all()):
            raise ValueError('samples are not finite after the x / y operations')
        list_batch_frac = _per_stage(batch_frac, 1)
        list_epochs = _per_stage(epochs, len(list_batch_frac))
        list_learning_rate = _per_stage(learning_rate, len(list_batch_frac))
        list_patience = _per_stage(patience, len(list_batch_frac))
        rng = np.random.RandomState(seed=seed)
        torch = dv.torch()
        device = dv.resolve_device(self.device)
        lib, stream, index = _lib.load(), dv.stream_of(device), device.index
        Xd, Yd = (torch.as_tensor(np.ascontiguousarray(a), device=device) for a in (Xs, Ys))      # uploaded once
        p = torch.as_tensor(self.initial_parameters(ndim, M, seed=seed), device=device)
        best, grad, m, v = (torch.empty_like(p) for _ in range(4))
        best.copy_(p)
        loss_d = torch.zeros(1, dtype=torch.float64, device=device)
        self.history = []

        def workspace(b):
            return torch.empty(int(lib.cp_mlp_workspace_doubles(int(b), ndim, net['L'], net['widths'], M)), dtype=torch.float64, device=device)

        def loss_grad(Xb, Yb, work, g):
            _lib.check(lib.cp_mlp_loss_grad(Xb.data_ptr(), Yb.data_ptr(), int(Xb.shape[0]), ndim, net['L'], net['widths'], net['acts'], M, p.data_ptr(), work.data_ptr(),
                                            work.numel(), loss_d.data_ptr(), g.data_ptr() if g is not None else None, index, stream))

        for stage_batch_frac, stage_epochs, stage_lr, stage_patience in zip(list_batch_frac, list_epochs, list_learning_rate, list_patience):
            index1, index2 = split_indices(rng, nsamples, validation_frac)
            i1, i2 = (torch.as_tensor(idx, device=device) for idx in (index1, index2))
            Xv, Yv, Xt, Yt = Xd[i1], Yd[i1], Xd[i2], Yd[i2]
            slices = batch_slices(len(index2), stage_batch_frac)
            batch_size = slices[0].stop - slices[0].start if slices else 0
            work_t, work_v = workspace(batch_size), workspace(len(index1))
            p.copy_(best)      # the best state of the previous stage, fresh moments
            m.zero_()
            v.zero_()
            best_loss, counter, step, losses = np.inf, 0, 0, []
            for epoch in range(int(stage_epochs)):
                for sl in slices:
                    step += 1
                    loss_grad(Xt[sl], Yt[sl], work_t, grad)
                    _lib.check(lib.cp_mlp_adam(p.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), p.numel(), float(stage_lr), ADAM_B1, ADAM_B2, ADAM_EPS,
                                               1. - ADAM_B1**step, 1. - ADAM_B2**step, index, stream))
                if len(index1):
                    loss_grad(Xv, Yv, work_v, None)
                    value = float(loss_d.item())      # the one read-back of an epoch
                else:
                    value = np.nan
                losses.append(value)
                if value < best_loss:
                    best_loss, counter = value, 0
                    best.copy_(p)
                else:
                    counter += 1
                if counter >= stage_patience:
                    break
            self.history.append({'batch_size': batch_size, 'learning_rate': float(stage_lr), 'epochs': len(losses), 'best_loss': float(best_loss), 'losses': losses})
        self.parameters = dv.to_host(best)
        self.ndim, self.M = ndim, M
        self._set_device(device, best)
        return self

    def _set_device(self, device, parameters=None):
        net = self._net(self.ndim, self.M)
        if parameters is None:
            packed = np.ascontiguousarray(self.parameters, dtype='f8')
            if packed.shape != (net['total'],):
                raise ValueError('parameters must be of shape ({:d},), got {}'.format(net['total'], packed.shape))
            parameters = dv.to_device(packed, device, cache=False)
        xoffset, xscale = (np.ascontiguousarray(np.broadcast_to(a, (self.ndim,))) for a in folded_affine(self.xoperations))
        yoffset, yscale = (np.ascontiguousarray(np.broadcast_to(a, (self.M,))) for a in folded_affine(self.yoperations))
        first = self.yoperations[0]['name']
        self._dev = dict(device=device, torch=dv.torch(), net=net, parameters=parameters, yfunction=_lib.MLP_YFUNCTIONS[first if first in ('log10', 'arcsinh') else None],
                         **{name: dv.to_device(value, device, cache=False) for name, value in dict(xoffset=xoffset, xscale=xscale, yoffset=yoffset, yscale=yscale).items()})
        # what every call of the C entry points passes after the points: the network and the operations (the tensors live as long as this dictionary)
        d = self._dev
        d['head'] = (net['ndim'], net['L'], net['widths'], net['acts'], net['M']) + tuple(d[name].data_ptr() for name in ('parameters', 'xoffset', 'xscale', 'yoffset', 'yscale')) \
            + (d['yfunction'],)

    def _enter(self, X):
        """The opening of :meth:`predict`, :meth:`jacobian` and :meth:`vjp`: the device state (set at the first call), ``X`` (B, ndim) on its device, B, the 13
        leading arguments of the C entry points (the points, the network, the operations) and their last two (device, stream)."""
        if self.parameters is None:
            raise ValueError('fit the engine first')
        if self._dev is None:
            self._set_device(dv.resolve_device(self.device, X))
        d = self._dev
        net = d['net']
        X = dv.to_device(X, d['device'], cache=False)
        if X.ndim != 2 or int(X.shape[1]) != net['ndim']:
            raise ValueError('X must be of shape (B, {:d}), got {}'.format(net['ndim'], tuple(X.shape)))
        B = int(X.shape[0])
        head = (X.data_ptr(), B) + d['head']
        return d, X, B, head, (d['device'].index, dv.stream_of(d['device']))

    def predict(self, X, columns=None):
        """Network at the points ``X`` (B, ndim) of raw parameters, a device tensor (or host array, uploaded): device tensor (B, M) of the calculator's
        outputs (the y operations inverted).  One launch; nothing but the result is allocated, nothing is read back and the call does not wait for the
        device.  ``columns = (start, stop)``: those columns of it only, a (B, stop - start) tensor, bit for bit the same numbers
        (``cp_mlp_predict_columns``: the hidden layers as ever, the output layer and the y operations on that range alone; every column is the range
        (0, M) of the same call, so a refusal names that entry point; ``cp_mlp_predict`` itself is there for C callers)."""
        d, X, B, head, where = self._enter(X)
        start, ncols = _columns(columns, d['net']['M'])
        out = _empty(d, B, max(ncols, 0))
        _lib.check(_lib.load().cp_mlp_predict_columns(*head, start, ncols, out.data_ptr(), ncols, *where))
        return out

    def jacobian(self, X, columns=None, return_value=False, out=None):
        """Derivative of :meth:`predict` with respect to the raw parameters at the points ``X`` (B, ndim): device tensor ``J`` (B, ndim, M),
        ``J[b, i, c] = d predict(X)[b, c] / d X[b, i]``, computed analytically by forward mode through the network (``cp_mlp_jacobian``: the x operations
        contribute 1 / xscale[i], the inverse y operations yscale[c] f'(v) with f' the derivative of 10^v or sinh v).  ``columns = (start, stop)``: those
        output columns only, (B, ndim, stop - start), bit for bit the same numbers.  ``return_value=True``: ``(value, J)`` with ``value`` what
        ``predict(X, columns=columns)`` returns, bit for bit.  Nothing is read back and the call does not wait for the device.
        ``out = (value or None, J)``: device tensors to write instead of new ones, views into wider buffers with rows of any stride
        (:func:`base._jacobian_out`)."""
        d, X, B, head, where = self._enter(X)
        start, ncols = _columns(columns, d['net']['M'])
        width = max(ncols, 0)
        value, ldv, jac, ldj = _jacobian_out(d, out, B, d['net']['ndim'], width, return_value or out is None)
        if value is None:      # the kernel writes the value in any case
            value, ldv = _empty(d, B, width), width
        _lib.check(_lib.load().cp_mlp_jacobian(*head, start, ncols, value.data_ptr(), ldv, jac.data_ptr(), ldj, *where))
        return (value, jac) if return_value else jac

    def vjp(self, X, cotangent, columns=None, return_value=False):
        """Vector-Jacobian product of :meth:`predict` at the points ``X`` (B, ndim): device tensor ``G`` (B, ndim),
        ``G[b, i] = sum_c cotangent[b, c] d predict(X)[b, c] / d X[b, i]``, by reverse mode through the network (``cp_mlp_vjp``: three launches whatever the
        depth, no (B, ndim, M) array anywhere).  ``cotangent``: (B, M) device tensor (or host array, uploaded), rows of any stride.
        ``columns = (start, stop)``: the sum over those output columns only, ``cotangent`` (B, stop - start).  ``return_value=True``:
        ``(predict(X, columns=columns), G)``, the value bit for bit, from the same forward pass.  Nothing is read back and the call does not wait for
        the device."""
        d, X, B, head, where = self._enter(X)
        net = d['net']
        start, ncols = _columns(columns, net['M'])
        width = max(ncols, 0)
        cotangent, ldc = _cotangent(cotangent, B, width, d['device'])
        lib = _lib.load()
        need = int(lib.cp_mlp_vjp_workspace_doubles(B, net['ndim'], net['L'], net['widths'], net['M'], width))
        if need < 0:
            _lib.check(-need)
        work, grad = _empty(d, need), _empty(d, B, net['ndim'])
        value = _empty(d, B, width) if return_value else None
        _lib.check(lib.cp_mlp_vjp(*head, start, ncols, cotangent.data_ptr(), ldc, value.data_ptr() if return_value else None, width, grad.data_ptr(), work.data_ptr(), need,
                                  *where))
        return (value, grad) if return_value else grad

    def vjp2(self, X, cotangent, columns=None, return_value=False):
        """Second derivatives of :meth:`predict` contracted with a cotangent at the points ``X`` (B, ndim): device tensor ``C`` (B, ndim, ndim),
        ``C[b, i, j] = sum_c cotangent[b, c] d^2 predict(X)[b, c] / d X[b, i] d X[b, j]``, symmetric bit for bit -- with ``cotangent = w (data - predict)``
        the residual-curvature term of the Hessian of chi2 (``cp_mlp_vjp2``: the output layer is contracted with the cotangent once per point as in
        :meth:`vjp`, then second-order forward mode with a row per (point, pair i <= j) ends in a dot product over the last hidden layer; with a
        y function its own curvature is a Gauss-Newton contraction with signed weights; no (B, ndim (ndim + 1) / 2, M) array anywhere).  ``cotangent``,
        ``columns`` and ``return_value`` as in :meth:`vjp`.  Nothing is read back and the call does not wait for the device."""
        d, X, B, head, where = self._enter(X)
        net = d['net']
        start, ncols = _columns(columns, net['M'])
        width = max(ncols, 0)
        cotangent, ldc = _cotangent(cotangent, B, width, d['device'])
        lib = _lib.load()
        need = int(lib.cp_mlp_vjp2_workspace_doubles(B, net['ndim'], net['L'], net['widths'], net['M'], width, d['yfunction']))
        if need < 0:
            _lib.check(-need)
        work, hess = _empty(d, need), _empty(d, B, net['ndim'], net['ndim'])
        value = _empty(d, B, width) if return_value else None
        _lib.check(lib.cp_mlp_vjp2(*head, start, ncols, cotangent.data_ptr(), ldc, value.data_ptr() if return_value else None, width, hess.data_ptr(), work.data_ptr(), need,
                                   *where))
        return (value, hess) if return_value else hess

    def jvp(self, X, tangents, columns=None, return_value=False):
        """Jacobian-vector product of :meth:`predict` at the points ``X`` (B, ndim) along ``tangents`` (B, ndim) -- device tensor (B, M),
        ``out[b, c] = sum_i tangents[b, i] d predict(X)[b, c] / d X[b, i]`` -- or (B, K, ndim), K directions per point -- (B, K, M) --, a device tensor or
        host array (uploaded), in raw-parameter units; by forward mode through the network with a row per (point, direction) pair (``cp_mlp_jvp``: the
        kernel of :meth:`jacobian` with ``tangents / xscale`` as the input tangent; no (B, ndim, M) array anywhere, and ndim identity tangents give the
        bits of :meth:`jacobian`).  ``columns = (start, stop)``: those output columns only, bit for bit the same numbers.  ``return_value=True``:
        ``(predict(X, columns=columns), out)``, the value bit for bit.  Nothing is read back and the call does not wait for the device."""
        d, X, B, head, where = self._enter(X)
        start, ncols = _columns(columns, d['net']['M'])
        width = max(ncols, 0)
        tangents, K, single = _tangent(tangents, B, d['net']['ndim'], d['device'])
        value, out = _empty(d, B, width), _empty(d, B, K, width)
        _lib.check(_lib.load().cp_mlp_jvp(*head, start, ncols, tangents.data_ptr(), K, value.data_ptr(), width, out.data_ptr(), width, *where))
        out = out[:, 0] if single else out
        return (value, out) if return_value else out

    def jvp2(self, X, tangents, tangents2=None, columns=None, return_value=False, return_first=False):
        """Second directional derivatives of :meth:`predict` at the points ``X`` (B, ndim) along the pairs of directions ``tangents``, ``tangents2``, both
        (B, ndim) -- device tensor (B, M), ``out[b, c] = sum_ij tangents[b, i] tangents2[b, j] d^2 predict(X)[b, c] / d X[b, i] d X[b, j]`` -- or
        (B, K, ndim), K pairs per point -- (B, K, M) --, device tensors or host arrays (uploaded), in raw-parameter units; ``tangents2=None``: the
        second directional derivative along ``tangents``.  By second-order forward mode through the network with a row per (point, pair) (``cp_mlp_jvp2``:
        no (B, ndim, ndim, M) array anywhere; exchanging the two sets gives the same bits).  ``columns = (start, stop)``: those output columns only, bit
        for bit the same numbers.  ``return_value=True``: ``predict(X, columns=columns)`` is prepended, bit for bit; ``return_first=True``: what
        :meth:`jvp` gives along ``tangents`` (and along ``tangents2``, where given) is inserted before the result, bit for bit.  Nothing is read back and
        the call does not wait for the device."""
        d, X, B, head, where = self._enter(X)
        start, ncols = _columns(columns, d['net']['M'])
        width = max(ncols, 0)
        tangents, K, single = _tangent(tangents, B, d['net']['ndim'], d['device'])
        mixed = tangents2 is not None
        if mixed:
            tangents2, K2, single2 = _tangent(tangents2, B, d['net']['ndim'], d['device'])
            if (K2, single2) != (K, single):
                raise ValueError('tangents and tangents2 must share one shape')
        first = return_first or d['yfunction'] != 0      # the y function's chain rule reads the first-order products
        value, out = _empty(d, B, width), _empty(d, B, K, width)
        firsts = [_empty(d, B, K, width) if first else None for _ in range(2 if mixed else 1)] + ([] if mixed else [None])
        ptr = lambda tensor: tensor.data_ptr() if tensor is not None else None      # noqa: E731
        _lib.check(_lib.load().cp_mlp_jvp2(*head, start, ncols, tangents.data_ptr(), ptr(tangents2), K, value.data_ptr(), width, ptr(firsts[0]), ptr(firsts[1]), width,
                                           out.data_ptr(), width, *where))
        toret = ([value] if return_value else []) + ([f[:, 0] if single else f for f in firsts if f is not None] if return_first else [])
        toret.append(out[:, 0] if single else out)
        return tuple(toret) if len(toret) > 1 else toret[0]

    def gauss_newton(self, X, weights, data=None, columns=None, return_value=False):
        """Fisher matrices and Gauss-Newton normal equations of :meth:`predict` at the points ``X`` (B, ndim), with ``J`` the Jacobian of :meth:`jacobian`:
        device tensors ``fisher`` (B, ndim, ndim), ``fisher[b, i, j] = sum_c weights[b, c] J[b, i, c] J[b, j, c]`` (symmetric bit for bit), and with
        ``data`` ``(fisher, grad, chi2)``, ``grad[b, i] = sum_c weights[b, c] (data[b, c] - predict(X)[b, c]) J[b, i, c]`` (B, ndim) and
        ``chi2[b] = sum_c weights[b, c] (data[b, c] - predict(X)[b, c])^2`` (B,) (``cp_mlp_gauss_newton``: the tangent kernel's tile of ``J`` is contracted
        over its columns in registers and LDS; no (B, ndim, M) array anywhere).  ``weights``, ``data``: (M,) shared by all points or (B, M), device tensors
        or host arrays (uploaded), rows of any stride.  A weight of exactly 0 drops its column, whatever it holds.  ``columns = (start, stop)``: the sums
        over those output columns only, ``weights`` and ``data`` (stop - start,) or (B, stop - start).  ``return_value=True``:
        ``predict(X, columns=columns)`` is prepended, bit for bit.  Nothing is read back and the call does not wait for the device."""
        d, X, B, head, where = self._enter(X)
        net = d['net']
        start, ncols = _columns(columns, net['M'])
        lib = _lib.load()
        need = int(lib.cp_mlp_gauss_newton_workspace_doubles(B, net['ndim'], net['L'], net['widths'], net['M'], ncols))
        return _gauss_newton(d, _lib.check, lib.cp_mlp_gauss_newton, need, head, where, B, net['ndim'], start, ncols, weights, data, return_value)

    def __getstate__(self):
        state = {'name': self.name, 'nhidden': tuple(self.nhidden), 'activation': tuple(self.activation), 'params': self.params,
                 'xoperations': [dict(op) for op in self.xoperations], 'yoperations': [dict(op) for op in self.yoperations]}
        if self.parameters is not None:
            state.update(parameters=np.asarray(self.parameters), ndim=self.ndim, M=self.M)
        return state

    def __setstate__(self, state):
        self.nhidden = tuple(int(n) for n in state['nhidden'])
        self.activation = tuple(str(a) for a in state['activation'])
        self.loss = 'mse'
        self.params = list(state['params']) if state.get('params', None) is not None else None
        self.xoperations, self.yoperations = ([dict(op) for op in state[name]] for name in ('xoperations', 'yoperations'))
        self.device, self._dev, self.history = None, None, []
        self.parameters = None
        if 'parameters' in state:
            self.parameters = np.asarray(state['parameters'], dtype='f8')
            self.ndim, self.M = int(state['ndim']), int(state['M'])

    @classmethod
    def from_state(cls, state, device=None):
        new = cls.__new__(cls)
        new.__setstate__(state)
        new.device = device
        return new
