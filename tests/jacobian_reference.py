"""Restatement of the emulators' parameter derivatives for the tests (tests/test_jacobian_host.py, test_mlp_jacobian_gpu.py, test_taylor_jacobian_gpu.py,
test_emulator_jacobian_gpu.py): the forward-mode pass of the MLP on top of tests/mlp_reference.py and the derivative of the Taylor polynomial, in any
floating-point type.  ``np.longdouble`` is the truth, float64 the reference implementation that is not the code under test.

Tolerance rule (the rule of the gradient of ``cp_mlp_loss_grad``), :func:`levels` and :func:`assert_within`: a block is one
(parameter, output column) pair over the batch; its rounding level is the float64 restatement's largest distance from the longdouble truth relative
to the block's largest entry, floored at FLOOR = 1.1e-16 (no float64 result is expected closer to the truth than its own rounding); the device is
allowed ALLOW = 16 times that level (another summation order, MFMA steps of 4, its own exp)."""
import numpy as np

import mlp_reference as mr

LD = np.longdouble
FLOOR = 1.1e-16
ALLOW = 16.


def activate_derivative(name, v, alpha, beta):
    """act'(v) in the type of v; relu: 0 at v <= 0, and a NaN stays one."""
    if name == 'silu':
        s = mr.sigmoid(v)
        return s * (1 + v * (1 - s))
    if name == 'relu':
        return np.where(v != v, v, (v > 0).astype(v.dtype))
    if name == 'tanh':
        return 1 - np.tanh(v)**2
    s = mr.sigmoid(alpha * v)
    return (1 - beta) + beta * (s + alpha * v * s * (1 - s))


def mlp_jacobian(packed, dims, activations, X, xoffset, xscale, yoffset, yscale, yfunction, dtype='f8'):
    """(value (B, M), J (B, ndim, M)) of the engine's prediction by forward mode in ``dtype``: J[b, i, c] = d value[b, c] / d X[b, i]."""
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    layers = mr.unpack(packed, dims, dtype)
    ndim = dims[0]
    h = (t(X) - t(xoffset)) / t(xscale)
    dh = np.zeros((len(h), ndim, ndim), dtype=dtype)      # (point, parameter, neuron)
    dh[:, np.arange(ndim), np.arange(ndim)] = 1 / t(np.broadcast_to(xscale, (ndim,)))
    for (kernel, bias, alpha, beta), name in zip(layers[:-1], activations):
        z = h @ kernel + bias
        dz = dh @ kernel
        h = mr.activate(name, z, alpha, beta)
        dh = activate_derivative(name, z, alpha, beta)[:, None, :] * dz
    v = (h @ layers[-1][0] + layers[-1][1]) * t(yscale) + t(yoffset)
    dv = (dh @ layers[-1][0]) * t(yscale)
    if yfunction == 'log10':
        value = 10**v
        return value, dv * (np.log(np.asarray(10, dtype=dtype)) * value)[:, None, :]
    if yfunction == 'arcsinh':
        return np.sinh(v), dv * np.cosh(v)[:, None, :]
    return v, dv


def taylor_left(center, powers, X, dtype='f8'):
    """(B, ndim, T): entry (b, i, t) = p_ti (x_i - c_i)^(p_ti - 1) prod_{j != i} (x_j - c_j)^p_tj.  Factors of power 0 are skipped (exactly 1 for NaN, Inf),
    a term with p_ti = 0 is exactly 0 whatever x holds, p_ti = 1 drops the factor of x_i."""
    powers = np.asarray(powers)
    d = np.asarray(X).astype(dtype) - np.asarray(center).astype(dtype)
    B, ndim = d.shape
    left = np.zeros((B, ndim, len(powers)), dtype=dtype)
    for t, power in enumerate(powers):
        factors = {j: d[:, j]**int(p) for j, p in enumerate(power) if p > 0}
        for i, p in enumerate(power):
            if p <= 0:
                continue
            m = np.full(B, int(p), dtype=dtype)
            if p > 1:
                m = m * d[:, i]**int(p - 1)
            for j, f in factors.items():
                if j != i:
                    m = m * f
            left[:, i, t] = m
    return left


def taylor_predict(center, powers, derivatives, X, dtype='f8'):
    powers = np.asarray(powers)
    d = np.asarray(X).astype(dtype) - np.asarray(center).astype(dtype)
    mono = np.ones((len(d), len(powers)), dtype=dtype)
    for t, power in enumerate(powers):
        for j, p in enumerate(power):
            if p > 0:
                mono[:, t] = mono[:, t] * d[:, j]**int(p)
    return mono @ np.asarray(derivatives).astype(dtype)


def taylor_jacobian(center, powers, derivatives, X, dtype='f8'):
    """J (B, ndim, M) of the polynomial in ``dtype``."""
    return taylor_left(center, powers, X, dtype) @ np.asarray(derivatives).astype(dtype)


def levels(J_ld, J_64):
    """(top, level), each (ndim, ncols): per block the largest |entry| of the truth and the rounding level of the float64 restatement."""
    top = np.abs(J_ld).max(axis=0)
    dist = np.abs(np.asarray(J_64).astype(LD) - J_ld).max(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        level = np.where(top > 0, dist / top, 0)
    return top, np.maximum(np.asarray(level, dtype='f8'), FLOOR)


def assert_within(J_dev, J_ld, J_64, what='', extra=0.):
    """Every block of the device's J within ALLOW x its rounding level (plus ``extra``, relative as well) of the truth; prints the largest fraction used."""
    top, level = levels(J_ld, J_64)
    dist = np.abs(np.asarray(J_dev).astype(LD) - J_ld).max(axis=0)
    allowed = (ALLOW * level + extra) * top
    with np.errstate(divide='ignore', invalid='ignore'):
        fraction = np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0))
    print('%s: largest fraction of the allowance %.3g (level at most %.3g)' % (what, float(fraction.max()), float(level.max())))
    assert np.isfinite(np.asarray(J_dev)).all(), what
    assert float(fraction.max()) <= 1., '{}: block {} at {:.3g} of its allowance'.format(what, np.unravel_index(np.argmax(fraction), fraction.shape), float(fraction.max()))
