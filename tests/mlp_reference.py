"""Restatement of the MLP emulator's arithmetic for the tests (tests/test_mlp_host.py, test_mlp_gpu.py, test_mlp_edges_gpu.py, test_mlp_train_edges_gpu.py): forward and manual
backward pass in any floating-point type (``np.longdouble`` is the truth, float64 the reference implementation that is not the code under test), the
running error bound of the forward pass, and Adam.

Forward bound (derived, not measured; eps = 2^-53).  Next to the longdouble truth h a bound err on the float64 result's distance from it is carried:
* input: x' = (x - offset) / scale, two roundings: 2 eps |x'|;
* layer z = h W + b: ``|W|^T err_in + 2 (n_in + 2) eps (|W|^T |h| + |b|)`` -- ``dot_bound`` of tests/test_taylor_edges_gpu.py with the bias as one more term;
  the factor 2 because the reference's float64 product and the device's each carry that error;
* activation: err_z times its Lipschitz constant (relu, tanh 1; silu 1.1, the maximum of its derivative 1.0998; identity-silu |1 - beta| + 1.1 |beta|,
  for d/dv [v s(alpha v)] is silu' at alpha v) plus its own rounding: ACT_EPS |h| with ACT_EPS = 2.3e-16 + 2 eps for silu and tanh (2.3e-16 is what
  tests/test_math_gpu.py holds the device's exp to; 1 + e and the division add eps each, and e / (1 + e) <= 1), 0 for relu, and for identity-silu
  (2.3e-16 + 5 eps) (|1 - beta| + |beta|) |v| (the product alpha v shifts exp's argument by eps |alpha v|, and |a| s (1 - s) <= 0.23; 1 - beta, the sum and
  the product with v add eps each);
* epilogue y = v scale + offset: ``|scale| err + 2 eps (|v scale| + |offset|)``, then 10^y: ``10^y (expm1(ln 10 err_y) + 2.3e-16 + eps)``."""
import numpy as np

EPS = 2.**-53
LD = np.longdouble
EXP_EPS = 2.3e-16
ACT_EPS = EXP_EPS + 2. * EPS
ACTIVATIONS = ('silu', 'relu', 'tanh', 'identity-silu')


def unpack(packed, dims, dtype='f8'):
    """[(kernel, bias, alpha, beta)] per layer from the packed buffer (alpha = beta = None for the output layer)."""
    packed = np.asarray(packed).astype(dtype)
    layers, offset = [], 0
    for l in range(len(dims) - 1):
        nin, nout = dims[l], dims[l + 1]
        kernel = packed[offset:offset + nin * nout].reshape(nin, nout)
        bias = packed[offset + nin * nout:offset + (nin + 1) * nout]
        offset += (nin + 1) * nout
        alpha = beta = None
        if l < len(dims) - 2:
            alpha, beta = packed[offset], packed[offset + 1]
            offset += 2
        layers.append((kernel, bias, alpha, beta))
    assert offset == packed.size
    return layers


def nparams(dims):
    return sum((dims[l] + 1) * dims[l + 1] for l in range(len(dims) - 1)) + 2 * (len(dims) - 2)


def blocks(dims):
    """{name: slice} of the packed buffer: per layer kernel, bias and (hidden layers) the pair alpha, beta."""
    out, offset = {}, 0
    for l in range(len(dims) - 1):
        nin, nout = dims[l], dims[l + 1]
        out['kernel%d' % l] = slice(offset, offset + nin * nout)
        out['bias%d' % l] = slice(offset + nin * nout, offset + (nin + 1) * nout)
        offset += (nin + 1) * nout
        if l < len(dims) - 2:
            out['alphabeta%d' % l] = slice(offset, offset + 2)
            offset += 2
    return out


def sigmoid(v):
    return 1 / (1 + np.exp(-v))


def activate(name, v, alpha, beta):
    if name == 'silu':
        return v / (1 + np.exp(-v))
    if name == 'relu':
        return np.maximum(v, 0)
    if name == 'tanh':
        return np.tanh(v)
    return ((1 - beta) + beta / (1 + np.exp(-alpha * v))) * v


def forward(layers, activations, X):
    """(pre-activations, activations with X first, output) in the type of X and the layers."""
    h, zs, hs = X, [], [X]
    for (kernel, bias, alpha, beta), name in zip(layers[:-1], activations):
        z = h @ kernel + bias
        h = activate(name, z, alpha, beta)
        zs.append(z)
        hs.append(h)
    return zs, hs, h @ layers[-1][0] + layers[-1][1]


def predict(packed, dims, activations, X, xoffset, xscale, yoffset, yscale, yfunction, dtype='f8'):
    """The engine's prediction restated: affine x operation, network, inverse y operations."""
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    v = forward(unpack(packed, dims, dtype), activations, (t(X) - t(xoffset)) / t(xscale))[2] * t(yscale) + t(yoffset)
    if yfunction == 'log10':
        return 10**v
    return np.sinh(v) if yfunction == 'arcsinh' else v


def predict_bound(packed, dims, activations, X, xoffset, xscale, yoffset, yscale, yfunction):
    """(truth rounded to float64, bound) of the module docstring, both (B, M)."""
    t = lambda a: np.asarray(a).astype(LD)      # noqa: E731
    layers = unpack(packed, dims, LD)
    h = (t(X) - t(xoffset)) / t(xscale)
    err = 2 * EPS * np.abs(h)
    for l, (kernel, bias, alpha, beta) in enumerate(layers):
        z = h @ kernel + bias
        err = err @ np.abs(kernel) + 2 * (kernel.shape[0] + 2) * EPS * (np.abs(h) @ np.abs(kernel) + np.abs(bias))
        if l == len(layers) - 1:
            h = z
            break
        name = activations[l]
        h = activate(name, z, alpha, beta)
        if name == 'silu':
            err = 1.1 * err + ACT_EPS * np.abs(h)
        elif name == 'tanh':
            err = err + ACT_EPS * np.abs(h)
        elif name == 'identity-silu':
            err = (abs(1 - beta) + 1.1 * abs(beta)) * err + (EXP_EPS + 5 * EPS) * (abs(1 - beta) + abs(beta)) * np.abs(z)
    v = h * t(yscale) + t(yoffset)
    err = np.abs(t(yscale)) * err + 2 * EPS * (np.abs(h * t(yscale)) + np.abs(t(yoffset)))
    if yfunction == 'log10':
        v = LD(10)**v
        err = v * (np.expm1(np.log(LD(10)) * err) + EXP_EPS + EPS)
    elif yfunction == 'arcsinh':
        err = np.cosh(np.abs(v) + err) * err + (EXP_EPS + 3 * EPS) * np.cosh(v)
        v = np.sinh(v)
    return np.asarray(v, dtype='f8'), np.asarray(err, dtype='f8') + EPS * np.abs(np.asarray(v, dtype='f8'))      # (+ the rounding of the truth itself)


def loss_grad(packed, dims, activations, X, Y, dtype='f8'):
    """MSE loss mean((Y - prediction)^2) and its gradient in the packed layout by a manual backward pass, in ``dtype``."""
    layers = unpack(packed, dims, dtype)
    X, Y = np.asarray(X).astype(dtype), np.asarray(Y).astype(dtype)
    zs, hs, out = forward(layers, activations, X)
    r = out - Y
    loss = np.mean(r**2)
    g = 2 * r / r.size
    grads = [None] * len(layers)
    grads[-1] = [hs[-1].T @ g, g.sum(axis=0)]
    dh = g @ layers[-1][0].T
    for l in range(len(layers) - 2, -1, -1):
        kernel, bias, alpha, beta = layers[l]
        v, name = zs[l], activations[l]
        extra = [np.zeros((), dtype=dtype)] * 2
        if name == 'silu':
            s = sigmoid(v)
            d = s * (1 + v * (1 - s))
        elif name == 'relu':
            d = (v > 0).astype(dtype)
        elif name == 'tanh':
            d = 1 - np.tanh(v)**2
        else:
            s = sigmoid(alpha * v)
            d = (1 - beta) + beta * (s + alpha * v * s * (1 - s))
            extra = [np.sum(dh * beta * s * (1 - s) * v * v), np.sum(dh * (s - 1) * v)]
        dz = dh * d
        grads[l] = [hs[l].T @ dz, dz.sum(axis=0), np.array(extra, dtype=dtype)]
        dh = dz @ kernel.T
    return loss, np.concatenate([np.ravel(a) for layer in grads for a in layer])


def gradient_levels(packed, dims, activations, X, Y):
    """Per block of the packed layout: (largest |gradient| of the longdouble pass, rounding level of the float64 pass = its largest distance from the
    longdouble one relative to that, floored at eps -- no float64 result is expected closer to the truth than its own rounding), with the longdouble
    loss and gradient and the float64 ones."""
    loss_ld, grad_ld = loss_grad(packed, dims, activations, X, Y, LD)
    loss_64, grad_64 = loss_grad(packed, dims, activations, X, Y, 'f8')
    levels = {}
    for name, sl in blocks(dims).items():
        top = float(np.abs(grad_ld[sl]).max())
        levels[name] = (top, max(float(np.abs(grad_64[sl] - grad_ld[sl]).max()) / top, EPS) if top > 0. else 0.)
    return levels, (loss_ld, grad_ld), (loss_64, grad_64)


def adam(p, m, v, g, lr, step, b1=0.9, b2=0.999, eps=1e-8):
    """One Adam step (optax.adam), every operation rounded once: new (p, m, v)."""
    m = b1 * m + (1. - b1) * g
    v = b2 * v + (1. - b2) * (g * g)
    return p - lr * (m / (1. - b1**step)) / (np.sqrt(v / (1. - b2**step)) + eps), m, v


def toy(a, b, c):
    """The toy function of tools/gen_taylor_golden.py: 3 parameters, 8 outputs."""
    x = np.linspace(0.1, 1., 7)
    a, b, c = (np.asarray(v, dtype='f8')[..., None] for v in (a, b, c))
    return np.concatenate([np.exp(a * x) * np.sin(b * x) + c**3 * x, a * b * c], axis=-1)


TOY_LIMITS = {'a': (0.8, 1.2), 'b': (1.8, 2.2), 'c': (0.4, 0.6)}


def golden_config(g, i):
    dims = (3,) + tuple(int(n) for n in g['c%d_nhidden' % i]) + (g['c%d_Yq' % i].shape[1],)
    return dict(dims=dims, activations=[str(a) for a in g['c%d_activation' % i]], packed=g['c%d_parameters' % i], yfunction=str(g['c%d_yfunction' % i]),
                kind=str(g['c%d_xkind' % i]), **{name: g['c%d_%s' % (i, name)] for name in ('xoffset', 'xscale', 'yoffset', 'yscale', 'Xq', 'Yq')})


def engine_state(cfg):
    """State of an MLPEmulatorEngine for a configuration of :func:`golden_config` (or a synthetic one with the same keys)."""
    yops = ([{'name': cfg['yfunction']}] if cfg['yfunction'] else []) + [{'name': cfg.get('kind', 'scale'), 'offset': cfg['yoffset'], 'scale': cfg['yscale']}]
    return {'name': 'mlp', 'nhidden': cfg['dims'][1:-1], 'activation': cfg['activations'], 'params': None, 'parameters': cfg['packed'], 'ndim': cfg['dims'][0],
            'M': cfg['dims'][-1], 'xoperations': [{'name': cfg.get('kind', 'scale'), 'offset': cfg['xoffset'], 'scale': cfg['xscale']}], 'yoperations': yops}
