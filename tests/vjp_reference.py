"""Restatement of the emulators' vector-Jacobian products for the tests (tests/test_vjp_host.py, test_mlp_vjp_gpu.py, test_taylor_vjp_gpu.py,
test_emulator_vjp_gpu.py): the reverse pass of the MLP on top of tests/mlp_reference.py and of the Taylor polynomial, in any floating-point type.
``np.longdouble`` is the truth, float64 the reference implementation that is not the code under test.

Tolerance rule.  G[b, i] = sum_c cot[b, c] d predict[b, c] / d x[b, i] is a sum with cancellation, and the Jacobian's rule (a
multiple of one float64 pass's distance from the truth per block) does not transfer: another float64 summation order lies up to 7.7 x that allowance
away, one pass's chance error being no measure of another order's.  The yardstick is the MAGNITUDE PASS A[b, i]: the same reverse pass in longdouble with
every factor replaced by its absolute value (|cot yscale f'|, |W|, |act'|, 1 / |xscale|; Taylor: sum_t |d mono_t / d x_i| sum_c |cot| |D|), which is what the
rounding errors of any order scale with.  Per entry, no case left out:

    |G_dev - G_ld| <= 16 level 2^-53 A[b, i],     level = max(1, largest error / (2^-53 A) over three float64 orders)

the orders being the reverse pass, ``cot`` contracted with the forward-mode Jacobian of tests/jacobian_reference.py, and the reverse pass with the
outputs summed in a permuted order in chunks of 40, all measured in the test for that very case.  16 is the project's margin (another summation order,
MFMA steps of 4, the device's own exp); the floor of 1 keeps a lucky float64 pass from forbidding rounding.  Measured on the CPU with weights from
N(0, 0.4): level at most 9 (log10), 3.9 (arcsinh), 2.5 (no y function); tests/test_vjp_host.py holds it to 32 for every shape the device tests use."""
import numpy as np

import jacobian_reference as jr
import mlp_reference as mr

LD = np.longdouble
EPS = 2.**-53
ALLOW = 16.
CHUNK = 40


def draw_network(rng, dims, yfunction=''):
    """Packed weights for the vjp tests: kernels and biases N(0, 0.4^2) (saturated tanh under wider weights makes 1 - t^2 lose its relative accuracy), the
    output kernel and bias x 0.1 under a y function (the prediction 10^v stays within a few decades), alpha and beta in (0.3, 1.2)."""
    packed = np.zeros(mr.nparams(dims))
    last = len(dims) - 2
    for name, sl in mr.blocks(dims).items():
        if name.startswith('alphabeta'):
            packed[sl] = rng.uniform(0.3, 1.2, 2)
        else:
            packed[sl] = rng.normal(0., 0.4, sl.stop - sl.start) * (0.1 if yfunction and int(name[-1]) == last else 1.)
    return packed


def _weighted_cotangent(layers, activations, X, xoffset, xscale, yoffset, yscale, yfunction, cot, dtype, magnitude):
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    zs, hs, out = mr.forward(layers, activations, (t(X) - t(xoffset)) / t(xscale))
    v = out * t(yscale) + t(yoffset)
    w = t(cot) * t(yscale)
    if yfunction == 'log10':
        w = w * (np.log(np.asarray(10, dtype=dtype)) * 10**v)
    elif yfunction == 'arcsinh':
        w = w * np.cosh(v)
    return zs, (np.abs(w) if magnitude else w)


def _walk_back(layers, activations, zs, dh, xscale, dtype, magnitude):
    mag = np.abs if magnitude else (lambda a: a)
    for l in range(len(layers) - 2, -1, -1):
        kernel, bias, alpha, beta = layers[l]
        dz = dh * mag(jr.activate_derivative(activations[l], zs[l], alpha, beta))
        dh = dz @ mag(kernel).T
    return dh / mag(np.broadcast_to(np.asarray(xscale).astype(dtype), (dh.shape[1],)))


def mlp_vjp(packed, dims, activations, X, xoffset, xscale, yoffset, yscale, yfunction, cot, dtype='f8', magnitude=False, permutation=None):
    """G (B, ndim) of the engine's prediction by reverse mode in ``dtype``.  ``magnitude``: every factor replaced by its absolute value (the module
    docstring's A).  ``permutation`` of the M outputs: the product with the transposed output kernel summed in that order, in chunks of CHUNK."""
    layers = mr.unpack(packed, dims, dtype)
    zs, w = _weighted_cotangent(layers, activations, X, xoffset, xscale, yoffset, yscale, yfunction, cot, dtype, magnitude)
    Wout = np.abs(layers[-1][0]) if magnitude else layers[-1][0]
    if permutation is None:
        dh = w @ Wout.T
    else:
        dh = np.zeros((len(w), Wout.shape[0]), dtype=dtype)
        for a in range(0, len(permutation), CHUNK):
            idx = permutation[a:a + CHUNK]
            dh = dh + w[:, idx] @ Wout[:, idx].T
    return _walk_back(layers, activations, zs, dh, xscale, dtype, magnitude)


def mlp_case(cfg, cot, columns=None):
    """(G_ld, A, level) of a configuration (keys of tests/test_mlp_jacobian_gpu.py ``config``) and a cotangent (B, M), zero outside ``columns``: the truth,
    the magnitude pass, and the level of the rule measured over the three float64 orders."""
    args = (cfg['packed'], cfg['dims'], cfg['activations'], cfg['X'], cfg['xoffset'], cfg['xscale'], cfg['yoffset'], cfg['yscale'], cfg['yfunction'])
    cot = np.asarray(cot, dtype='f8')
    if columns is not None:
        full = np.zeros((len(cot), cfg['dims'][-1]))
        full[:, columns[0]:columns[1]] = cot
        cot = full
    G_ld = mlp_vjp(*args, cot, dtype=LD)
    A = mlp_vjp(*args, cot, dtype=LD, magnitude=True)
    perm = np.random.default_rng(cot.shape[1]).permutation(cot.shape[1])
    orders = [mlp_vjp(*args, cot), np.einsum('bc,bic->bi', cot, jr.mlp_jacobian(*args, dtype='f8')[1]), mlp_vjp(*args, cot, permutation=perm)]
    return G_ld, A, level_of(orders, G_ld, A)


def level_of(orders, G_ld, A):
    worst = 0.
    for G in orders:
        dist = np.abs(np.asarray(G).astype(LD) - G_ld)
        with np.errstate(divide='ignore', invalid='ignore'):
            used = np.where(A > 0, dist / (EPS * A), np.where(dist > 0, np.inf, 0))
        worst = max(worst, float(used.max()))
    return max(1., worst)


def taylor_vjp(center, powers, derivatives, X, cot, dtype='f8', magnitude=False, permutation=None):
    """G (B, ndim) of the polynomial in ``dtype``: S = cot . D^T, then its contraction with the derivatives of the monomials."""
    left = jr.taylor_left(center, powers, X, dtype)      # (B, ndim, T)
    D, cot = np.asarray(derivatives).astype(dtype), np.asarray(cot).astype(dtype)
    if magnitude:
        left, D, cot = np.abs(left), np.abs(D), np.abs(cot)
    if permutation is None:
        S = cot @ D.T
    else:
        S = np.zeros((len(cot), len(D)), dtype=dtype)
        for a in range(0, len(permutation), CHUNK):
            idx = permutation[a:a + CHUNK]
            S = S + cot[:, idx] @ D[:, idx].T
    return np.einsum('bit,bt->bi', left, S)


def taylor_case(c, cot, columns=None):
    """(G_ld, A, level) of a Taylor case (center, powers, derivatives, X) and a cotangent (B, M), zero outside ``columns``."""
    args = (c['center'], c['powers'], c['derivatives'], c['X'])
    cot = np.asarray(cot, dtype='f8')
    if columns is not None:
        full = np.zeros((len(cot), np.shape(c['derivatives'])[1]))
        full[:, columns[0]:columns[1]] = cot
        cot = full
    G_ld = taylor_vjp(*args, cot, dtype=LD)
    A = taylor_vjp(*args, cot, dtype=LD, magnitude=True)
    perm = np.random.default_rng(cot.shape[1]).permutation(cot.shape[1])
    orders = [taylor_vjp(*args, cot), np.einsum('bc,bic->bi', cot, jr.taylor_jacobian(*args, dtype='f8')), taylor_vjp(*args, cot, permutation=perm)]
    return G_ld, A, level_of(orders, G_ld, A)


def assert_within(G_dev, G_ld, A, level, what='', extra=0.):
    """Every entry of the device's G within ALLOW x level x 2^-53 A (plus ``extra``, absolute, per entry) of the truth; prints and returns the largest
    fraction of the allowance used."""
    G_dev = np.asarray(G_dev)
    dist = np.abs(G_dev.astype(LD) - G_ld)
    allowed = ALLOW * level * EPS * A + extra
    with np.errstate(divide='ignore', invalid='ignore'):
        fraction = np.where(allowed > 0, dist / allowed, np.where(dist > 0, np.inf, 0))
    worst = float(fraction.max()) if fraction.size else 0.
    print('%s: largest fraction of the allowance %.3g (level %.3g)' % (what, worst, level))
    assert np.isfinite(G_dev).all(), what
    assert worst <= 1., '{}: entry {} at {:.3g} of its allowance'.format(what, np.unravel_index(np.argmax(fraction), fraction.shape), worst)
    return worst


def mlp_config(B=65, ndim=3, widths=(5, 17), M=257, activations='silu', yfunction='', seed=0):
    """A synthetic engine with the weights of :func:`draw_network`, points in its unit box, and a cotangent (B, M) from N(0, 1)."""
    rng = np.random.default_rng(1000 * B + 100 * ndim + 10 * sum(widths) + M + seed)
    dims = (ndim,) + tuple(widths) + (M,)
    activations = [activations] * len(widths) if isinstance(activations, str) else list(activations)
    lo, xscale = rng.uniform(-1., 1., ndim), rng.uniform(0.5, 2., ndim)
    cfg = dict(dims=dims, activations=activations, packed=draw_network(rng, dims, yfunction), yfunction=yfunction, xoffset=lo, xscale=xscale,
               yoffset=rng.normal(0., 1., M), yscale=rng.uniform(0.5, 2., M))
    cfg['X'] = lo + xscale * rng.uniform(0., 1., (B, ndim))
    cfg['cot'] = rng.normal(0., 1., (B, M))
    return cfg


# one dimension at a time around B = 65, ndim = 3, widths (5, 17), M = 257 (tests/test_mlp_vjp_gpu.py says why these values)
MLP_CASES = ([dict()] + [dict(B=B) for B in (1, 63, 64, 129)] + [dict(ndim=n) for n in (1, 2, 8, 32)] + [dict(widths=(5, w)) for w in (1, 16, 33, 49, 64)]
             + [dict(widths=(w, 17)) for w in (33, 64)] + [dict(M=M) for M in (1, 8, 9, 65, 1025)] + [dict(widths=(17,)), dict(widths=(16,) * 8, activations='tanh')]
             + [dict(activations=a) for a in ('relu', 'tanh', 'identity-silu')] + [dict(activations=['identity-silu', 'relu', 'tanh', 'silu'], widths=(9, 12, 7, 17))]
             + [dict(yfunction=y) for y in ('log10', 'arcsinh')] + [dict(yfunction='log10', activations='identity-silu', widths=(33, 64))])
MLP_RANGES = ((1, 2), (3, 200), (256, 257))


def taylor_config(B=65, ndim=3, T=65, M=257):
    """The polynomial of tests/test_taylor_jacobian_gpu.py ``config`` (powers from {0, 1, 2, 3}, one term at power 15, term 0 the constant) and a cotangent."""
    rng = np.random.default_rng(1000 * B + 100 * ndim + 10 * T + M)
    powers = rng.integers(0, 4, (T, ndim)).astype('i4')
    powers[0] = 0
    if T > 1:
        powers[T // 2, rng.integers(ndim)] = 15
    return dict(center=rng.uniform(-0.5, 0.5, ndim), powers=powers, derivatives=rng.normal(0., 1., (T, M)), X=rng.uniform(-1., 1., (B, ndim)),
                cot=rng.normal(0., 1., (B, M)))


TAYLOR_CASES = ([dict()] + [dict(B=B) for B in (1, 64)] + [dict(ndim=n) for n in (1, 32)] + [dict(T=T) for T in (1, 32, 33, 64, 257)] + [dict(M=M) for M in (1, 4, 5)])


def case_id(case):
    return '-'.join('%s=%s' % item for item in case.items()).replace(' ', '') or 'base'
