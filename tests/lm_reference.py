"""Restatement of cp_lm_step and cp_spd_inverse (csrc/cp_lm.hip) for the tests (tests/test_lm_host.py, test_lm_step_gpu.py,
test_emulator_least_squares_gpu.py): the rules of include/cosmoprimo_amd.h in numpy, every operation in the kernel's order, in any floating-point type.
``np.longdouble`` is the truth, float64 the reference implementation that is not the code under test.

Tolerance rule: FLOOR, ALLOW and the block rule of tests/jacobian_reference.py (:func:`assert_within`): a block is one fit's ``next`` (or one fit's
inverse); its level is the distance of the float64 restatement from the longdouble truth over the block's largest entry, floored at 1.1e-16; the device is
allowed 16 levels.  Discrete results (status, naccepted, the held set, info) are compared exactly, lambda and the copied state bit for bit.

:func:`make_case` builds the batches of the device tests: fit b is of kind ``KINDS[b % len(KINDS)]``."""
import numpy as np

import jacobian_reference as jr

LD = np.longdouble
FLOOR, ALLOW = jr.FLOOR, jr.ALLOW
CONTROLS = dict(up=10., down=0.1, lmin=1e-12, lmax=1e12, ftol=1e-8)
STATE = ('x', 'fisher', 'gradient', 'chi2', 'lambda', 'status', 'naccepted')
TRIAL = ('x', 'fisher', 'gradient', 'chi2')


def factor(A, diag, held):
    """(L, bad) of the matrices A (B, n, n) (the triangle j <= i is read) with the diagonal ``diag`` (B, n) and the parameters ``held`` (B, n) taken out
    (row and column of the identity), in the type of A: columns in order, t_i = A[i][j] - sum_k L[i][k] L[j][k] with k ascending; bad: 0, or the 1-based
    column of the first pivot that is not > 0 or not finite."""
    B, n = diag.shape
    L = np.zeros_like(A)
    bad = np.zeros(B, dtype='i4')
    with np.errstate(all='ignore'):
        for j in range(n):
            t = A[:, :, j].copy()
            t[:, j] = diag[:, j]
            unit = np.zeros(n, dtype=A.dtype)
            unit[j] = 1
            t = np.where(held | held[:, j:j + 1], unit, t)
            for k in range(j):
                t = t - L[:, :, k] * L[:, j:j + 1, k]
            d = t[:, j]
            bad = np.where((bad == 0) & ~((d > 0) & np.isfinite(d)), j + 1, bad).astype('i4')
            r = np.sqrt(d)
            column = t / r[:, None]
            column[:, j] = r
            L[:, j:, j] = column[:, j:]
    return L, bad


def solve(L, r, first=0):
    """z of L L^T z = r (B, n), r zero before ``first``: forward with j ascending, back with j descending; valid from ``first`` on."""
    r = r.copy()
    n = r.shape[1]
    with np.errstate(all='ignore'):
        for j in range(first, n):
            y = r[:, j] / L[:, j, j]
            r[:, j] = y
            r[:, j + 1:] = r[:, j + 1:] - L[:, j + 1:, j] * y[:, None]
        for j in range(n - 1, first - 1, -1):
            z = r[:, j] / L[:, j, j]
            r[:, j] = z
            r[:, :j] = r[:, :j] - L[:, j, :j] * z[:, None]
    return r


def step(state, trial, lo, hi, dtype='f8', up=10., down=0.1, lmin=1e-12, lmax=1e12, ftol=1e-8):
    """One cp_lm_step in ``dtype``: ``(new state, next (B, ndim), held (B, ndim))``.  ``state`` and ``trial`` are dictionaries of float64 (and int32)
    arrays under the names of STATE and TRIAL, and are left as they are."""
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    x, F, g, chi, lam = (t(state[name]).copy() for name in STATE[:5])
    status, nacc = state['status'].copy(), state['naccepted'].copy()
    xt, Ft, gt, chit = (t(trial[name]) for name in TRIAL)
    lo, hi, up, down, lmin, lmax, ftol = (t(v) for v in (lo, hi, up, down, lmin, lmax, ftol))
    with np.errstate(all='ignore'):
        frozen = status != 0
        accept = ~frozen & np.isfinite(chit) & (chit <= chi)
        converged = accept & np.isfinite(chi) & (chi - chit <= ftol * chi)
        lower = lam * down
        lower = np.where(lower < lmin, lmin, lower)
        lam = np.where(accept & (nacc > 0), lower, lam)
        reject = ~frozen & ~accept
        failed = reject & (chi == np.inf)
        raised = lam * up
        stalled = reject & ~failed & (raised > lmax)
        lam = np.where(reject & ~failed, np.where(raised > lmax, lmax, raised), lam)
        status = np.where(converged, 1, np.where(failed, 3, np.where(stalled, 2, status))).astype('i4')
        nacc = (nacc + accept).astype('i4')
        x, g, chi = np.where(accept[:, None], xt, x), np.where(accept[:, None], gt, g), np.where(accept, chit, chi)
        F = np.where(accept[:, None, None], Ft, F)
        held = (status == 0)[:, None] & (((x >= hi) & (g > 0)) | ((x <= lo) & (g < 0)))
        fii = np.diagonal(F, axis1=1, axis2=2)
        L, bad = factor(F, fii + lam[:, None] * fii, held)
        status = np.where((status == 0) & (bad > 0), 3, status).astype('i4')
        delta = solve(L, np.where(held, 0, g))
        moved = x + delta
        moved = np.where(moved < lo, lo, moved)
        moved = np.where(moved > hi, hi, moved)
        nxt = np.where((status == 0)[:, None] & ~held, moved, x)
    new = dict(zip(STATE, (x, F, g, chi, lam, status, nacc)))
    return new, nxt, held


def spd_inverse(A, dtype='f8'):
    """(inverse (B, n, n), info (B,)) as cp_spd_inverse forms them, in ``dtype``."""
    A = np.asarray(A).astype(dtype)
    B, n = A.shape[:2]
    L, bad = factor(A, np.diagonal(A, axis1=1, axis2=2).copy(), np.zeros((B, n), dtype='?'))
    inv = np.empty_like(A)
    for c in range(n):
        unit = np.zeros((B, n), dtype=A.dtype)
        unit[:, c] = 1
        z = solve(L, unit, first=c)
        inv[:, c:, c] = z[:, c:]
        inv[:, c, c:] = z[:, c:]
    inv[bad > 0] = np.nan
    return inv, bad


def assert_within(dev, truth, restated, what=''):
    """Blocks along the first axis (one fit each): the rule of tests/jacobian_reference.py on (B, ...) arrays."""
    B = len(truth)
    flat = lambda a: np.asarray(a).reshape(B, -1).T      # noqa: E731
    jr.assert_within(flat(dev), flat(truth), flat(restated), what)


def worst_level(truth, restated):
    """The largest level over the blocks, in floors."""
    B = len(truth)
    return float(jr.levels(np.asarray(truth).reshape(B, -1).T, np.asarray(restated).reshape(B, -1).T)[1].max() / FLOOR)


NDIMS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)
KINDS = ('half', 'equal', 'worse', 'nan', 'inf', 'first', 'first-bad', 'lmax', 'terminal', 'bounds', 'zero-diagonal', 'indefinite', 'ill', 'ftol')


def lanes(ndim):
    """(lanes per fit, fits per wave, fits per workgroup) by the stated rule: the smallest power of two >= ndim; four waves a workgroup, two at 32 lanes."""
    G = 1
    while G < ndim:
        G *= 2
    return G, 64 // G, (128 if G == 32 else 256) // G


def batch_sizes(ndim):
    """One below, at and one above the fits per wave and per workgroup, and three workgroups + 2."""
    G, per_wave, per_workgroup = lanes(ndim)
    sizes = {per_wave - 1, per_wave, per_wave + 1, per_workgroup - 1, per_workgroup, per_workgroup + 1, 3 * per_workgroup + 2}
    return sorted(size for size in sizes if size > 0)


def spd(rng, n, scales=True):
    """A random J W J^T with n + 8 columns, its parameters on scales over two decades."""
    J = rng.standard_normal((n, n + 8))
    F = (J * 10.**rng.uniform(-1., 1., n + 8)) @ J.T
    s = 10.**rng.uniform(-1., 1., n) if scales else np.ones(n)
    F = F * s[:, None] * s[None, :]
    return (F + F.T) / 2.


def ill_conditioned(rng, n, condition=1e10):
    """Unit diagonal up to rounding is not asked for: eigenvalues from 1 down to 1 / condition in a random basis."""
    Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
    F = (Q * np.geomspace(1., 1. / condition, n)) @ Q.T
    return (F + F.T) / 2.


def make_case(ndim, B, seed=0):
    """(state, trial, lo, hi, kinds) of a batch of B fits of ndim parameters, fit b of kind ``KINDS[(b + seed) % len(KINDS)]``:
    half / equal / worse: the trial's chi2 at 0.5 x, exactly 1 x (converged) and 1.5 x the state's; nan / inf: such a trial chi2; first / first-bad: a state
    chi2 of +inf with a finite and with a NaN trial; lmax: a rejection that takes lambda beyond lmax; terminal: a status of 1, 2 or 3 already; bounds: an
    accepted trial that sits on hi with the gradient pointing out (held), on lo with it pointing in (free), on lo pointing out and on hi pointing in (as far
    as ndim gives parameters); zero-diagonal: a parameter nothing depends on; indefinite: the last diagonal entry negated; ill: a rejected trial on a state
    matrix of condition number 1e10 with lambda = 1e-11; ftol: a decrease of 1e-10 of chi2 (converged)."""
    rng = np.random.default_rng(1000 * ndim + 7 * B + seed)
    n = ndim
    lo, hi = -1. - rng.uniform(0., 1., n), 1. + rng.uniform(0., 1., n)
    if n >= 3:
        lo[2], hi[2] = -np.inf, np.inf
    width = np.where(np.isfinite(hi - lo), hi - lo, 2.)
    state = dict(x=rng.uniform(-0.5, 0.5, (B, n)), fisher=np.empty((B, n, n)), gradient=np.empty((B, n)), chi2=10.**rng.uniform(0., 2., B),
                 status=np.zeros(B, dtype='i4'), naccepted=rng.integers(1, 6, B).astype('i4'))
    state['lambda'] = 10.**rng.uniform(-4., -1., B)
    trial = dict(x=rng.uniform(-0.5, 0.5, (B, n)), fisher=np.empty((B, n, n)), gradient=np.empty((B, n)), chi2=np.empty(B))
    kinds = [KINDS[(b + seed) % len(KINDS)] for b in range(B)]
    for b, kind in enumerate(kinds):
        for d in (state, trial):
            d['fisher'][b] = spd(rng, n)
            d['gradient'][b] = d['fisher'][b] @ (rng.uniform(-0.2, 0.2, n) * width)
        ratio = {'half': 0.5, 'equal': 1., 'worse': 1.5, 'nan': np.nan, 'inf': np.inf, 'first-bad': np.nan, 'ftol': 1. - 1e-10, 'ill': 1.5, 'lmax': 2.}.get(kind, 0.75)
        trial['chi2'][b] = state['chi2'][b] * ratio
        which = (b // len(KINDS)) % n
        if kind in ('first', 'first-bad'):
            state['chi2'][b], state['naccepted'][b] = np.inf, 0
            trial['chi2'][b] = 3.5 if kind == 'first' else np.nan
        elif kind == 'lmax':
            state['lambda'][b] = 0.5e12
        elif kind == 'terminal':
            state['status'][b] = 1 + (b // len(KINDS)) % 3
        elif kind == 'bounds':
            finite = [i for i in range(n) if np.isfinite(lo[i])]
            for i, (side, sign) in zip(finite, ((hi, 1.), (lo, 1.), (lo, -1.), (hi, -1.))):
                trial['x'][b, i] = side[i]
                trial['gradient'][b, i] = sign * abs(trial['gradient'][b, i])
        elif kind == 'zero-diagonal':
            trial['fisher'][b, which, :] = trial['fisher'][b, :, which] = 0.
        elif kind == 'indefinite':
            trial['fisher'][b, n - 1, n - 1] *= -1.
        elif kind == 'ill':
            state['fisher'][b] = ill_conditioned(rng, n)
            state['gradient'][b] = state['fisher'][b] @ (rng.uniform(-0.2, 0.2, n) * width)
            state['lambda'][b] = 1e-12
    return state, trial, lo, hi, kinds


def make_matrices(ndim, B, seed=0):
    """(B, ndim, ndim) for cp_spd_inverse: random J W J^T, every fifth ill-conditioned (1e6), fit 1 (where there is one) with a failing pivot -- a zero row
    and column, or the last diagonal entry negated -- and its index."""
    rng = np.random.default_rng(2000 * ndim + 7 * B + seed)
    A = np.stack([ill_conditioned(rng, ndim, 1e6) if b % 5 == 4 else spd(rng, ndim) for b in range(B)])
    failing = {}
    for b in range(1, B, 7):
        if (b // 7) % 2:
            which = (b // 7) % ndim
            A[b, which, :] = A[b, :, which] = 0.
            failing[b] = which + 1
        else:
            A[b, ndim - 1, ndim - 1] *= -1.
            failing[b] = ndim
    return A, failing
