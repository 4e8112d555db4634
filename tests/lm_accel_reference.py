"""Restatement of cp_lm_step_velocity and cp_lm_accelerate (csrc/cp_lm.hip) for the tests (tests/test_lm_accel_host.py, test_lm_accel_gpu.py,
test_emulator_geodesic_gpu.py): the rules of include/cosmoprimo_amd.h in numpy on top of tests/lm_reference.py (``factor``, ``solve``, ``step``), every
operation in the kernel's order, in any floating-point type.  ``np.longdouble`` is the truth, float64 the reference implementation that is not the code
under test.

Tolerance rule: that of tests/lm_reference.py (a block is one fit's ``next`` or ``velocity``; 16 levels, floor 1.1e-16).  The discrete results -- the set
of fits that take the correction, the counter, the held set -- are compared exactly: :func:`make_case` draws ``h`` so that the gate
``4 sa <= alpha^2 sv`` is nowhere within a factor 1.25 of equality, in float64 and in longdouble (checked by :func:`gate_ratio` in the host test).

:func:`make_case` builds the batches of the device tests: fit b is of kind ``KINDS[b % len(KINDS)]``."""
import numpy as np

import lm_reference as lr

LD = np.longdouble
ALPHA = 0.75
KINDS = ('pass', 'refuse', 'zero-h', 'nan-h', 'inf-h', 'zero-v', 'terminal', 'bounds', 'cross', 'pivot', 'ill')
ACCEL = ('x', 'fisher', 'gradient', 'lambda', 'status')      # what cp_lm_accelerate reads of the state


def _system(state, lo, hi, dtype):
    """(x, g, status, held, fii, L, bad) of the state as cp_lm_step left it: the held set by its rule, the factor of F + lambda diag F with it taken out."""
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    x, F, g, lam = (t(state[name]) for name in ('x', 'fisher', 'gradient', 'lambda'))
    status = np.asarray(state['status'])
    lo, hi = t(lo), t(hi)
    with np.errstate(all='ignore'):
        held = (status == 0)[:, None] & (((x >= hi) & (g > 0)) | ((x <= lo) & (g < 0)))
        fii = np.diagonal(F, axis1=1, axis2=2).copy()
        L, bad = lr.factor(F, fii + lam[:, None] * fii, held)
    return x, g, status, held, fii, L, bad


def velocity(state, lo, hi, dtype='f8'):
    """What cp_lm_step_velocity writes beside ``next``, from the state it leaves (a failed pivot is a status of 3 there): delta on the free parameters of a
    running fit, exact 0 elsewhere."""
    x, g, status, held, fii, L, bad = _system(state, lo, hi, dtype)
    with np.errstate(all='ignore'):
        delta = lr.solve(L, np.where(held, 0, g))
    return np.where(((status == 0) & (bad == 0))[:, None] & ~held, delta, np.zeros_like(delta))


def step_velocity(state, trial, lo, hi, dtype='f8', **controls):
    """One cp_lm_step_velocity in ``dtype``: ``(new state, next, held, velocity)``, the first three those of ``lm_reference.step``."""
    new, nxt, held = lr.step(state, trial, lo, hi, dtype=dtype, **controls)
    return new, nxt, held, velocity(new, lo, hi, dtype)


def _gate(state, v, h, lo, hi, alpha, dtype):
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    x, g, status, held, fii, L, bad = _system(state, lo, hi, dtype)
    v, h, alpha = t(v), t(h), t(alpha)
    with np.errstate(all='ignore'):
        a = lr.solve(L, np.where(held, 0, -h))
        ta, tv = (fii * a) * a, (fii * v) * v
        sa, sv = np.zeros(len(x), dtype=dtype), np.zeros(len(x), dtype=dtype)
        for i in range(x.shape[1]):      # over the free parameters, ascending
            sa, sv = np.where(held[:, i], sa, sa + ta[:, i]), np.where(held[:, i], sv, sv + tv[:, i])
        running = (status == 0) & (bad == 0)
        take = running & (sv > 0) & np.isfinite(sa) & (4 * sa <= (alpha * alpha) * sv)
    return x, held, running, a, sa, sv, take


def gate_ratio(state, v, h, lo, hi, alpha=ALPHA, dtype='f8'):
    """``4 sa / (alpha^2 sv)`` (B,) of the running fits with sv > 0 (NaN elsewhere): the gate takes the correction where it is finite and <= 1."""
    x, held, running, a, sa, sv, take = _gate(state, v, h, lo, hi, alpha, dtype)
    alpha = np.asarray(alpha).astype(dtype)
    with np.errstate(all='ignore'):
        return np.where(running & (sv > 0), 4 * sa / ((alpha * alpha) * sv), np.nan)


def accelerate(state, v, h, lo, hi, alpha=ALPHA, dtype='f8', sign=1.):
    """One cp_lm_accelerate in ``dtype``: ``(next (B, ndim), taken (B,) bool)``; the counter goes up by ``taken``.  ``state``, ``v``, ``h``: float64 (and int32)
    arrays, left as they are.  ``sign=-1``: the acceleration with the wrong sign (for the test that tells the rule from a wrong one)."""
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    x, held, running, a, sa, sv, take = _gate(state, v, h, lo, hi, alpha, dtype)
    v, lo, hi = t(v), t(lo), t(hi)
    with np.errstate(all='ignore'):
        half = t(0.5) * a
        moved = x + np.where(take[:, None], v + (half if sign > 0 else -half), v)
        moved = np.where(moved < lo, lo, moved)
        moved = np.where(moved > hi, hi, moved)
        nxt = np.where(running[:, None] & ~held, moved, x)
    return nxt, take


def make_case(ndim, B, seed=0, alpha=ALPHA):
    """(state, velocity, h, lo, hi, kinds) of a batch of B fits of ndim parameters, the state as cp_lm_step leaves it (running fits between two of its
    calls), ``velocity`` the float64 restatement's, fit b of kind ``KINDS[(b + seed) % len(KINDS)]``:
    pass / refuse: ``h`` drawn so that ``4 sa / (alpha^2 sv)`` is 0.3 and 3 (``h`` scaled up); zero-h: ``h = 0`` (the correction is taken and changes
    nothing); nan-h / inf-h: such an entry in ``h`` (refused); zero-v: a zero gradient, ``v = 0`` (refused: sv = 0); terminal: a status of 1, 2 or 3;
    bounds: a parameter on hi with the gradient pointing out (held; its ``h`` is arbitrary), one on lo with it pointing in (free), the gate passes;
    cross: the gate passes and the corrected step of parameter 0 goes twice as far as its bound is (clipped to it exactly); pivot: the last diagonal entry
    negated, status still 0; ill: a matrix of condition number 1e10 with lambda = 1e-12, the gate passes."""
    rng = np.random.default_rng(3000 * ndim + 7 * B + seed)
    n = ndim
    lo, hi = -1. - rng.uniform(0., 1., n), 1. + rng.uniform(0., 1., n)
    if n >= 3:
        lo[2], hi[2] = -np.inf, np.inf
    width = np.where(np.isfinite(hi - lo), hi - lo, 2.)
    state = dict(x=rng.uniform(-0.5, 0.5, (B, n)), fisher=np.empty((B, n, n)), gradient=np.empty((B, n)), status=np.zeros(B, dtype='i4'))
    state['lambda'] = 10.**rng.uniform(-4., -1., B)
    kinds = [KINDS[(b + seed) % len(KINDS)] for b in range(B)]
    for b, kind in enumerate(kinds):
        state['fisher'][b] = lr.ill_conditioned(rng, n) if kind == 'ill' else lr.spd(rng, n)
        state['gradient'][b] = state['fisher'][b] @ (rng.uniform(-0.02, 0.02, n) * width)
        if kind == 'ill':
            state['lambda'][b] = 1e-12
        elif kind == 'zero-v':
            state['gradient'][b] = 0.
        elif kind == 'terminal':
            state['status'][b] = 1 + (b // len(KINDS)) % 3
        elif kind == 'bounds':
            finite = [i for i in range(n) if np.isfinite(lo[i])]
            for i, side in zip(finite, (hi, lo)):
                state['x'][b, i] = side[i]
                state['gradient'][b, i] = abs(state['gradient'][b, i])
    # h = -A (c d): the acceleration is c d on the free parameters, c from the ratio the kind asks for
    v = velocity(state, lo, hi, 'f8')
    held = (state['status'] == 0)[:, None] & (((state['x'] >= hi) & (state['gradient'] > 0)) | ((state['x'] <= lo) & (state['gradient'] < 0)))
    h = np.zeros((B, n))
    for b, kind in enumerate(kinds):
        F = state['fisher'][b]
        fii = np.diag(F).copy()
        d = np.where(held[b], 0., rng.standard_normal(n) / np.sqrt(fii))
        sv, sd = (fii * v[b]**2).sum(), (fii * d**2).sum()
        ratio = {'refuse': 3., 'zero-h': 0.}.get(kind, 0.3)
        c = alpha * np.sqrt(ratio * sv / (4. * sd)) if sv > 0 else 1.
        A = F + np.diag(state['lambda'][b] * fii)
        h[b] = -(A @ (c * d))
        h[b, held[b]] = rng.standard_normal(int(held[b].sum()))
        which = (b // len(KINDS)) % n
        if kind == 'nan-h':
            h[b, which] = np.nan
        elif kind == 'inf-h':
            h[b, which] = np.inf if b % 2 else -np.inf
        elif kind == 'cross':
            move = v[b, 0] + 0.5 * c * d[0]
            state['x'][b, 0] = hi[0] - 0.5 * move if move > 0 else lo[0] - 0.5 * move
    for b, kind in enumerate(kinds):
        if kind == 'pivot':
            state['fisher'][b, n - 1, n - 1] *= -1.
            v[b] = rng.uniform(-0.1, 0.1, n)      # (what a caller would not have: the step itself fails this fit)
    return state, v, h, lo, hi, kinds


def rosenbrock(x):
    """(fisher, gradient, chi2, curvature(v)) of Rosenbrock's valley as two residuals, y = (10 (x1 - x0^2), x0) against the data (0, 1) with unit weights, at
    the points x (B, 2), in the type of x: what gauss_newton returns there, and h = J y''(v, v)."""
    one = np.ones_like(x[:, 0])
    J = np.stack([np.stack([-20 * x[:, 0], one], axis=1), np.stack([10 * one, 0 * one], axis=1)], axis=1)      # (B, parameter, output)
    r = np.stack([-10 * (x[:, 1] - x[:, 0]**2), 1 - x[:, 0]], axis=1)
    fisher, gradient, chi2 = np.einsum('bic,bjc->bij', J, J), np.einsum('bic,bc->bi', J, r), (r * r).sum(axis=1)

    def curvature(v):
        q = np.stack([-20 * v[:, 0]**2, 0 * v[:, 0]], axis=1)
        return np.einsum('bic,bc->bi', J, q)

    return fisher, gradient, chi2, curvature


def fit_rosenbrock(geodesic, sign=1., start=(-1.2, 1.), alpha=ALPHA, lambda0=1e-3, most=500, dtype='f8'):
    """The loop of Emulator.least_squares restated on :func:`rosenbrock`, with an open box and the default controls: ``(evaluations until status is 1 (or
    ``most``), final x, naccelerated)``."""
    big = np.full(2, np.inf)
    x = np.array([start], dtype='f8')
    state = dict(x=x.copy(), fisher=np.zeros((1, 2, 2)), gradient=np.zeros((1, 2)), chi2=np.full(1, np.inf), status=np.zeros(1, dtype='i4'), naccepted=np.zeros(1, dtype='i4'))
    state['lambda'] = np.full(1, lambda0)
    count = 0
    for evaluation in range(1, most + 1):
        fisher, gradient, chi2, curvature = rosenbrock(x)
        trial = dict(x=x, fisher=fisher, gradient=gradient, chi2=chi2)
        state, x, held, v = step_velocity(state, trial, -big, big, dtype=dtype, **lr.CONTROLS)
        state = {name: np.asarray(value, dtype='i4' if name in ('status', 'naccepted') else 'f8') for name, value in state.items()}
        x, v = np.asarray(x, dtype='f8'), np.asarray(v, dtype='f8')
        if state['status'][0] != 0:
            return evaluation, state['x'][0], count
        if geodesic:
            h = rosenbrock(state['x'])[3](v)
            x, taken = accelerate(state, v, h, -big, big, alpha=alpha, dtype=dtype, sign=sign)
            x = np.asarray(x, dtype='f8')
            count += int(taken[0])
    return most, state['x'][0], count
