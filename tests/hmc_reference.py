"""Restatement of cp_hmc_factor and cp_hmc_step (csrc/cp_hmc.hip) for the tests (tests/test_hmc_host.py, test_hmc_step_gpu.py,
test_emulator_hmc_gpu.py): Philox4x32-10, the uniforms and every rule of include/cosmoprimo_amd.h in numpy, every operation in the kernel's order, in any
floating-point type.  ``np.longdouble`` is the truth, float64 the reference implementation that is not the code under test.  The factorisation is
``lm_reference.factor``; the forward and the back substitution here are the two halves of ``lm_reference.solve`` (tests/test_hmc_host.py compares them).

Tolerance rule: FLOOR, ALLOW and the block rule of tests/jacobian_reference.py (:func:`assert_levels`): a block is one chain's ``z``, ``next`` or ``sample``
(or its ``h0``, its ``eps``); its level is the distance of the float64 restatement from the longdouble truth over the block's largest entry, floored at
1.1e-16; the device is allowed 16 levels.  A NaN (a chain fed a NaN gradient) must be a NaN in all three.  Discrete results (accept, ``out``, ``status``,
``naccepted``, ``nout``) are compared exactly, the state copied on acceptance and a frozen chain's buffers bit for bit.

:func:`make_case` builds the batches of the device tests: chain b is of kind ``KINDS[(b + seed) % len(KINDS)]``.  :func:`run` is ``Emulator.hmc``'s loop on any
``evaluate(x) -> (fisher, gradient, chi2)``; :class:`LinearModel` is such a function with a known Gaussian posterior."""
import numpy as np

import jacobian_reference as jr
import lm_reference as lr

LD = np.longdouble
FLOOR, ALLOW = jr.FLOOR, jr.ALLOW
STATE = ('x', 'gradient', 'chi2', 'status', 'naccepted', 'nout')
TRAJECTORY = ('z', 'h0', 'eps', 'out')
TRIAL = ('x', 'gradient', 'chi2')
INTEGERS = ('status', 'naccepted', 'nout', 'out')
NDIMS = lr.NDIMS
lanes = lr.lanes

M0, M1, W0, W1 = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85))
MASK = np.uint64(0xffffffff)
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(counter, key):
    """The four output words (uint64 arrays holding 32-bit values) of Philox4x32-10 for the counter words ``counter`` (four arrays or numbers) and ``key``."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter]))
    k0, k1 = (np.uint64(k) & MASK for k in key)
    for r in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniform(wa, wb, dtype='f8'):
    """min(((wa >> 5) 2^26 + (wb >> 6) + 0.5) 2^-53, 1 - 2^-53) in ``dtype``, every operation rounded once: strictly inside (0, 1).  (In float64 the sum
    with 0.5 is rounded; for the largest 53-bit integer alone it comes to 2^53, which the minimum takes back.)"""
    t = np.dtype(dtype).type
    k = (np.asarray(wa, dtype=np.uint64) >> np.uint64(5)).astype(dtype) * t(67108864.) + (np.asarray(wb, dtype=np.uint64) >> np.uint64(6)).astype(dtype)
    u = (k + t(0.5)) * t(2.)**-53
    return np.minimum(u, t(1.) - t(2.)**-53)


def words(seed, b, t, slot):
    seed = int(seed) & 0xffffffffffffffff
    b = np.asarray(b, dtype=np.uint64)
    return philox((b & MASK, b >> np.uint64(32), np.uint64(t), np.uint64(slot)), (seed & 0xffffffff, seed >> 32))


def normals(seed, b, t, ndim, dtype='f8'):
    """z (B, ndim) of trajectory ``t`` for the chains ``b``: slot s gives parameters 2 s and 2 s + 1."""
    ty = np.dtype(dtype).type
    z = np.empty((len(b), ndim), dtype=dtype)
    for s in range((ndim + 1) // 2):
        w = words(seed, b, t, s)
        r = np.sqrt(ty(-2.) * np.log(uniform(w[0], w[1], dtype)))
        angle = ty(6.283185307179586) * uniform(w[2], w[3], dtype)
        z[:, 2 * s] = r * np.cos(angle)
        if 2 * s + 1 < ndim:
            z[:, 2 * s + 1] = r * np.sin(angle)
    return z


def jitter_and_energy(seed, b, t, dtype='f8'):
    """(u_j, e) of slot 16 of trajectory ``t``."""
    w = words(seed, b, t, 16)
    return uniform(w[0], w[1], dtype), -np.log(uniform(w[2], w[3], dtype))


def factor(metric, status, dtype='f8'):
    """(L, status) as cp_hmc_factor leaves them: L of ``metric`` (B, n, n) in ``dtype`` with a zero strict upper triangle (meaningless where a pivot fails),
    status 3 there."""
    A = np.asarray(metric).astype(dtype)
    B, n = A.shape[:2]
    L, bad = lr.factor(A, np.diagonal(A, axis1=1, axis2=2).copy(), np.zeros((B, n), dtype='?'))
    return L, np.where(bad > 0, 3, status).astype('i4')


def forward(L, r):
    """y of L y = r (B, n): j ascending (the first half of ``lm_reference.solve``)."""
    r = r.copy()
    n = r.shape[1]
    with np.errstate(all='ignore'):
        for j in range(n):
            y = r[:, j] / L[:, j, j]
            r[:, j] = y
            r[:, j + 1:] = r[:, j + 1:] - L[:, j + 1:, j] * y[:, None]
    return r


def backward(L, r):
    """z of L^T z = r (B, n): j descending (the second half of ``lm_reference.solve``)."""
    r = r.copy()
    n = r.shape[1]
    with np.errstate(all='ignore'):
        for j in range(n - 1, -1, -1):
            z = r[:, j] / L[:, j, j]
            r[:, j] = z
            r[:, :j] = r[:, :j] - L[:, j, :j] * z[:, None]
    return r


def squares(z):
    """sum_i z_i z_i, i ascending, from 0."""
    s = np.zeros(len(z), dtype=z.dtype)
    for i in range(z.shape[1]):
        s = s + z[:, i] * z[:, i]
    return s


def step(state, trial, L, lo, hi, step_size, t_close=None, t_open=None, jitter=0.1, seed=0, dtype='f8', first=0):
    """One cp_hmc_step in ``dtype``: ``(new state, next (B, ndim), extra)``.  ``state`` holds the arrays of STATE and TRAJECTORY, ``trial`` those of TRIAL
    (float64 and int32; left as they are), ``L`` the factors (float64: the device's own input), chain b of the batch is chain ``first + b`` of the streams.
    ``extra``: ``accept`` (B,) bool, ``margin`` = H1 - h0 - e and ``scale`` = max(1, |h0|, |H1|) of the chains a close decides by energy (NaN elsewhere),
    ``sample`` and ``sample_chi2`` where the call closes."""
    ty = np.dtype(dtype).type
    t = lambda a: np.asarray(a).astype(dtype)      # noqa: E731
    x, g, chi = (t(state[name]).copy() for name in STATE[:3])
    status, nacc, nout = (state[name].copy() for name in STATE[3:])
    z, h0, eps = (t(state[name]).copy() for name in TRAJECTORY[:3])
    out = state['out'].copy()
    xt, gt, chit = (t(trial[name]) for name in TRIAL)
    L, lo, hi, size, jitter = t(L), t(lo), t(hi), t(np.broadcast_to(step_size, chi.shape)), ty(jitter)
    B, n = x.shape
    b = first + np.arange(B)
    closing, opening = t_close is not None, t_open is not None
    inside = lambda cand: np.isfinite(cand) & (cand >= lo) & (cand <= hi)      # noqa: E731
    extra = {'accept': np.zeros(B, dtype='?'), 'margin': np.full(B, np.nan, dtype=dtype), 'scale': np.ones(B, dtype=dtype)}
    with np.errstate(all='ignore'):
        run = status == 0
        nxt = x.copy()
        if closing or not opening:
            y = forward(L, gt)
            ke = ty(0.5) * eps if closing else eps
            z = np.where((run & (out == 0))[:, None], z + ke[:, None] * y, z)
        if not closing and not opening:
            cand = xt + eps[:, None] * backward(L, z)
            leaves = ~inside(cand).all(axis=1)
            nxt = np.where(run[:, None], np.where(((out != 0) | leaves)[:, None], xt, cand), x)
            out = np.where(run & leaves, 1, out).astype('i4')
        if closing:
            h1 = ty(0.5) * chit + ty(0.5) * squares(z)
            e = jitter_and_energy(seed, b, t_close, dtype)[1]
            was_out = run & (out != 0)
            nout = (nout + was_out).astype('i4')
            decided = run & ~was_out
            accept = decided & np.isfinite(chit) & np.isfinite(h1) & (h1 - h0 < e)
            by_energy = decided & np.isfinite(chit) & np.isfinite(h1)
            extra['accept'] = accept
            extra['margin'] = np.where(by_energy, h1 - h0 - e, np.nan)
            extra['scale'] = np.where(by_energy, np.maximum(1, np.maximum(np.abs(h0), np.abs(h1))), 1)
            x, g, chi = np.where(accept[:, None], xt, x), np.where(accept[:, None], gt, g), np.where(accept, chit, chi)
            nacc = (nacc + accept).astype('i4')
            extra['sample'], extra['sample_chi2'] = x.copy(), chi.copy()
            nxt = x.copy()
        if opening:
            good = np.isfinite(size) & (size > 0)
            drawn = normals(seed, b, t_open, n, dtype)
            uj = jitter_and_energy(seed, b, t_open, dtype)[0]
            eps_new = size * (ty(1.) + jitter * (ty(2.) * uj - ty(1.)))
            h0_new = ty(0.5) * chi + ty(0.5) * squares(drawn)
            z_new = drawn + (ty(0.5) * eps_new)[:, None] * forward(L, g)
            cand = x + eps_new[:, None] * backward(L, z_new)
            leaves = ~inside(cand).all(axis=1)
            ok = run & good
            status = np.where(run & ~good, 3, status).astype('i4')
            z, eps, h0 = np.where(ok[:, None], z_new, z), np.where(ok, eps_new, eps), np.where(ok, h0_new, h0)
            out = np.where(ok, leaves, out).astype('i4')
            nxt = np.where(ok[:, None], np.where(leaves[:, None], x, cand), x)
    new = dict(zip(STATE + TRAJECTORY, (x, g, chi, status, nacc, nout, z, h0, eps, out)))
    return new, nxt, extra


def blocks(a):
    a = np.asarray(a)
    return a.reshape(len(a), -1)


def assert_levels(dev, truth, restated, what=''):
    """Blocks along the first axis (one chain each) by the rule of tests/jacobian_reference.py; a NaN of the restatement must be one on the device and in
    the truth, and is then left out."""
    dev, truth, restated = blocks(dev), blocks(truth), blocks(restated)
    nan = np.isnan(restated)
    assert np.array_equal(np.isnan(dev), nan) and np.array_equal(np.isnan(truth), nan), what + ': the NaNs differ'
    clean = lambda a: np.where(nan, 0, a).T      # noqa: E731
    jr.assert_within(clean(dev), clean(truth), clean(restated), what)


def worst_level(truth, restated):
    """The largest level over the blocks, in floors (NaNs of both left out)."""
    truth, restated = blocks(truth), blocks(restated)
    nan = np.isnan(restated)
    assert np.array_equal(np.isnan(truth), nan)
    return float(jr.levels(np.where(nan, 0, truth).T, np.where(nan, 0, restated).T)[1].max() / FLOOR)


KINDS = ('accept', 'reject', 'coin', 'out', 'leave', 'nan-gradient', 'bad-chi2', 'frozen', 'bad-step', 'bad-pivot')
FLAGS = {'inner': (None, None), 'close': (5, None), 'open': (None, 0), 'both': (7, 8)}
JITTER, SEED = 0.1, 20261021


def batch_sizes(ndim):
    """One chain, the chains of a workgroup, and one more."""
    per_workgroup = lanes(ndim)[2]
    return sorted({1, per_workgroup, per_workgroup + 1})


def make_case(ndim, B, seed=0):
    """(state, trial, metric, lo, hi, step_size, kinds) of a batch of B chains of ndim parameters in the middle of a trajectory, chain b of kind
    ``KINDS[(b + seed) % len(KINDS)]``.  ``h0`` is set against the H1 a close of this call finds (computed here in float64), so that the kinds are what they say
    whatever the random numbers:
    accept / reject: H1 - h0 = -1 and +50 (e > 0 always, and e = 50 has a chance of 2e-22); coin: H1 - h0 = 0.7, accepted where e > 0.7; out: ``out``
    already set by an earlier step; leave: a metric 4e12 times lighter than the others', so that the drift of this call leaves the box; nan-gradient: a NaN in
    the trial's gradient; bad-chi2: a trial chi2 of +inf or NaN; frozen: a status of 1, 2 or 3 already; bad-step: a ``step_size`` of 0, -1, NaN or +inf;
    bad-pivot: a metric whose last pivot fails (cp_hmc_factor sets status 3).  The box is finite but for parameter 2 (where there is one)."""
    rng = np.random.default_rng(3000 * ndim + 11 * B + seed)
    n = ndim
    lo, hi = -1. - rng.uniform(0., 1., n), 1. + rng.uniform(0., 1., n)
    if n >= 3:
        lo[2], hi[2] = -np.inf, np.inf
    kinds = [KINDS[(b + seed) % len(KINDS)] for b in range(B)]
    metric = np.stack([(1e-10 if kind == 'leave' else 400.) * lr.spd(rng, n) for kind in kinds])
    delta = lambda: rng.uniform(-0.01, 0.01, (B, n))      # noqa: E731
    state = dict(x=rng.uniform(-0.5, 0.5, (B, n)), gradient=np.einsum('bij,bj->bi', metric, delta()), chi2=10.**rng.uniform(0., 2., B), status=np.zeros(B, dtype='i4'),
                 naccepted=rng.integers(0, 6, B).astype('i4'), nout=rng.integers(0, 3, B).astype('i4'), z=rng.standard_normal((B, n)), h0=np.zeros(B),
                 eps=0.25 * (1. + 0.1 * rng.uniform(-1., 1., B)), out=np.zeros(B, dtype='i4'))
    trial = dict(x=rng.uniform(-0.5, 0.5, (B, n)), gradient=np.einsum('bij,bj->bi', metric, delta()), chi2=10.**rng.uniform(0., 2., B))
    step_size = 0.25 * (1. + 0.2 * rng.uniform(-1., 1., B))
    for b, kind in enumerate(kinds):
        turn = b // len(KINDS)
        if kind == 'out':
            state['out'][b] = 1
        elif kind == 'nan-gradient':
            trial['gradient'][b, turn % n] = np.nan
        elif kind == 'bad-chi2':
            trial['chi2'][b] = (np.inf, np.nan)[turn % 2]
        elif kind == 'frozen':
            state['status'][b] = 1 + turn % 3
        elif kind == 'bad-step':
            step_size[b] = (0., -1., np.nan, np.inf)[turn % 4]
        elif kind == 'bad-pivot':
            metric[b, n - 1, n - 1] *= -1.
    L = factor(metric, state['status'])[0]
    with np.errstate(all='ignore'):
        h1 = 0.5 * trial['chi2'] + 0.5 * squares(state['z'] + (0.5 * state['eps'])[:, None] * forward(L, trial['gradient']))
    offset = np.array([{'reject': -50., 'coin': -0.7}.get(kind, 1.) for kind in kinds])
    state['h0'] = np.where(np.isfinite(h1), h1, 10.) + offset
    return state, trial, metric, lo, hi, step_size, kinds


class LinearModel(object):
    """A calculator linear in ndim parameters with Gaussian data: y = A theta + c (ncols outputs), weights w, data d.  ``evaluate(x)`` is what
    ``gauss_newton`` returns; the posterior of exp(-chi2 / 2) is the Gaussian of mean ``mode`` and precision ``fisher``."""

    def __init__(self, ndim, ncols=8, seed=0):
        rng = np.random.default_rng(100 * ndim + seed)
        self.ndim, self.ncols = ndim, ncols
        self.A = rng.standard_normal((ncols, ndim))
        self.c = rng.standard_normal(ncols)
        self.sigma = 0.05 * (1. + rng.uniform(0., 1., ncols))
        self.weights = 1. / self.sigma**2
        self.truth = rng.uniform(-0.2, 0.2, ndim)
        self.data = self.A @ self.truth + self.c + self.sigma * rng.standard_normal(ncols)
        self.fisher = (self.A.T * self.weights) @ self.A
        self.mode = np.linalg.solve(self.fisher, (self.A.T * self.weights) @ (self.data - self.c))

    def predict(self, x):
        return np.asarray(x) @ self.A.T + self.c

    def evaluate(self, x):
        r = self.data - self.predict(x)
        return np.broadcast_to(self.fisher, (len(x),) + self.fisher.shape), (r * self.weights) @ self.A, (self.weights * r * r).sum(axis=1)

    def whiten(self, samples):
        """(B, ndim) draws of the posterior -> draws of the unit normal: U (theta - mode) with fisher = U^T U."""
        U = np.linalg.cholesky(self.fisher).T
        return (np.asarray(samples) - self.mode) @ U.T

    def limits(self, width=10.):
        """A box of ``width`` posterior standard deviations on each side of the mode."""
        sd = np.sqrt(np.diag(np.linalg.inv(self.fisher)))
        return self.mode - width * sd, self.mode + width * sd


def run(evaluate, start, lo, hi, nsamples=1, nwarmup=20, thin=1, nleapfrog=6, step_size=0.25, jitter=0.1, metric=None, seed=42, dtype='f8'):
    """``Emulator.hmc``'s loop in ``dtype`` on ``evaluate(x) -> (fisher, gradient, chi2)`` (float64 in, cast here): ``(samples (nsamples, B, ndim), chi2
    (nsamples, B), final state)``."""
    cast = lambda x: tuple(np.asarray(v).astype(dtype) for v in evaluate(np.asarray(x).astype('f8')))      # noqa: E731
    x = np.clip(np.asarray(start, dtype='f8'), lo, hi)
    B, n = x.shape
    fisher, gradient, chi2 = cast(x)
    status = np.where(np.isfinite(chi2), 0, 3).astype('i4')
    zero = np.zeros(B, dtype='i4')
    state = dict(x=x.astype(dtype), gradient=gradient, chi2=chi2, status=status, naccepted=zero, nout=zero.copy(), z=np.zeros((B, n), dtype=dtype),
                 h0=np.zeros(B, dtype=dtype), eps=np.zeros(B, dtype=dtype), out=zero.copy())
    metric = fisher if metric is None else np.broadcast_to(np.asarray(metric).astype(dtype), (B, n, n))
    L, state['status'] = factor(metric, state['status'], dtype)
    ntrajectories = nwarmup + nsamples * thin
    samples, samples_chi2 = np.empty((nsamples, B, n), dtype=dtype), np.empty((nsamples, B), dtype=dtype)
    controls = dict(jitter=jitter, seed=seed, dtype=dtype)
    step_typed = lambda state, trial, **kwargs: step(state, trial, L, lo, hi, step_size, **dict(controls, **kwargs))      # noqa: E731
    state, x, extra = step_typed(state, {name: state[name] for name in TRIAL}, t_open=0)
    for t in range(ntrajectories):
        for leap in range(nleapfrog):
            trial = dict(zip(TRIAL, (x,) + cast(x)[1:]))
            if leap < nleapfrog - 1:
                state, x, extra = step_typed(state, trial)
                continue
            state, x, extra = step_typed(state, trial, t_close=t, t_open=t + 1 if t + 1 < ntrajectories else None)
            s, rest = divmod(t - nwarmup + 1, thin)
            if t >= nwarmup and rest == 0:
                samples[s - 1], samples_chi2[s - 1] = extra['sample'], extra['sample_chi2']
    return samples, samples_chi2, state

