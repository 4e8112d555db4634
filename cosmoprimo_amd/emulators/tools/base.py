"""
The ``Emulator`` front end under the reference's name (cosmoprimo/emulators/tools/base.py ``Emulator``), reduced to what the Taylor and MLP engines need:
sample a calculator, fit an engine on the concatenation (npoints, M) of its flattened varied outputs, and give ``predict``, ``jacobian``, ``vjp`` and ``jvp`` back
by output key for B parameter points at once.

One front, four back ends.  Every method shares one plan (``Emulator._plan``: the keys asked for -> the maximal contiguous runs of columns of
:func:`column_runs`, the ``(key, shape, lo, hi)`` entries each run holds, the fixed outputs to return) and one split (``_split``: a run's buffer ->
``{key: view}``), and reads top to bottom as points, plan or objective, loop, format.  The loops are three: ``Emulator._forward`` behind ``jacobian``,
``jvp`` and ``jvp2`` (the engine once per run, every tensor it returns split by key), ``Emulator._reverse`` behind ``vjp`` and ``vjp2`` (a run's operands
as one block, :func:`_block`; the runs' results added in run order), and the objective ``_Chi2`` behind ``gauss_newton``, ``chi2_hessian``,
``least_squares`` and ``hmc``: weights or a dense precision, and data, checked and staged once, then ``evaluate`` (Fisher matrix, gradient, chi2 at any
points), ``cotangent`` (of residuals or second derivatives, under either kind of weights), ``pull`` and ``curvature``.  What ``Emulator`` uses of an
engine: ``name``, ``device``, ``_dev`` (for its device: ``Emulator._device_of``), and ``predict`` / ``jacobian`` / ``jvp`` / ``jvp2`` / ``vjp`` / ``vjp2`` /
``gauss_newton`` with ``columns=`` / ``return_value=``.

The helpers that both engines' ``predict`` / ``jacobian`` / ``vjp`` open with (``_columns``, ``_cotangent``, ``_tangent``, ``_operand``, ``_gauss_newton``, ``_empty``) live here as well; the engines
import this module, which imports them only where it builds one.  Nothing on the path of a call imports anything: at B = 1 a call is its Python.

``Emulator.least_squares`` runs batched Levenberg-Marquardt fits on ``gauss_newton``; what stands between two of its calls is one launch, :func:`lm_step` (with
:func:`lm_state` and :func:`spd_inverse`: module-level, over device tensors, for normal equations of any origin; with ``geodesic=True`` also the engines' ``jvp2``
and ``vjp`` and one more launch, :func:`lm_accelerate`).  Under a dense precision matrix
(``precision=``) the normal equations come from :func:`gauss_newton_dense`, module-level as well: one GEMM on a Jacobian of any origin, which the engines'
``jacobian`` write run by run into one buffer (``out=``).

``Emulator.hmc`` runs batched Hamiltonian Monte Carlo chains on the same evaluations; what stands between two of them is again one launch, :func:`hmc_step`
(with :func:`hmc_state` and :func:`hmc_factor`: module-level, over device tensors, for gradients of any origin).
"""
import numpy as np

from ... import _device as dv
from ... import _lib


def _columns(columns, M):
    """``(start, ncols)`` of ``columns = (start, stop)``, of every one of the ``M`` columns for None.  ``ncols`` is as given, positive or not: the C entry
    points refuse a bad range by name."""
    start, stop = (int(c) for c in columns) if columns is not None else (0, M)
    return start, stop - start


def _empty(d, *shape):
    """An uninitialised float64 tensor on the device of an engine's device state ``d`` (which holds the torch module: no import on the path of a call)."""
    return d['torch'].empty(shape, dtype=d['torch'].float64, device=d['device'])


def _cotangent(cotangent, B, ncols, device):
    """``(cotangent, ldc)``: the cotangent (B, ncols) on ``device`` as the C entry points read it -- float64, columns contiguous, rows ``ldc >= ncols``
    apart: the tensor itself where it is that already (rows of any stride), else a contiguous copy."""
    torch = dv.torch()
    cotangent = dv.to_device(cotangent, device, cache=False)
    if tuple(cotangent.shape) != (B, ncols):
        raise ValueError('cotangent must be of shape ({:d}, {:d}), got {}'.format(B, ncols, tuple(cotangent.shape)))
    if cotangent.dtype != torch.float64 or (ncols > 1 and cotangent.stride(1) != 1) or (B > 1 and cotangent.stride(0) < ncols):
        cotangent = cotangent.to(torch.float64).contiguous()
    return cotangent, int(cotangent.stride(0)) if B > 1 else ncols


def _operand(operand, B, ncols, device, what):
    """``(operand, ld)``: weights or data on ``device`` as ``cp_*_gauss_newton`` reads them -- one row (ncols,) shared by all points, ``ld = 0``, or
    (B, ncols) as :func:`_cotangent` gives it (rows of any stride at least ncols)."""
    torch = dv.torch()
    operand = dv.to_device(operand, device, cache=False)
    if operand.ndim == 1:
        if int(operand.shape[0]) != ncols:
            raise ValueError('{} must be of shape ({:d},) or ({:d}, {:d}), got {}'.format(what, ncols, B, ncols, tuple(operand.shape)))
        return operand.to(torch.float64).contiguous(), 0
    if tuple(operand.shape) != (B, ncols):
        raise ValueError('{} must be of shape ({:d},) or ({:d}, {:d}), got {}'.format(what, ncols, B, ncols, tuple(operand.shape)))
    return _cotangent(operand, B, ncols, device)


def _jacobian_out(d, out, B, ndim, width, return_value):
    """What both engines' ``jacobian`` write: ``(value or None, ldv, jac, ldj)``.  ``out = (value or None, jac)``: the caller's device tensors, written in
    place -- views (B, width) and (B, ndim, width) of wider buffers (a column slice of the operands of :func:`gauss_newton_dense`), float64 with contiguous
    columns, the rows of ``jac`` ``ldj >= width`` apart with a point's rows following each other, those of ``value`` ``ldv >= width`` apart --; None: new
    contiguous tensors (the value only where ``return_value`` asks for it or the engine writes it anyway)."""
    if out is None:
        return (_empty(d, B, width) if return_value else None), width, _empty(d, B, ndim, width), width
    value, jac = out
    torch = d['torch']
    for tensor, shape in ((value, (B, width)), (jac, (B, ndim, width))):
        if tensor is None:
            continue
        ld = int(tensor.stride(-2))
        if tuple(tensor.shape) != shape or tensor.dtype != torch.float64 or tensor.device != d['device'] or (width > 1 and tensor.stride(-1) != 1) or ld < width \
                or (tensor.ndim == 3 and B > 1 and tensor.stride(0) != ndim * ld):
            raise ValueError('out must hold float64 tensors of shapes {} and {} on {} with contiguous columns and evenly spaced rows'.format((B, width), (B, ndim, width), d['device']))
    if return_value and value is None:
        raise ValueError('out holds no tensor for the value')
    return value, int(value.stride(0)) if value is not None else width, jac, int(jac.stride(1))


def _gauss_newton(d, check, entry, need, head, where, B, ndim, start, ncols, weights, data, return_value):
    """What both engines' ``gauss_newton`` do behind their ``_enter``: the operands, the workspace (``need`` doubles, minus a status on an error: raised by ``check``), the
    results, one call of ``entry``.  Returns ``fisher``, or ``(fisher, grad, chi2)`` with data, the value (B, ncols) prepended if asked for."""
    if need < 0:
        check(-need)
    width = max(ncols, 0)
    weights, ldw = _operand(weights, B, width, d['device'], 'weights')
    if data is not None:
        data, ldd = _operand(data, B, width, d['device'], 'data')
    work, fisher = _empty(d, need), _empty(d, B, ndim, ndim)
    grad, chi2 = (_empty(d, B, ndim), _empty(d, B)) if data is not None else (None, None)
    value = _empty(d, B, width) if return_value else None
    check(entry(*head, start, ncols, weights.data_ptr(), ldw, data.data_ptr() if data is not None else None, ldd if data is not None else 0,
                     value.data_ptr() if return_value else None, width, fisher.data_ptr(), grad.data_ptr() if data is not None else None,
                     chi2.data_ptr() if data is not None else None, work.data_ptr(), need, *where))
    toret = (fisher, grad, chi2) if data is not None else (fisher,)
    toret = ((value,) if return_value else ()) + toret
    return toret[0] if len(toret) == 1 else toret


def _in_place(tensor, shape, dtype, device):
    """Is ``tensor`` what a launch writes in place: a contiguous torch tensor of that shape and dtype on ``device``, taken as it is or not at all?"""
    return dv.is_torch(tensor) and tuple(tensor.shape) == shape and tensor.dtype == dtype and tensor.is_contiguous() and tensor.device == device


def _checked_state(state, spec, lo, hi):
    """What :func:`lm_step`, :func:`lm_accelerate` and :func:`hmc_step` check of the state they write in place and of the box: ``(B, ndim, shapes, lo, hi)``.
    ``spec``: ``{name: (rank, dtype name)}`` of the state's tensors, one of rank r of shape ``(B,) + (ndim,) * (r - 1)``."""
    torch = dv.torch()
    x = state['x']
    if x.ndim != 2:
        raise ValueError('the state holds x of shape (B, ndim), got {}'.format(tuple(x.shape)))
    B, ndim = (int(s) for s in x.shape)
    by_rank, shapes = (None, (B,), (B, ndim), (B, ndim, ndim)), {}
    for name, (rank, dtype) in spec.items():      # the predicate of _in_place, in line: this runs per tensor between any two evaluations of a fit or a chain
        tensor, shape = state[name], by_rank[rank]
        if tuple(tensor.shape) != shape or tensor.dtype != getattr(torch, dtype) or not tensor.is_contiguous() or tensor.device != x.device:
            raise ValueError('state[{!r}] must be a contiguous {} tensor of shape {} on {}'.format(name, dtype, shape, x.device))
        shapes[name] = shape
    lo, hi = (dv.to_device(bound, x.device).reshape(-1) for bound in (lo, hi))
    if int(lo.shape[0]) != ndim or int(hi.shape[0]) != ndim:
        raise ValueError('lo and hi must be of shape ({:d},)'.format(ndim))
    return B, ndim, shapes, lo, hi


LM_SPEC = {'x': (2, 'float64'), 'fisher': (3, 'float64'), 'gradient': (2, 'float64'), 'chi2': (1, 'float64'), 'lambda': (1, 'float64'), 'status': (1, 'int32'),
           'naccepted': (1, 'int32')}
LM_STATE = tuple(LM_SPEC)
LM_TRIAL = ('x', 'fisher', 'gradient', 'chi2')


def lm_state(x, lambda0=1e-3):
    """The state of B Levenberg-Marquardt fits that start at ``x`` (B, ndim), a float64 device tensor, as :func:`lm_step` takes it: nothing accepted yet
    (``chi2 = +inf``: the first trial is the start itself), ``lambda = lambda0``, ``status = 0``."""
    torch = dv.torch()
    B, ndim = (int(s) for s in x.shape)
    new = lambda *shape, **kwargs: torch.zeros(shape, dtype=kwargs.get('dtype', torch.float64), device=x.device)      # noqa: E731
    return {'x': x.clone(), 'fisher': new(B, ndim, ndim), 'gradient': new(B, ndim), 'chi2': torch.full((B,), float('inf'), dtype=torch.float64, device=x.device),
            'lambda': torch.full((B,), float(lambda0), dtype=torch.float64, device=x.device), 'status': new(B, dtype=torch.int32), 'naccepted': new(B, dtype=torch.int32)}


def lm_step(state, trial, lo, hi, lambda_up=10., lambda_down=0.1, lambda_min=1e-12, lambda_max=1e12, ftol=1e-8, return_velocity=False):
    """Everything between two ``gauss_newton`` calls of B Levenberg-Marquardt fits at once, in one launch (``cp_lm_step``, csrc/cp_lm.hip), whatever
    produced the normal equations.  ``state``: contiguous device tensors ``x`` (B, ndim), ``fisher`` (B, ndim, ndim), ``gradient`` (B, ndim), ``chi2``,
    ``lambda`` (B,) float64, ``status``, ``naccepted`` (B,) int32 (:func:`lm_state`), updated in place.  ``trial``: ``x``, ``fisher``, ``gradient``,
    ``chi2``, what ``gauss_newton`` returned at ``trial['x']``.  ``lo``, ``hi``: (ndim,) device tensors, the box (infinite where open).

    Per fit: a fit whose ``status`` is not 0 is left alone.  The trial is accepted if its ``chi2`` is finite and not above the state's; it is then copied
    into the state, ``lambda`` is multiplied by ``lambda_down`` (not below ``lambda_min``; not on the first acceptance), and the fit has converged
    (``status = 1``) if ``chi2`` went down by no more than ``ftol`` times itself.  A rejected trial multiplies ``lambda`` by ``lambda_up``; beyond
    ``lambda_max`` the fit has stalled (``status = 2``); a start that is not finite fails (``status = 3``).  A running fit then holds the parameters that
    sit on a bound with the gradient pointing out of the box, solves ``(F + lambda diag F) delta = g`` on the others by Cholesky (a pivot that is not
    positive: ``status = 3``) and moves them by ``delta``, clipped to the box.  Returns ``next`` (B, ndim), the next trial point: ``x`` for a fit that is
    not running.  Nothing is read back and the call does not wait for the device.

    ``return_velocity=True``: ``(next, velocity)``, the same launch (``cp_lm_step_velocity``) and the same bits; ``velocity`` (B, ndim) is ``delta`` on the
    free parameters of a running fit and exactly 0 elsewhere: what :func:`lm_accelerate` takes."""
    torch = dv.torch()
    x = state['x']
    B, ndim, shapes, lo, hi = _checked_state(state, LM_SPEC, lo, hi)
    read = []
    for name in LM_TRIAL:
        tensor = dv.to_device(trial[name], x.device, cache=False)
        if tuple(tensor.shape) != shapes[name]:
            raise ValueError('trial[{!r}] must be of shape {}, got {}'.format(name, shapes[name], tuple(tensor.shape)))
        read.append(tensor)
    out = torch.empty_like(x)
    head = [B, ndim] + [state[name].data_ptr() for name in LM_STATE] + [tensor.data_ptr() for tensor in read] + [lo.data_ptr(), hi.data_ptr()] \
        + [float(lambda_up), float(lambda_down), float(lambda_min), float(lambda_max), float(ftol), out.data_ptr()]
    if not return_velocity:
        _lib.check(_lib.load().cp_lm_step(*head, x.device.index, dv.stream_of(x.device)))
        return out
    velocity = torch.empty_like(x)
    _lib.check(_lib.load().cp_lm_step_velocity(*head, velocity.data_ptr(), x.device.index, dv.stream_of(x.device)))
    return out, velocity


def lm_accelerate(state, velocity, curvature, lo, hi, alpha=0.75, naccelerated=None):
    """Geodesic acceleration (Transtrum & Sethna 2012) of the step :func:`lm_step` just solved, in one launch (``cp_lm_accelerate``, csrc/cp_lm.hip).
    ``state``: as :func:`lm_step` left it (read only); ``velocity`` (B, ndim): what ``lm_step(..., return_velocity=True)`` returned beside ``next``;
    ``curvature`` (B, ndim): ``h = J W y''(v, v)``, the vector-Jacobian product of the weighted second directional derivative of the prediction along the
    velocity, whatever produced it; ``lo``, ``hi``: the box.

    Per running fit: ``a = -(F + lambda diag F)^-1 h`` on the free parameters (the held set of :func:`lm_step`); the correction is taken where
    ``sv > 0``, ``sa`` is finite and ``4 sa <= alpha^2 sv``, with ``sa = sum F_ii a_i^2`` and ``sv = sum F_ii v_i^2`` over the free parameters
    (``2 |a| / |v| <= alpha`` in the Marquardt-scaled norm of the solve): ``next = clip(x + (v + a / 2))``.  Elsewhere ``next`` is the plain step
    ``clip(x + v)``, the bits of :func:`lm_step`'s ``next``; a fit that is over, or whose pivot fails, gets ``x``.  Returns ``next`` (B, ndim).
    ``naccelerated``: (B,) contiguous int32 device tensor, incremented in place where the correction is taken.  Nothing is read back and the call does not
    wait for the device."""
    torch = dv.torch()
    x = state['x']
    B, ndim, shapes, lo, hi = _checked_state(state, LM_SPEC, lo, hi)
    read = []
    for name, tensor in (('velocity', velocity), ('curvature', curvature)):
        tensor = dv.to_device(tensor, x.device, cache=False)
        if tuple(tensor.shape) != (B, ndim):
            raise ValueError('{} must be of shape {}, got {}'.format(name, (B, ndim), tuple(tensor.shape)))
        read.append(tensor.to(torch.float64).contiguous())
    if naccelerated is None:
        naccelerated = torch.zeros((B,), dtype=torch.int32, device=x.device)
    elif not _in_place(naccelerated, (B,), torch.int32, x.device):
        raise ValueError('naccelerated must be a contiguous int32 tensor of shape {} on {}'.format((B,), x.device))
    out = torch.empty_like(x)
    _lib.check(_lib.load().cp_lm_accelerate(B, ndim, *[state[name].data_ptr() for name in ('x', 'fisher', 'gradient', 'lambda', 'status')], lo.data_ptr(), hi.data_ptr(),
                                            read[0].data_ptr(), read[1].data_ptr(), float(alpha), out.data_ptr(), naccelerated.data_ptr(), x.device.index,
                                            dv.stream_of(x.device)))
    return out


def spd_inverse(a):
    """``(inverse, info)`` of the symmetric positive-definite matrices ``a`` (B, ndim, ndim), a device tensor, by Cholesky in one launch
    (``cp_spd_inverse``): symmetric bit for bit; ``info`` (B,) int32 is 0, or the 1-based index of the failing pivot of a matrix whose inverse is then NaN."""
    torch = dv.torch()
    a = a.to(torch.float64).contiguous()
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise ValueError('matrices of shape (B, ndim, ndim), got {}'.format(tuple(a.shape)))
    inv, info = torch.empty_like(a), torch.empty((int(a.shape[0]),), dtype=torch.int32, device=a.device)
    _lib.check(_lib.load().cp_spd_inverse(int(a.shape[0]), int(a.shape[1]), a.data_ptr(), inv.data_ptr(), info.data_ptr(), a.device.index, dv.stream_of(a.device)))
    return inv, info


HMC_STATE = ('x', 'gradient', 'chi2', 'status', 'naccepted', 'nout')
HMC_TRAJECTORY = ('z', 'h0', 'eps', 'out')
HMC_SPEC = {'x': (2, 'float64'), 'gradient': (2, 'float64'), 'chi2': (1, 'float64'), 'status': (1, 'int32'), 'naccepted': (1, 'int32'), 'nout': (1, 'int32'),
            'z': (2, 'float64'), 'h0': (1, 'float64'), 'eps': (1, 'float64'), 'out': (1, 'int32')}      # HMC_STATE, then HMC_TRAJECTORY
HMC_TRIAL = ('x', 'gradient', 'chi2')


def hmc_state(x, gradient, chi2):
    """The state of B Hamiltonian Monte Carlo chains that start at ``x`` (B, ndim), with ``gradient`` (B, ndim) and ``chi2`` (B,) what ``gauss_newton``
    returned there (float64 device tensors, copied), as :func:`hmc_step` takes it: nothing accepted yet, no trajectory open (``z``, ``h0``, ``eps``,
    ``out`` zero), ``status = 0``, and 3 -- by a ``torch.where``, nothing is read back -- where ``chi2`` is not finite: such a chain never moves."""
    torch = dv.torch()
    if x.ndim != 2 or tuple(gradient.shape) != tuple(x.shape) or tuple(chi2.shape) != (int(x.shape[0]),):
        raise ValueError('x and gradient of shape (B, ndim) and chi2 of shape (B,), got {}, {} and {}'.format(tuple(x.shape), tuple(gradient.shape), tuple(chi2.shape)))
    B, ndim = (int(s) for s in x.shape)
    new = lambda *shape, **kwargs: torch.zeros(shape, dtype=kwargs.get('dtype', torch.float64), device=x.device)      # noqa: E731
    chi2 = chi2.to(torch.float64).clone()
    status = torch.where(torch.isfinite(chi2), new(B, dtype=torch.int32), torch.full((B,), 3, dtype=torch.int32, device=x.device))
    return {'x': x.to(torch.float64).clone(), 'gradient': gradient.to(torch.float64).clone(), 'chi2': chi2, 'status': status, 'naccepted': new(B, dtype=torch.int32),
            'nout': new(B, dtype=torch.int32), 'z': new(B, ndim), 'h0': new(B), 'eps': new(B), 'out': new(B, dtype=torch.int32)}


def _hmc_step_size(step_size, B, device):
    """The step sizes of B chains as ``cp_hmc_step`` reads them: a contiguous float64 tensor (B,) on ``device``, from a scalar (a fill on the device) or (B,)."""
    torch = dv.torch()
    if not dv.is_torch(step_size) and np.ndim(step_size) == 0:
        return torch.full((B,), float(step_size), dtype=torch.float64, device=device)
    step_size = dv.to_device(step_size, device)
    if step_size.ndim == 0:
        return step_size.expand(B).contiguous()
    if tuple(step_size.shape) != (B,):
        raise ValueError('step_size must be a scalar or of shape ({:d},), got {}'.format(B, tuple(step_size.shape)))
    return step_size


def hmc_factor(metric, status):
    """The Cholesky factors ``L`` (B, ndim, ndim) of the mass matrices ``metric`` (B, ndim, ndim), a device tensor (its lower triangle is read), in one launch
    (``cp_hmc_factor``, csrc/cp_hmc.hip): lower triangular, the strict upper triangle zero.  ``status``: (B,) contiguous int32 device tensor (that of
    :func:`hmc_state`), set in place to 3 where a pivot is not positive and finite -- the chain then never moves -- and left as it is elsewhere."""
    torch = dv.torch()
    metric = metric.to(torch.float64).contiguous()
    if metric.ndim != 3 or metric.shape[1] != metric.shape[2]:
        raise ValueError('matrices of shape (B, ndim, ndim), got {}'.format(tuple(metric.shape)))
    B, ndim = int(metric.shape[0]), int(metric.shape[1])
    if not _in_place(status, (B,), torch.int32, metric.device):
        raise ValueError('status must be a contiguous int32 tensor of shape {} on {}'.format((B,), metric.device))
    factor = torch.empty_like(metric)
    _lib.check(_lib.load().cp_hmc_factor(B, ndim, metric.data_ptr(), factor.data_ptr(), status.data_ptr(), metric.device.index, dv.stream_of(metric.device)))
    return factor


def hmc_step(state, trial, factor, lo, hi, step_size, t_close=None, t_open=None, jitter=0.1, seed=0, sample=None, sample_chi2=None):
    """Everything between two ``gauss_newton`` calls of B Hamiltonian Monte Carlo chains of ``exp(-chi2 / 2)`` at once, in one launch (``cp_hmc_step``,
    csrc/cp_hmc.hip), whatever produced the gradients.  ``state``: contiguous device tensors ``x`` (B, ndim), ``gradient`` (B, ndim), ``chi2`` (B,) float64,
    ``status``, ``naccepted``, ``nout`` (B,) int32, and the open trajectory: the whitened momentum ``z`` (B, ndim), ``h0``, ``eps`` (B,), ``out`` (B,) int32
    (:func:`hmc_state`), updated in place.  ``trial``: ``x``, ``gradient``, ``chi2``, what ``gauss_newton`` returned at ``trial['x']``.  ``factor``: what
    :func:`hmc_factor` returned.  ``lo``, ``hi``: (ndim,), the box.  ``step_size``: a scalar or (B,), in units of the whitened coordinates.

    With neither ``t_close`` nor ``t_open`` the call is a leapfrog step inside a trajectory: a kick by the trial's gradient and a drift.  ``t_close``: the
    number of the trajectory the call closes (half a kick, then accept or reject against ``-log u`` of that trajectory's stream; ``naccepted`` counts);
    ``sample`` (B, ndim) and ``sample_chi2`` (B,), contiguous float64 device tensors given together, then take the state.  ``t_open``: the number of the
    trajectory it opens, after the close where both are given: fresh momenta, ``eps = step_size (1 + jitter (2 u - 1))``, half a kick and a drift.  A drift
    that leaves the box marks the chain ``out``: it stays where it is until its trajectory closes, which then rejects it (``nout`` counts), so nothing is
    ever evaluated outside the box.  The random numbers are Philox4x32-10 of ``(seed, chain, trajectory)`` in the kernel: they do not depend on B.
    A chain with ``status != 0`` is left alone.  Returns ``next`` (B, ndim), the next trial point.  Nothing is read back and the call does not wait for the
    device."""
    torch = dv.torch()
    x = state['x']
    B, ndim, shapes, lo, hi = _checked_state(state, HMC_SPEC, lo, hi)
    read = []
    for name in HMC_TRIAL:
        tensor = dv.to_device(trial[name], x.device, cache=False)
        if tuple(tensor.shape) != shapes[name]:
            raise ValueError('trial[{!r}] must be of shape {}, got {}'.format(name, shapes[name], tuple(tensor.shape)))
        read.append(tensor.to(torch.float64).contiguous())
    if not _in_place(factor, (B, ndim, ndim), torch.float64, x.device):
        raise ValueError('factor must be a contiguous float64 tensor of shape {} on {}'.format((B, ndim, ndim), x.device))
    step_size = _hmc_step_size(step_size, B, x.device)
    if (sample is None) != (sample_chi2 is None):
        raise ValueError('sample and sample_chi2 are given together')
    for name, tensor, shape in (('sample', sample, (B, ndim)), ('sample_chi2', sample_chi2, (B,))):
        if tensor is not None and not _in_place(tensor, shape, torch.float64, x.device):
            raise ValueError('{} must be a contiguous float64 tensor of shape {} on {}'.format(name, shape, x.device))
    out = torch.empty_like(x)
    _lib.check(_lib.load().cp_hmc_step(B, ndim, -1 if t_close is None else int(t_close), -1 if t_open is None else int(t_open),
                                       *[state[name].data_ptr() for name in HMC_STATE + HMC_TRAJECTORY], *[tensor.data_ptr() for tensor in read], factor.data_ptr(),
                                       lo.data_ptr(), hi.data_ptr(), step_size.data_ptr(), float(jitter), int(seed) & 0xffffffffffffffff, out.data_ptr(),
                                       sample.data_ptr() if sample is not None else None, sample_chi2.data_ptr() if sample_chi2 is not None else None,
                                       x.device.index, dv.stream_of(x.device)))
    return out


def _rows(x, shape, device, what):
    """``(x, ld)``: the operand ``x`` of shape ``shape = (..., nrows, ncols)`` on ``device`` as ``cp_gauss_newton_dense`` reads it -- float64, columns contiguous,
    rows ``ld >= ncols`` apart, a leading axis continuing the rows: the tensor itself where it is that already (rows of any admissible stride), else a
    contiguous copy.  A host array is uploaded (through the cache of :func:`_device.upload`: read only)."""
    torch = dv.torch()
    x = x.to(device=device) if dv.is_torch(x) else dv.upload(np.asarray(x, dtype='f8'), device)
    if tuple(x.shape) != shape:
        raise ValueError('{} must be of shape {}, got {}'.format(what, shape, tuple(x.shape)))
    ncols, ld = shape[-1], int(x.stride(-2))
    if x.dtype != torch.float64 or (ncols > 1 and x.stride(-1) != 1) or ld < max(ncols, 1) or (x.ndim == 3 and x.stride(0) != shape[1] * ld):
        x, ld = x.to(torch.float64).contiguous(), ncols
    return x, ld


def gauss_newton_dense(jacobian, value, precision, data=None):
    """Fisher matrices and Gauss-Newton normal equations under a dense precision matrix, whatever produced the Jacobian, in one GEMM on the matrix cores
    (``cp_gauss_newton_dense``, csrc/cp_gauss_newton_dense.hip).  ``jacobian`` (B, ndim, N), ``value`` (B, N) (None is accepted without ``data``),
    ``precision`` (N, N), symmetric and finite, shared by all points, ``data`` (B, N) or one row (N,): device tensors, with rows of any stride of at
    least N taken as they are, or host arrays (uploaded).  With ``A_b = [J_b ; data_b - value_b]`` and ``G_b = A_b P A_b^T``: returns ``fisher`` (B, ndim, ndim)
    ``= G_b[:ndim, :ndim]`` (symmetric bit for bit), or with ``data`` ``(fisher, gradient, chi2)``, ``gradient`` (B, ndim) ``= G_b[:ndim, ndim]`` and ``chi2``
    (B,) ``= G_b[ndim, ndim]``, device tensors.  A column ``c`` with ``precision[c, c] == 0`` is dropped, whatever the Jacobian, the value or the data hold there
    (NaN included): a mask.  No atomics: two calls give the same bits.  Nothing is read back and the call does not wait for the device."""
    torch = dv.torch()
    device = dv.resolve_device(None, jacobian, value, precision, data)
    if np.ndim(jacobian) != 3:
        raise ValueError('jacobian must be of shape (B, ndim, N), got {}'.format(tuple(np.shape(jacobian))))
    B, ndim, N = (int(s) for s in np.shape(jacobian))
    jacobian, ldj = _rows(jacobian, (B, ndim, N), device, 'jacobian')
    precision, ldp = _rows(precision, (N, N), device, 'precision')
    if data is not None and value is None:
        raise ValueError('data needs the value')
    ldv = ldd = 0
    if value is not None:
        value, ldv = _rows(value, (B, N), device, 'value')
    if data is not None:
        data = data if dv.is_torch(data) else np.asarray(data, dtype='f8')
        if data.ndim == 1:      # one row shared by all points
            data = _rows(data[None], (1, N), device, 'data')[0]
        else:
            data, ldd = _rows(data, (B, N), device, 'data')
    new = lambda *shape, **kwargs: (torch.zeros if kwargs.get('zero') else torch.empty)(shape, dtype=torch.float64, device=device)      # noqa: E731
    empty = B == 0 or N == 0      # nothing to launch: zeros
    fisher = new(B, ndim, ndim, zero=empty)
    grad, chi2 = (new(B, ndim, zero=empty), new(B, zero=empty)) if data is not None else (None, None)
    if not empty:
        lib = _lib.load()
        need = int(lib.cp_gauss_newton_dense_workspace_doubles(B, ndim, N))
        if need < 0:
            _lib.check(-need)
        work = new(need)
        ptr = lambda tensor: tensor.data_ptr() if tensor is not None else None      # noqa: E731
        _lib.check(lib.cp_gauss_newton_dense(jacobian.data_ptr(), ldj, B, ndim, N, ptr(value), ldv, ptr(data), ldd, precision.data_ptr(), ldp, fisher.data_ptr(), ptr(grad),
                                             ptr(chi2), work.data_ptr(), need, device.index, dv.stream_of(device)))
    return fisher if data is None else (fisher, grad, chi2)


def _tangent(tangents, B, ndim, device):
    """``(tangents (B, K, ndim), K, single)``: the directions on ``device`` as the C entry points read them -- float64, contiguous; ``single``: they were
    given as (B, ndim), one direction per point."""
    torch = dv.torch()
    tangents = dv.to_device(tangents, device, cache=False)
    single = tangents.ndim == 2
    if single:
        tangents = tangents[:, None, :]
    if tangents.ndim != 3 or int(tangents.shape[0]) != B or int(tangents.shape[2]) != ndim:
        raise ValueError('tangents must be of shape ({0:d}, {1:d}) or ({0:d}, K, {1:d}), got {2}'.format(B, ndim, tuple(tangents.shape)))
    return tangents.to(torch.float64).contiguous(), int(tangents.shape[1]), single


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


def _split(out, lead, entries, start, scalar):
    """``{key: view}`` of the buffer ``out`` (..., ncols) of a run of columns that starts at ``start``: per entry ``(key, shape, lo, hi)`` its columns as
    ``lead + shape``, without the leading axis if every parameter is a scalar."""
    toret = {}
    for key, shape, lo, hi in entries:
        block = out[..., lo - start:hi - start].reshape(lead + shape)
        toret[key] = block[0] if scalar else block
    return toret


def _block(operands, entries, B, dev):
    """The operands ``{key: array or tensor}`` of the ``entries`` of a run as one float64 tensor (B, ncols) on ``dev``, in the order of the columns: each is
    broadcast to ``(B,) + shape`` of its output; an output without columns holds none."""
    torch = dv.torch()
    blocks = [torch.broadcast_to(dv.to_device(operands[key], dev, cache=False).to(torch.float64), (B,) + shape).reshape(B, hi - lo)
              for key, shape, lo, hi in entries if hi > lo]
    return blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1)


class _Chi2(object):

    """The chi2 of a fit of ``data`` to the emulated outputs, as :meth:`Emulator.gauss_newton`, :meth:`Emulator.chi2_hessian`, :meth:`Emulator.least_squares` and
    :meth:`Emulator.hmc` share it: ``weights``, ``data`` (or None) and ``precision`` (or None) as :meth:`Emulator.gauss_newton` takes them, checked -- its
    ``KeyError`` / ``ValueError`` / ``TypeError`` are raised here -- and staged once on the device ``dev`` for B points, ``X`` (B, ndim) among what the device is
    resolved from.  ``runs``: the maximal contiguous runs ``[(start, stop, entries), ...]`` of :meth:`Emulator._plan` over the varied keys asked for (``keys``);
    ``weights`` and ``data``: per run, the operands as (B, stop - start) blocks (``data``: None each without data); ``fixed``: the fixed outputs asked for.

    Under a dense ``precision`` over the outputs ``weights`` lists (a sequence of distinct varied keys: those outputs flattened in C order and concatenated
    as listed, N entries), run r fills the columns ``columns[r]`` (a slice) of the N columns of the data vector in the order of the column plan; ``precision``
    (N, N), given in the listed order, is permuted here, once and on the device, to that order; ``jac`` (B, ndim, N) and ``value`` (B, N) are the buffers the
    engine's ``jacobian`` writes into, ``data`` views of one (B, N) block and ``weights`` None."""

    def __init__(self, emulator, weights, data, precision, X, B):
        torch = dv.torch()
        self.engine, self.B, self.ndim, self.has_data, self._masks = emulator.engine, B, len(emulator.params), data is not None, None
        if precision is None:
            self.dev = dev = emulator._device_of(X, *weights.values())
            self.keys, self.precision = weights, None
            self.runs, self.fixed = emulator._plan(list(weights), exact=True)
            if data is not None:
                unknown = [key for key in data if key not in weights]
                if unknown:
                    raise KeyError('data for {}, which hold no weights'.format(unknown))
                missing = [key for key in weights if key in emulator.varied_keys and key not in data]
                if missing:
                    raise ValueError('no data for {}'.format(missing))
            self.weights = [_block(weights, entries, B, dev) for start, stop, entries in self.runs]
            self.data = [_block(data, entries, B, dev) if data is not None else None for start, stop, entries in self.runs]
            return
        self.dev = dev = emulator._device_of(X, precision)
        if isinstance(weights, dict):
            raise TypeError('with a precision matrix, weights is the sequence of the output keys its rows and columns follow, not a dictionary')
        self.keys = keys = [weights] if isinstance(weights, str) else list(weights)
        if len(set(keys)) != len(keys):
            raise ValueError('keys listed twice in {}'.format(keys))
        unknown = [key for key in keys if key not in emulator.varied_keys]
        if unknown:
            raise KeyError('no varied output {}'.format(unknown))
        if data is not None:
            unknown = [key for key in data if key not in keys]
            if unknown:
                raise KeyError('data for {}, which the precision matrix does not cover'.format(unknown))
            missing = [key for key in keys if key not in data]
            if missing:
                raise ValueError('no data for {}'.format(missing))
        sizes = {key: int(np.prod(shape, dtype='i8')) for key, shape in zip(emulator.varied_keys, emulator.varied_shapes)}
        listed, N = {}, 0      # where a key starts in the listed order
        for key in keys:
            listed[key] = N
            N += sizes[key]
        if tuple(np.shape(precision)) != (N, N):
            raise ValueError('precision must be of shape ({0:d}, {0:d}) for {1}, got {2}'.format(N, keys, tuple(np.shape(precision))))
        self.runs, self.fixed = (emulator._plan(keys, exact=True)[0] if keys else []), {}
        self.columns, order, q = [], [], 0
        for start, stop, entries in self.runs:
            self.columns.append(slice(q, q + stop - start))
            order += [np.arange(listed[key], listed[key] + hi - lo) for key, shape, lo, hi in entries]
            q += stop - start
        order = np.concatenate(order) if order else np.zeros(0, dtype='i8')
        precision = precision.to(device=dev, dtype=torch.float64) if dv.is_torch(precision) else dv.upload(np.asarray(precision, dtype='f8'), dev)
        if not np.array_equal(order, np.arange(N)):
            index = dv.upload(order.astype('i8'), dev)
            precision = precision.index_select(0, index).index_select(1, index)
        self.precision, self.weights, self._data = precision.contiguous(), None, None
        if data is not None:
            self._data = _block(data, [entry for start, stop, entries in self.runs for entry in entries], B, dev) if N else torch.zeros((B, 0), dtype=torch.float64, device=dev)
        self.data = [self._data[:, cols] if data is not None else None for cols in self.columns]
        self.jac, self.value = (torch.empty(shape, dtype=torch.float64, device=dev) for shape in ((B, self.ndim, N), (B, N)))

    def _zeros(self, *shape):
        return dv.torch().zeros(shape, dtype=dv.torch().float64, device=self.dev)

    def evaluate(self, x, return_value=False):
        """One evaluation at the points ``x`` (B, ndim): ``(fisher,)``, with data ``(fisher, gradient, chi2)``, device tensors (B, ndim, ndim), (B, ndim) and
        (B,); ``return_value=True``: ``(values, totals)``, ``values`` the prediction per run, (B, stop - start).  Diagonal weights: the engine's
        ``gauss_newton`` once per run, the runs' results added in run order (no run: zeros).  Dense precision: the engine's ``jacobian`` once per run, written
        straight into its column slice of ``jac`` and -- with data, or where the value is asked for -- of ``value``, then :func:`gauss_newton_dense`."""
        if self.precision is not None:
            value = self.value if self.has_data or return_value else None
            for (start, stop, entries), cols in zip(self.runs, self.columns):
                self.engine.jacobian(x, columns=(start, stop), return_value=value is not None, out=(value[:, cols] if value is not None else None, self.jac[:, :, cols]))
            totals = gauss_newton_dense(self.jac, value, self.precision, data=self._data)
            totals = totals if isinstance(totals, tuple) else (totals,)
            return ([self.value[:, cols] for cols in self.columns], totals) if return_value else totals
        totals, values = None, []
        for (start, stop, entries), wblock, dblock in zip(self.runs, self.weights, self.data):
            out = self.engine.gauss_newton(x, wblock, data=dblock, columns=(start, stop), return_value=return_value)
            out = out if isinstance(out, tuple) else (out,)
            if return_value:
                values.append(out[0])
                out = out[1:]
            totals = out if totals is None else tuple(a + b for a, b in zip(totals, out))
        if totals is None:
            totals = (self._zeros(self.B, self.ndim, self.ndim),) + ((self._zeros(self.B, self.ndim), self._zeros(self.B)) if self.has_data else ())
        return (values, totals) if return_value else totals

    def cotangent(self, blocks):
        """Yield, per run, the cotangent (B, stop - start) of the ``blocks`` ``q`` -- per run a residual ``data - y`` or a second derivative of ``y`` -- under the
        weights: ``where(w == 0, 0, w q)`` (a select: NaN under a zero weight stay masked); under a dense precision ``P`` the ``q`` of all runs, the columns
        with ``P[c, c] == 0`` dropped as :func:`gauss_newton_dense` drops them, times ``P``, masked again.  ``blocks`` may be a generator: diagonal weights
        take a run's block when its cotangent is asked for, a precision, which couples the runs, takes them all first."""
        torch = dv.torch()
        if self._masks is None:
            self._masks = (self._zeros(), self.precision.diagonal() == 0 if self.precision is not None else None)
        zero, dropped = self._masks
        if self.precision is None:
            for w, q in zip(self.weights, blocks):
                yield torch.where(w == 0, zero, w * q)
            return
        blocks = list(blocks)
        if blocks:
            q = torch.where(dropped, zero, blocks[0] if len(blocks) == 1 else torch.cat(blocks, dim=1))
            q = torch.where(dropped, zero, torch.matmul(q, self.precision))
            for cols in self.columns:
                yield q[:, cols]

    def pull(self, method, x, blocks, rank):
        """The engine's ``method`` ('vjp', 'vjp2') at ``x`` on the cotangent ``blocks`` of :meth:`cotangent`, once per run, the runs' results
        (B,) + (ndim,) * rank added in run order (no run: zeros)."""
        total = None
        for (start, stop, entries), block in zip(self.runs, blocks):
            out = getattr(self.engine, method)(x, block, columns=(start, stop))
            total = out if total is None else total + out
        return total if total is not None else self._zeros(self.B, *((self.ndim,) * rank))

    def curvature(self, at, velocity):
        """``h = J W y''(v, v)`` (B, ndim) for :func:`lm_accelerate`: per run the second directional derivative of the prediction along ``velocity`` at the
        points ``at`` (the engine's ``jvp2``, a row per fit), its :meth:`cotangent`, and the engine's ``vjp`` of that."""
        return self.pull('vjp', at, self.cotangent(self.engine.jvp2(at, velocity, columns=(start, stop)) for start, stop, entries in self.runs), 1)


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
                from .taylor import TaylorEmulatorEngine
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

    def _device_of(self, *operands):
        """The device of a call: the fitted engine's, else what :func:`_device.resolve_device` makes of the engine's ``device`` and the ``operands``."""
        return self.engine._dev['device'] if self.engine._dev is not None else dv.resolve_device(self.engine.device, *operands)

    def _points(self, params):
        """(X (B, ndim) in the order of ``self.params``, a host array unless a parameter is a device tensor; B; whether every parameter is a scalar)."""
        missing = [name for name in self.params if name not in params]
        if missing:
            raise ValueError('missing parameters {}'.format(missing))
        values = [params[name] for name in self.params]
        dev = self._device_of(*values)
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

    def _plan(self, keys, exact=False):
        """What :meth:`predict`, :meth:`jacobian`, :meth:`vjp` and :meth:`jvp` compute for ``keys`` -- a list of output names or section prefixes, or one such string
        (``exact``: names only, the keys of cotangents), or None for every output: ``(runs, fixed)``, ``runs = [(start, stop, entries), ...]`` the maximal
        contiguous runs of columns of :func:`column_runs` (None: all columns as one run) with the ``(key, shape, lo, hi)`` of the varied outputs asked
        for that each holds, ``fixed`` the fixed outputs asked for.  A name that matches no output raises ``KeyError``; one that matches fixed outputs
        only needs no column."""
        columns = _key_columns(self.varied_keys, self.varied_shapes)
        if keys is None:
            return [(0, columns[-1][3] if columns else 0, columns)], dict(self.fixed)
        names = [keys] if isinstance(keys, str) else list(keys)
        asked = (lambda key, names: key in names) if exact else _requested
        unknown = [name for name in names if not any(asked(key, [name]) for key in list(self.varied_keys) + list(self.fixed))]
        if unknown:
            raise KeyError('no output {}'.format(unknown))
        runs = column_runs(self.varied_keys, self.varied_shapes, [name for name in names if any(asked(key, [name]) for key in self.varied_keys)])
        return ([(start, stop, [entry for entry in columns if start <= entry[2] and entry[3] <= stop and asked(entry[0], names)]) for start, stop in runs],
                {key: value for key, value in self.fixed.items() if asked(key, names)})

    def predict(self, params, device=False, keys=None):
        """Outputs at ``params``, a dictionary of scalars or arrays of B values (host arrays or device tensors): the calculator's keys, varied ones of shape
        ``(B,) + shape`` (no leading axis if every parameter is a scalar), fixed ones as they are.  Host arrays by default; ``device=True``: torch tensors,
        views into one (B, M) buffer, and no synchronisation with the device.

        ``keys``: a list of output names, or a section prefix such as 'background' (every 'background.*' key): these outputs only.  Their columns are
        planned by :func:`column_runs`; each maximal contiguous run of them is one launch of the engine on that range (B, ncols) -- the keys of a section
        are adjacent, so normally one -- and no other column is computed or stored.  The varied keys asked for and the fixed ones under the prefix (or
        among the names) are returned."""
        X, B, scalar = self._points(params)
        runs, fixed = self._plan(keys)
        toret = {}
        for start, stop, entries in runs:
            out = self.engine.predict(X, columns=None if keys is None else (start, stop))
            toret.update(_split(out if device else dv.to_host(out), (B,), entries, start, scalar))
        toret.update(fixed)
        return toret

    def jacobian(self, params, device=False, keys=None, return_value=False):
        """Derivatives of the varied outputs with respect to the parameters at ``params`` (as in :meth:`predict`: scalars or arrays of B values, host or
        device), computed analytically on the device (:meth:`MLPEmulatorEngine.jacobian`, :meth:`TaylorEmulatorEngine.jacobian`):
        ``{key: array (B, ndim) + shape}``, the ``ndim`` axis in the order of ``Emulator.params``, without the leading ``B`` axis if every parameter is a
        scalar.  Fixed outputs are not returned: their derivative is identically zero.  Host arrays by default; ``device=True``: torch tensors, views
        into the (B, ndim, ncols) buffer(s), and no synchronisation with the device.

        ``keys``: as in :meth:`predict` -- the columns are planned by :func:`column_runs`, one call of the engine per maximal contiguous run, and no other
        column is computed.  ``return_value=True``: ``(values, jacobian)``, ``values`` what ``predict(params, device=device, keys=keys)`` returns."""
        X, B, scalar = self._points(params)
        return self._forward('jacobian', X, scalar, self._plan(keys), keys, device, [(B,)] * bool(return_value) + [(B, len(self.params))], return_value=return_value)

    def _forward(self, method, X, scalar, plan, keys, device, leads, *operands, **flags):
        """The run loop of :meth:`jacobian`, :meth:`jvp` and :meth:`jvp2`: the engine's ``method`` on ``X`` and ``operands`` once per run of
        ``plan = self._plan(keys)`` (``columns=None`` for every output), each tensor it returns split by key with its lead shape of ``leads`` (host arrays
        unless ``device``), the values -- the first, under ``return_value=True`` among the ``flags`` -- completed by the fixed outputs.  Returns the
        dictionaries as a tuple, a single one as it is."""
        runs, fixed = plan
        toret = [{} for lead in leads]
        for start, stop, entries in runs:
            out = getattr(self.engine, method)(X, *operands, columns=None if keys is None else (start, stop), **flags)
            for result, lead, tensor in zip(toret, leads, out if isinstance(out, tuple) else (out,)):
                result.update(_split(tensor if device else dv.to_host(tensor), lead, entries, start, scalar))
        if flags.get('return_value'):
            toret[0].update(fixed)
        return tuple(toret) if len(toret) > 1 else toret[0]

    def _values(self, params, values, asked, fixed, device):
        """``values`` -- the varied outputs the runs of a plan over the keys ``asked`` gave -- as ``predict(params, device=device, keys=list(asked))``
        returns them: with the outputs that hold no column, in the calculator's order, then the ``fixed`` outputs."""
        for key in self.varied_keys:      # empty outputs hold no column and join no run
            if key in asked and key not in values:
                values[key] = self.predict(params, device=device, keys=[key])[key]
        values = {key: values[key] for key in self.varied_keys if key in values}
        values.update(fixed)
        return values

    def _reverse(self, method, rank, params, cotangents, device, return_value):
        """The run loop of :meth:`vjp` (``rank`` 1) and :meth:`vjp2` (2): the engine's ``method`` once per run of the plan over the cotangents' varied keys,
        on that run's block of cotangents, the runs' results (B,) + (ndim,) * rank added in run order (no run: zeros).  Returns ``(values, total, scalar)``:
        ``values`` what ``predict(params, device=device, keys=list(cotangents))`` returns (None unless asked for), ``total`` a host array unless ``device``."""
        X, B, scalar = self._points(params)
        runs, fixed = self._plan(list(cotangents), exact=True)
        dev = self._device_of(X, *cotangents.values())
        total, values = None, {}
        for start, stop, entries in runs:
            out = getattr(self.engine, method)(X, _block(cotangents, entries, B, dev), columns=(start, stop), return_value=return_value)
            value, result = out if return_value else (None, out)
            total = result if total is None else total + result
            if return_value:
                values.update(_split(value if device else dv.to_host(value), (B,), entries, start, scalar))
        if total is None:
            total = dv.torch().zeros((B,) + (len(self.params),) * rank, dtype=dv.torch().float64, device=dev)
        return self._values(params, values, cotangents, fixed, device) if return_value else None, total if device else dv.to_host(total), scalar

    def vjp(self, params, cotangents, device=False, return_value=False):
        """Vector-Jacobian product: the gradient with respect to the parameters of a scalar function of the outputs whose derivative with respect to
        them is ``cotangents``, for every point of a batch -- what ``jax.vjp`` / ``jax.grad`` of the reference's ``predict`` give, and what a
        gradient-based sampler wants of a log-likelihood.  ``params`` as in :meth:`predict`.  ``cotangents``: ``{varied key: array or tensor}``, each
        broadcastable to ``(B,) + shape`` of that output (``shape`` alone with scalar parameters).  A fixed key is accepted and contributes nothing (its
        derivative is zero), an unknown key raises ``KeyError``, an empty dictionary gives zeros.

        Returns ``{parameter name: (B,) array}`` in the order of ``Emulator.params``, ``sum over keys and entries of cotangent * d output / d parameter``
        (scalars if every parameter is a scalar).  Computed by reverse mode on the device (:meth:`MLPEmulatorEngine.vjp`,
        :meth:`TaylorEmulatorEngine.vjp`) without forming the Jacobian, on the columns of the cotangents' varied keys only (:meth:`_reverse`).  Host arrays by
        default; ``device=True``: the views ``G[:, i]`` of one (B, ndim) tensor, and no synchronisation with the device.  ``return_value=True``:
        ``(values, gradients)``, ``values`` what ``predict(params, device=device, keys=list(cotangents))`` returns."""
        values, total, scalar = self._reverse('vjp', 1, params, cotangents, device, return_value)
        grads = {name: (total[0, i] if scalar else total[:, i]) for i, name in enumerate(self.params)}
        return (values, grads) if return_value else grads

    def vjp2(self, params, cotangents, device=False, return_value=False):
        """Second derivatives of the varied outputs contracted with cotangents: the Hessian with respect to the parameters of ``sum cotangent * output`` at
        fixed cotangents, for every point of a batch -- the second-order part of what ``jax.hessian`` of a scalar function of the reference's ``predict``
        gives (with ``cotangents = w (data - y)`` the residual-curvature term of the Hessian of chi2, :meth:`chi2_hessian`).  ``params`` and ``cotangents``
        as in :meth:`vjp`, with its rules for fixed, unknown and no keys.

        Returns ``(B, ndim, ndim)`` in the order of ``Emulator.params`` (no leading axis if every parameter is a scalar),
        ``sum over keys and entries of cotangent * d^2 output / d parameter_i d parameter_j``, symmetric bit for bit.  Computed on the device
        (:meth:`MLPEmulatorEngine.vjp2`, :meth:`TaylorEmulatorEngine.vjp2`) without forming any second derivative of an output (:meth:`_reverse`).  Host
        array by default; ``device=True``: a torch tensor, and no synchronisation with the device.  ``return_value=True``: ``(values, matrices)``, ``values``
        what ``predict(params, device=device, keys=list(cotangents))`` returns."""
        values, total, scalar = self._reverse('vjp2', 2, params, cotangents, device, return_value)
        total = total[0] if scalar else total
        return (values, total) if return_value else total

    def _directions(self, tangents, B):
        """(T (B, ndim) or (B, K, ndim) float64, K or None) of ``tangents = {parameter name: value}``, a host array unless a tangent is a device tensor: a
        value of dimension <= 1 broadcasts against (B,) and is one direction, one of dimension 2 is (B or 1, K); a missing name is a zero component."""
        unknown = [name for name in tangents if name not in self.params]
        if unknown:
            raise KeyError('no parameter {}'.format(unknown))
        if all(not dv.is_torch(v) for v in tangents.values()):
            xp, values = np, {name: np.asarray(value, dtype='f8') for name, value in tangents.items()}
        else:
            xp = dv.torch()
            dev = self._device_of(*tangents.values())
            values = {name: dv.to_device(value, dev, cache=False) for name, value in tangents.items()}
            values[None] = xp.zeros((), dtype=xp.float64, device=dev)
        if any(v.ndim > 2 for v in values.values()):
            raise ValueError('a tangent is a scalar, (B,) or (B or 1, K)')
        counts = {int(v.shape[1]) for v in values.values() if v.ndim == 2}
        if len(counts) > 1:
            raise ValueError('tangents must share one count of directions, got {}'.format(sorted(counts)))
        K = counts.pop() if counts else None
        columns = []
        for name in self.params:
            v = values.get(name, values.get(None, np.zeros(())))
            columns.append(xp.broadcast_to(v.reshape(-1, 1) if K is not None and v.ndim == 1 else v, (B,) if K is None else (B, K)))
        return xp.stack(columns, -1), K

    def jvp(self, params, tangents, device=False, keys=None, return_value=False):
        """Jacobian-vector product: the derivative of the varied outputs along given directions in parameter space, for every point of a batch -- what
        ``jax.jvp`` / ``jax.linearize`` of the reference's ``predict`` give.  ``params`` as in :meth:`predict`.  ``tangents``:
        ``{parameter name: value}`` in raw-parameter units; a value of dimension <= 1 broadcasts against ``(B,)`` and gives one direction, a value of
        dimension 2 is ``(B or 1, K)``, K directions per point (all such values share one K).  A name that is no parameter raises ``KeyError``, a missing
        name is a zero component, an empty dictionary gives zeros.

        Returns ``{varied key: (B,) + shape}``, or ``{varied key: (B, K) + shape}`` with K directions,
        ``sum_i tangent_i d output / d parameter_i``, without the leading ``B`` axis if every parameter is a scalar.  Fixed outputs are not returned:
        their derivative is identically zero.  Computed by forward mode on the device (:meth:`MLPEmulatorEngine.jvp`,
        :meth:`TaylorEmulatorEngine.jvp`) without forming the Jacobian.  ``keys``: as in :meth:`predict` -- one call of the engine per maximal
        contiguous run of columns, and no other column is computed.  Host arrays by default; ``device=True``: torch tensors, views into the run's
        buffer, and no synchronisation with the device.  ``return_value=True``: ``(values, tangents_out)``, ``values`` what
        ``predict(params, device=device, keys=keys)`` returns."""
        X, B, scalar = self._points(params)
        plan = self._plan(keys)
        T, K = self._directions(tangents, B)
        return self._forward('jvp', X, scalar, plan, keys, device, [(B,)] * bool(return_value) + [(B,) if K is None else (B, K)], T, return_value=return_value)

    def jvp2(self, params, tangents, tangents2=None, device=False, keys=None, return_value=False, return_first=False):
        """Second directional derivatives of the varied outputs along pairs of directions in parameter space, for every point of a batch -- what
        ``jax.jvp`` of ``jax.jvp`` of the reference's ``predict`` gives: ``sum_ij tangent_i tangent2_j d^2 output / d parameter_i d parameter_j``.
        ``params`` and the two dictionaries of tangents as in :meth:`jvp` (scalars, ``(B,)`` or ``(B or 1, K)`` values; a missing name is a zero
        component, a name that is no parameter raises ``KeyError``); both share one K.  ``tangents2=None``: the second directional derivative along
        ``tangents`` (the ``r''(v, v)`` of geodesic acceleration).

        Returns ``{varied key: (B,) + shape}``, or ``{varied key: (B, K) + shape}`` with K pairs, without the leading ``B`` axis if every parameter is a
        scalar.  Fixed outputs are not returned.  Computed by second-order forward mode on the device (:meth:`MLPEmulatorEngine.jvp2`,
        :meth:`TaylorEmulatorEngine.jvp2`), a row per (point, pair): no Hessian is formed, and exchanging the two dictionaries gives the same bits.
        ``keys``: as in :meth:`predict` -- one call of the engine per maximal contiguous run of columns.  Host arrays by default; ``device=True``: torch
        tensors, views into the run's buffer, and no synchronisation with the device.  ``return_value=True``: the values of
        ``predict(params, device=device, keys=keys)`` are prepended; ``return_first=True``: what :meth:`jvp` gives along ``tangents`` (and along
        ``tangents2``, where given) is inserted before the result."""
        X, B, scalar = self._points(params)
        plan = self._plan(keys)
        T, K = self._directions(tangents, B)
        T2 = None
        if tangents2 is not None:
            T2, K2 = self._directions(tangents2, B)
            if K2 != K:
                raise ValueError('tangents and tangents2 must share one count of directions, got {} and {}'.format(K, K2))
        nfirst = (2 if T2 is not None else 1) if return_first else 0
        leads = [(B,)] * bool(return_value) + [(B,) if K is None else (B, K)] * (nfirst + 1)
        return self._forward('jvp2', X, scalar, plan, keys, device, leads, T, T2, return_value=return_value, return_first=return_first)

    def hessian(self, params, device=False, keys=None):
        """Second derivatives of the varied outputs with respect to the parameters at ``params`` (as in :meth:`predict`) -- what ``jax.hessian`` of the
        reference's ``predict`` gives: ``{key: array (B, ndim, ndim) + shape}``, both ``ndim`` axes in the order of ``Emulator.params``, without the
        leading ``B`` axis if every parameter is a scalar.  One :meth:`jvp2` call on the ``ndim (ndim + 1) / 2`` pairs of unit directions ``i <= j``,
        mirrored: symmetric bit for bit.  Fixed outputs are not returned.  ``keys``, ``device``: as in :meth:`jvp2`."""
        names = list(self.params)
        ndim = len(names)
        pairs = [(i, j) for i in range(ndim) for j in range(i, ndim)]
        units = [{name: np.array([[float(pair[side] == n) for pair in pairs]]) for n, name in enumerate(names)} for side in range(2)]
        X, B, scalar = self._points(params)
        out = self.jvp2(params, units[0], units[1], device=device, keys=keys)
        index = np.zeros((ndim, ndim), dtype='i8')
        for p, (i, j) in enumerate(pairs):
            index[i, j] = index[j, i] = p
        toret = {}
        axis = 0 if scalar else 1
        for key, block in out.items():      # (B, npairs) + shape, or (npairs,) + shape
            if device:      # (views stacked: no index array goes to the device)
                full = dv.torch().stack([block.select(axis, int(p)) for p in index.ravel()], dim=axis)
            else:
                full = np.take(block, index.ravel(), axis=axis)
            toret[key] = full.reshape(tuple(block.shape[:axis]) + (ndim, ndim) + tuple(block.shape[axis + 1:]))
        return toret

    def gauss_newton(self, params, weights, data=None, device=False, return_value=False, precision=None):
        """Fisher matrices and Gauss-Newton normal equations of a weighted least-squares fit of ``data`` to the emulated outputs, for every point of a batch,
        with ``J`` the Jacobian of :meth:`jacobian` and ``y`` the prediction: ``fisher[b, i, j] = sum w J_i J_j``,
        ``gradient[b, i] = sum w (data - y) J_i``, ``chi2[b] = sum w (data - y)^2``, the sums over the entries of the outputs that ``weights`` names.
        A Levenberg-Marquardt step solves ``(F + lambda diag F) delta = g``: ``g = -1/2 d chi2 / d theta`` and ``F`` is the Gauss-Newton half Hessian
        (:meth:`least_squares` runs such fits on the device).
        ``params`` as in :meth:`predict`.  ``weights`` (inverse variances) and ``data``: ``{varied key: array or tensor}``, each broadcastable to
        ``(B,) + shape`` of that output (``shape`` alone with scalar parameters), as :meth:`vjp` takes its cotangents.  A weight of exactly 0 drops its entry,
        whatever the data or the emulator hold there (NaN included): a mask.  The keys of ``weights`` select the outputs: a fixed key is accepted and
        contributes nothing, an unknown key raises ``KeyError``, an empty dictionary gives zeros; a key of ``data`` that is not in ``weights`` raises
        ``KeyError``, a varied key of ``weights`` missing from a given ``data`` ``ValueError``.

        Returns ``fisher`` (B, ndim, ndim) in the order of ``Emulator.params`` (no leading axis if every parameter is a scalar), or with ``data``
        ``(fisher, gradient, chi2)``, ``gradient`` ``{parameter name: (B,)}`` as :meth:`vjp` returns its gradients and ``chi2`` (B,).  Computed on the
        device without forming the Jacobian (:meth:`MLPEmulatorEngine.gauss_newton`, :meth:`TaylorEmulatorEngine.gauss_newton`), on the columns of the
        varied keys of ``weights`` only.  Host arrays by default; ``device=True``: torch tensors, and no synchronisation with the device.
        ``return_value=True``: the values are prepended, what ``predict(params, device=device, keys=list(weights))`` returns.

        ``precision``: a dense precision matrix, ``chi2 = r^T P r`` with ``r = data - y``, ``fisher = J P J^T``, ``gradient = J P r``.  ``weights`` is then
        the sequence of the distinct varied keys the data vector is made of -- those outputs flattened in C order and concatenated in the listed order, N
        entries -- (a dictionary raises ``TypeError``, a fixed or unknown key ``KeyError``), ``precision`` (N, N), symmetric, a host array or a device tensor,
        shared by all points (another shape: ``ValueError``), ``data`` ``{key: ...}`` for exactly those keys.  A column with ``precision[c, c] == 0`` is
        dropped whatever it holds.  The engine's ``jacobian`` writes the (B, ndim, N) Jacobian run by run and :func:`gauss_newton_dense` contracts it in
        one GEMM on the matrix cores.  Returns, ``device=`` and ``return_value=`` as above.  The staging and the evaluation of both routes: ``_Chi2``."""
        X, B, scalar = self._points(params)
        objective = _Chi2(self, weights, data, precision, X, B)
        out = objective.evaluate(X, return_value=return_value)
        values, totals = out if return_value else (None, out)
        return self._normal_equations(objective, params, totals, values, scalar, device)

    def _normal_equations(self, objective, params, totals, values, scalar, device):
        """What :meth:`gauss_newton` and :meth:`chi2_hessian` return of an evaluation of ``objective`` at ``params``: of the device tensors ``totals``, the
        matrix (B, ndim, ndim), then with data the gradient by parameter name and chi2; before them, where ``values`` (per run, (B, stop - start)) is not
        None, what ``predict(params, device=device, keys=...)`` returns for the keys of the objective.  Host arrays unless ``device``, no leading axis if
        ``scalar``; a single result as it is."""
        if not device:
            totals = tuple(dv.to_host(total) for total in totals)
        toret = (totals[0][0] if scalar else totals[0],)
        if len(totals) > 1:
            toret += ({name: (totals[1][0, i] if scalar else totals[1][:, i]) for i, name in enumerate(self.params)}, totals[2][0] if scalar else totals[2])
        if values is not None:
            split = {}
            for (start, stop, entries), block in zip(objective.runs, values):
                split.update(_split(block if device else dv.to_host(block.contiguous()), (objective.B,), entries, start, scalar))
            toret = (self._values(params, split, objective.keys, objective.fixed, device),) + toret
        return toret[0] if len(toret) == 1 else toret

    def chi2_hessian(self, params, weights, data, device=False, precision=None, return_value=False):
        """The full half Hessian of chi2 of a weighted least-squares fit of ``data`` to the emulated outputs, for every point of a batch:
        ``(hessian, gradient, chi2)`` with ``gradient`` and ``chi2`` those of ``gauss_newton(params, weights, data=data, precision=precision)``, bit for
        bit, and ``hessian = fisher - vjp2(q)`` (B, ndim, ndim) ``= 1/2 d^2 chi2 / d theta d theta``: the Gauss-Newton half Hessian minus the
        residual-curvature term ``sum_c q_c d^2 y_c``, so that ``d gradient_i / d theta_j = -hessian_ij`` -- what ``jax.hessian`` of the reference's
        ``1/2 chi2(predict(theta))`` gives, for Newton steps, Laplace approximations and Riemannian samplers where the residuals are not small.
        ``params``, ``weights``, ``data``, ``precision`` and their argument rules as in :meth:`gauss_newton`.  One evaluation gives the value, the Fisher
        matrix, the gradient and chi2; the cotangent of the residuals is formed on the device: with diagonal weights ``q = w (data - y)``, exactly 0 where
        ``w == 0`` (a select: NaN data under a zero weight stay masked); with ``precision`` ``q = (data - y) P``, the columns with ``P[c, c] == 0``
        dropped as :func:`gauss_newton_dense` drops them; then the engine's ``vjp2`` of it, run by run.  Host arrays by default (no leading axis if every parameter is a
        scalar); ``device=True``: torch tensors, and no synchronisation with the device.  ``return_value=True``: the values are prepended."""
        X, B, scalar = self._points(params)
        objective = _Chi2(self, weights, data, precision, X, B)
        values, (fisher, gradient, chi2) = objective.evaluate(X, return_value=True)
        residuals = [block - value for block, value in zip(objective.data, values)]
        hessian = fisher - objective.pull('vjp2', X, objective.cotangent(residuals), 2)
        return self._normal_equations(objective, params, (hessian, gradient, chi2), values if return_value else None, scalar, device)

    def _box(self, bounds, X, dev):
        """``(lo, hi, x)``: the box ``bounds = {name: (lo, hi)}`` of :meth:`least_squares` and :meth:`hmc` -- by default, and for the names it leaves out,
        the limits of ``Emulator.params``; a name that is no parameter raises ``KeyError`` -- as (ndim,) tensors on ``dev``, and the start ``X`` clipped to it."""
        limits = dict(self.params)
        if bounds is not None:
            unknown = [name for name in bounds if name not in limits]
            if unknown:
                raise KeyError('no parameter {}'.format(unknown))
            limits.update({name: tuple(limit) for name, limit in bounds.items()})
        lo, hi = (dv.to_device(np.array([limits[name][side] for name in self.params], dtype='f8'), dev) for side in (0, 1))
        return lo, hi, dv.torch().clamp(dv.to_device(X, dev, cache=False), min=lo, max=hi)

    def least_squares(self, params, weights, data, bounds=None, niterations=20, lambda0=1e-3, lambda_up=10., lambda_down=0.1, lambda_min=1e-12, lambda_max=1e12,
                      ftol=1e-8, device=False, precision=None, geodesic=False, alpha=0.75):
        """B weighted least-squares fits of ``data`` to the emulated outputs at once, by Levenberg-Marquardt on the device: ``niterations`` times
        :meth:`gauss_newton` at the trial points, then :func:`lm_step` (one launch: acceptance, the damping of each fit, the active set of the box, the
        damped Cholesky solve, the stopping rule).  ``params``: the start, as :meth:`predict` takes it (scalars or arrays of B values); ``weights``,
        ``data``: as :meth:`gauss_newton` takes them, with the same ``KeyError`` / ``ValueError`` rules (their broadcast blocks are staged once, not per
        iteration).  ``bounds``: ``{name: (lo, hi)}``, by default the limits of ``Emulator.params`` -- the box the emulator was trained on --, infinite
        where open; the start is clipped to them.  ``lambda0``: the first damping of ``(F + lambda diag F) delta = g``; the other controls are those of
        :func:`lm_step`.  The count of iterations is fixed and a fit that is over (``status``: 1 converged by ``ftol``, 2 stalled at ``lambda_max``, 3 no
        finite start or no positive-definite system) is left alone by the later steps: nothing is tested on the host.

        Returns ``(best, chi2, info)``: ``best`` ``{parameter name: (B,)}`` the best point met, ``chi2`` (B,) there, ``info`` a dictionary of ``fisher``
        (B, ndim, ndim) and ``gradient`` ``{name: (B,)}`` there (the bits :meth:`gauss_newton` returns at ``best``), ``covariance`` (the inverse of the
        undamped ``fisher`` by :func:`spd_inverse`, NaN where it is not positive definite), ``status``, ``naccepted`` and ``lambda`` (B,); no leading
        axis if every parameter is a scalar.  Host arrays by default; ``device=True``: torch tensors, and no synchronisation with the device anywhere.

        ``precision``: a dense precision matrix (N, N), ``weights`` then the sequence of the keys its rows and columns follow, as :meth:`gauss_newton` takes
        them.  It is permuted and staged once; an iteration is the engine's ``jacobian`` calls, :func:`gauss_newton_dense` and :func:`lm_step`, and
        ``info['covariance']`` the inverse of the dense-precision Fisher matrix.

        ``geodesic=True``: geodesic acceleration (Transtrum & Sethna 2012) of every step.  After :func:`lm_step` (which then also returns the velocity
        ``v`` it solved) an iteration takes ``h = J W y''(v, v)`` at the accepted point (``_Chi2.curvature``: the engine's ``jvp2``, a row per fit, the
        cotangent of that under the weights or the precision, and the engine's ``vjp`` of it); then :func:`lm_accelerate` takes
        ``x + v + a / 2`` with ``a = -(F + lambda diag F)^-1 h`` where ``2 |a| / |v| <= alpha`` and the plain step elsewhere.  ``info`` then also holds
        ``naccelerated`` (B,), the count of corrections each fit took.  ``alpha`` must be finite and positive (``ValueError``)."""
        X, B, scalar = self._points(params)
        torch = dv.torch()
        if data is None:
            raise ValueError('least_squares needs data')
        objective = _Chi2(self, weights, data, precision, X, B)
        names = list(self.params)
        lo, hi, x = self._box(bounds, X, objective.dev)
        state = lm_state(x, lambda0=lambda0)
        controls = dict(lambda_up=lambda_up, lambda_down=lambda_down, lambda_min=lambda_min, lambda_max=lambda_max, ftol=ftol)
        if geodesic:
            alpha = float(alpha)
            if not (0. < alpha < float('inf')):
                raise ValueError('alpha must be finite and positive, got {}'.format(alpha))
            naccelerated = torch.zeros((B,), dtype=torch.int32, device=objective.dev)
        for iteration in range(int(niterations)):
            trial = dict(zip(LM_TRIAL, (x,) + objective.evaluate(x)))
            if not geodesic:
                x = lm_step(state, trial, lo, hi, **controls)
                continue
            x, velocity = lm_step(state, trial, lo, hi, return_velocity=True, **controls)
            x = lm_accelerate(state, velocity, objective.curvature(state['x'], velocity), lo, hi, alpha=alpha, naccelerated=naccelerated)
        covariance = spd_inverse(state['fisher'])[0]
        out = dict(state, covariance=covariance)
        if geodesic:
            out['naccelerated'] = naccelerated
        if not device:
            out = {name: dv.to_host(value) for name, value in out.items()}
        if scalar:
            out = {name: value[0] for name, value in out.items()}
        best = {name: out['x'][..., i] for i, name in enumerate(names)}
        info = {name: out[name] for name in ('fisher', 'covariance', 'status', 'naccepted', 'lambda') + (('naccelerated',) if geodesic else ())}
        info['gradient'] = {name: out['gradient'][..., i] for i, name in enumerate(names)}
        return best, out['chi2'], info

    def hmc(self, params, weights, data, nsamples=100, nwarmup=20, thin=1, nleapfrog=6, step_size=0.25, jitter=0.1, metric=None, bounds=None, seed=42, device=False,
            precision=None):
        """B independent Hamiltonian Monte Carlo chains of ``exp(-chi2 / 2)`` inside the box, on the device: one :meth:`gauss_newton` evaluation and one
        launch of :func:`hmc_step` per leapfrog step (kick, drift and box test; at the end of a trajectory also the accept / reject, the sample and the
        momenta of the next one, drawn by a counter-based generator in the kernel).  Nothing is tested on the host.  ``params``: the start, as
        :meth:`predict` takes it (scalars or arrays of B values); ``weights``, ``data``, ``precision``, ``bounds``: as :meth:`least_squares` takes them, with
        the same errors; they are staged once, and the start is clipped to the box.  ``metric``: the mass matrix, (ndim, ndim) or (B, ndim, ndim) in the
        order of ``Emulator.params`` (e.g. ``least_squares(...)[2]['fisher']``; another shape: ``ValueError``); by default the Fisher matrix
        :meth:`gauss_newton` returns at the start, per chain.  ``step_size``: a scalar or (B,), in units of the coordinates the metric whitens: 0.25 x 6
        steps, about pi / 2, is a quarter period of a Gaussian target under its own Fisher metric; every trajectory multiplies it by
        ``1 + jitter (2 u - 1)``, ``0 <= jitter < 1``.  The run is ``nwarmup + nsamples thin`` trajectories of ``nleapfrog`` steps; the state after every
        ``thin``-th trajectory past the warm-up is a sample.  A trajectory that leaves the box is rejected (exact for a target that is zero outside it):
        the chain waits at its last point inside, and the emulator is never evaluated outside the box.  A chain whose start has no finite ``chi2``, whose
        metric is not positive definite or whose step size is not finite and positive has ``status = 3`` and stays at its start.  The same ``seed`` gives
        the same bits, whatever B.

        Returns ``(samples, chi2, info)``: ``samples`` ``{parameter name: (nsamples, B)}``, ``chi2`` (nsamples, B) there, ``info`` a dictionary of
        ``naccepted``, ``nout`` (the trajectories that left the box), ``status`` (B,), ``acceptance`` (``naccepted`` over the number of trajectories),
        ``metric`` (B, ndim, ndim) and ``step_size`` (B,); no batch axis if every parameter is a scalar.  Host arrays by default; ``device=True``: torch
        tensors, and no synchronisation with the device anywhere."""
        X, B, scalar = self._points(params)
        torch = dv.torch()
        if data is None:
            raise ValueError('hmc needs data')
        nsamples, nwarmup, thin, nleapfrog = int(nsamples), int(nwarmup), int(thin), int(nleapfrog)
        if nsamples < 1 or nwarmup < 0 or thin < 1 or nleapfrog < 1:
            raise ValueError('nsamples, thin and nleapfrog must be at least 1 and nwarmup at least 0, got {:d}, {:d}, {:d} and {:d}'.format(nsamples, thin, nleapfrog, nwarmup))
        jitter = float(jitter)
        if not (0. <= jitter < 1.):
            raise ValueError('jitter must be in [0, 1), got {}'.format(jitter))
        names = list(self.params)
        ndim = len(names)
        if metric is not None and tuple(np.shape(metric)) not in ((ndim, ndim), (B, ndim, ndim)):
            raise ValueError('metric must be of shape {} or {}, got {}'.format((ndim, ndim), (B, ndim, ndim), tuple(np.shape(metric))))
        objective = _Chi2(self, weights, data, precision, X, B)
        dev = objective.dev
        lo, hi, x = self._box(bounds, X, dev)
        fisher, gradient, chi2 = objective.evaluate(x)
        state = hmc_state(x, gradient, chi2)
        if metric is None:
            metric = fisher
        else:
            metric = dv.to_device(metric, dev)
            metric = (metric.expand(B, ndim, ndim) if metric.ndim == 2 else metric).contiguous()
        factor = hmc_factor(metric, state['status'])
        step = _hmc_step_size(step_size, B, dev)
        ntrajectories = nwarmup + nsamples * thin
        samples, samples_chi2 = torch.empty((nsamples, B, ndim), dtype=torch.float64, device=dev), torch.empty((nsamples, B), dtype=torch.float64, device=dev)
        controls = dict(jitter=jitter, seed=seed)
        x = hmc_step(state, {name: state[name] for name in HMC_TRIAL}, factor, lo, hi, step, t_open=0, **controls)
        for t in range(ntrajectories):
            for leap in range(nleapfrog):
                trial = dict(zip(HMC_TRIAL, (x,) + objective.evaluate(x)[1:]))
                if leap < nleapfrog - 1:
                    x = hmc_step(state, trial, factor, lo, hi, step, **controls)
                    continue
                s, rest = divmod(t - nwarmup + 1, thin)
                record = t >= nwarmup and rest == 0
                x = hmc_step(state, trial, factor, lo, hi, step, t_close=t, t_open=t + 1 if t + 1 < ntrajectories else None,
                             sample=samples[s - 1] if record else None, sample_chi2=samples_chi2[s - 1] if record else None, **controls)
        out = {'samples': samples, 'chi2': samples_chi2, 'naccepted': state['naccepted'], 'nout': state['nout'], 'status': state['status'],
               'acceptance': state['naccepted'].to(torch.float64) / ntrajectories, 'metric': metric, 'step_size': step}
        if not device:
            out = {name: dv.to_host(value) for name, value in out.items()}
        if scalar:
            out = {name: (value[:, 0] if name in ('samples', 'chi2') else value[0]) for name, value in out.items()}
        samples = {name: out['samples'][..., i] for i, name in enumerate(names)}
        return samples, out['chi2'], {name: out[name] for name in ('naccepted', 'nout', 'status', 'acceptance', 'metric', 'step_size')}

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
            from .taylor import TaylorEmulatorEngine
            new.engine = TaylorEmulatorEngine.from_state(state['engine'], device=device)
        else:
            raise NotImplementedError('engine {} (only the Taylor and MLP engines are built)'.format(name))
        new.varied_keys, new.varied_shapes, new.fixed = list(state['varied_keys']), [tuple(s) for s in state['varied_shapes']], dict(state['fixed'])
        return new
