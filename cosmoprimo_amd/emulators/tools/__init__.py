"""Emulation tools under the reference's names (cosmoprimo/emulators/tools): the finite-difference and quasi Monte-Carlo samplers, the ``Emulator``
front end, the Taylor-expansion engine and the multi-layer perceptron engine."""
from .samples import DiffSampler, QMCSampler, Samples, deriv_ncoeffs, rqrs_points
from .base import Emulator, column_runs, gauss_newton_dense, hmc_factor, hmc_state, hmc_step, lm_accelerate, lm_state, lm_step, spd_inverse
from .taylor import TaylorEmulatorEngine, fd_weights, taylor_operator
from .mlp import MLPEmulatorEngine

__all__ = ['DiffSampler', 'QMCSampler', 'Samples', 'Emulator', 'TaylorEmulatorEngine', 'MLPEmulatorEngine', 'deriv_ncoeffs', 'fd_weights', 'taylor_operator', 'rqrs_points', 'column_runs', 'gauss_newton_dense', 'lm_state', 'lm_step', 'lm_accelerate', 'spd_inverse', 'hmc_state', 'hmc_factor', 'hmc_step']
