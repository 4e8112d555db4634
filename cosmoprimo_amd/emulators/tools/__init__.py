"""Emulation tools under the reference's names (cosmoprimo/emulators/tools): the finite-difference sampler and the Taylor-expansion engine."""
from .samples import DiffSampler, Samples, deriv_ncoeffs
from .taylor import Emulator, TaylorEmulatorEngine, fd_weights, taylor_operator

__all__ = ['DiffSampler', 'Samples', 'Emulator', 'TaylorEmulatorEngine', 'deriv_ncoeffs', 'fd_weights', 'taylor_operator']
