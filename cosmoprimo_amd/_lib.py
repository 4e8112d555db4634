"""ctypes binding of libcosmoprimo_amd.so (C ABI declared in include/cosmoprimo_amd.h).

The library is the product: there is no Python/CPU fallback.  If it is missing (or its ABI does
not match) importing any compute entry point raises, loudly.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libcosmoprimo_amd.so')
ABI_VERSION = 5

CP_OK, CP_EINVAL, CP_EUNSUPPORTED, CP_EDEVICE, CP_ENOMEM = range(5)
EXTRAP_CONSTANT, EXTRAP_EDGE, EXTRAP_LOGLOG = range(3)
(KERNEL_BESSEL_J, KERNEL_SPHERICAL_BESSEL_J, KERNEL_TOPHAT, KERNEL_TOPHAT_SQ, KERNEL_GAUSSIAN, KERNEL_GAUSSIAN_SQ) = range(6)
KERNEL_CUSTOM = 100


class FFTlogSpec(ctypes.Structure):
    """cp_fftlog_spec (include/cosmoprimo_amd.h): kernel, tilt and convention of one transform of a plan."""
    _fields_ = [('kind', ctypes.c_int), ('param', ctypes.c_double), ('q', ctypes.c_double), ('xy', ctypes.c_double), ('pre_power', ctypes.c_double),
                ('pre_const', ctypes.c_double), ('post_sign', ctypes.c_double)]


_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int_p = ctypes.POINTER(ctypes.c_int)

# name -> (restype, argtypes); every symbol of include/cosmoprimo_amd.h
SIGNATURES = {
    'cp_abi_version': (ctypes.c_int, []),
    'cp_last_error': (ctypes.c_char_p, []),
    'cp_device_count': (ctypes.c_int, []),
    'cp_loggamma': (ctypes.c_int, [_c_double_p, _c_double_p, ctypes.c_longlong]),
    'cp_gamma': (ctypes.c_int, [_c_double_p, _c_double_p, ctypes.c_longlong]),
    'cp_kernel_eval': (ctypes.c_int, [ctypes.c_int, ctypes.c_double, _c_double_p, _c_double_p, ctypes.c_longlong]),
    'cp_fftlog_padded_size': (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    'cp_fftlog_tables': (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _c_double_p, ctypes.POINTER(FFTlogSpec), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       _c_double_p, _c_double_p] + [_c_double_p] * 8),
    'cp_fftlog_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_double_p,
                                            _c_double_p, _c_double_p, ctypes.c_int]),
    'cp_fftlog_execute': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double,
                                        ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]),
    'cp_fftlog_execute_window': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double,
                                               ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_fftlog_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_fftlog_plan_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, _c_int_p, _c_int_p, _c_int_p]),
    'cp_background_distance': (ctypes.c_int, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_derived_parameters': (ctypes.c_int, [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    'cp_background_knots': (ctypes.c_int, [_c_double_p, ctypes.c_int]),
    'cp_background_init': (ctypes.c_int, [ctypes.c_int]),
    'cp_distance_from_radial': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    'cp_ncdm_knots': (ctypes.c_int, [_c_double_p, ctypes.c_int]),
    'cp_growth_ode_knots': (ctypes.c_int, [_c_double_p, ctypes.c_int]),
    'cp_growth_ode_tables': (ctypes.c_int, [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p]),
    'cp_ncdm_tables': None,        # filled below (takes cp_param by value)
    'cp_background_eval': (ctypes.c_int, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_power_workspace_bytes': (ctypes.c_longlong, [ctypes.c_longlong]),
    'cp_rfft_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int]),
    'cp_rfft_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_rfft_forward': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]),
    'cp_rfft_backward': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]),
    'cp_sigma_rz_workspace_bytes': (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int]),
    'cp_sigma_rz_fused_available': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    'cp_geospline_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _c_double_p, ctypes.c_int, _c_double_p, ctypes.c_int, ctypes.c_int]),
    'cp_geospline_plan_create_prefiltered': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, _c_double_p, _c_double_p, _c_double_p,
                                                           _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_int]),
    'cp_geospline_basis': (ctypes.c_int, [ctypes.c_double, _c_double_p]),
    'cp_geospline_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_geospline_plan_info': (ctypes.c_int, [ctypes.c_void_p, _c_int_p, _c_int_p, _c_int_p]),
    'cp_fftlog_geospline_execute': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                                  ctypes.c_int, ctypes.c_void_p]),
    'cp_fftlog_spline_execute': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]),
    'cp_spline_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _c_double_p, ctypes.c_int, _c_double_p, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    'cp_linop_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.c_int, _c_double_p, ctypes.c_int]),
    'cp_spline_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]),
    'cp_spline_apply_grouped': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]),
    'cp_spline_apply_outer': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                            ctypes.c_double, ctypes.c_void_p]),
    'cp_linop_apply_mid': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_double,
                                         ctypes.c_void_p]),
    'cp_tables_rows_available': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    'cp_tables_rows': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]),
    'cp_spline_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_spline_plan_info': (ctypes.c_int, [ctypes.c_void_p, _c_int_p, _c_int_p, _c_int_p]),
    'cp_spline_plan_columns': (ctypes.c_int, [ctypes.c_void_p, _c_int_p, _c_int_p]),
    'cp_spline_columns_scratch_doubles': (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int]),
    'cp_spline_rows_at_queries': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_spline_columns': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    'cp_wallish_box': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_void_p]),
    'cp_wallish_dd_box': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    'cp_splice_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _c_double_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int, _c_double_p, ctypes.c_int]),
    'cp_splice_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    'cp_splice_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_splice_plan_scheme': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_math_eval': (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p]),
    'cp_splice_plan_set_scheme': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    'cp_splice_plan_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    'cp_spline_rows_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_double_p,
                                                 ctypes.c_int]),
    'cp_spline_rows_plan_info': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_int)]),
    'cp_spline_rows_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.c_void_p]),
    'cp_spline_rows_second_derivatives': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]),
    'cp_spline_rows_pairs': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p]),
    'cp_spline_rows_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_tables_rows_direct': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                            ctypes.c_double, ctypes.c_void_p]),
    'cp_gap_spline': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_wallish_finish': (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_brieden_ratio': (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_brieden_knots': (ctypes.c_int, [ctypes.c_void_p] * 5 + [ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_void_p]),
    'cp_brieden_finish': (ctypes.c_int, [ctypes.c_void_p] * 3 + [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_brieden_resample': (ctypes.c_int, [ctypes.c_void_p] * 6 + [ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_brieden_smooth': (ctypes.c_int, [ctypes.c_void_p] * 7 + [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_dst_plan_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, _c_double_p, ctypes.c_int]),
    'cp_dst_execute': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_bilinear_pairs': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_int, ctypes.c_void_p]),
    'cp_interp_linear': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int,
                                        ctypes.c_void_p]),
    'cp_interp_table_create': (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), ctypes.c_longlong, _c_double_p, _c_double_p, ctypes.c_int]),
    'cp_interp_table_law': (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]),
    'cp_interp_table_apply': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]),
    'cp_interp_table_apply_f32': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p]),
    'cp_interp_table_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_spline_points': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    'cp_rows_screen': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p]),
    'cp_dst_plan_destroy': (ctypes.c_int, [ctypes.c_void_p]),
    'cp_dst_forward_analytic_workspace_bytes': (ctypes.c_longlong, [ctypes.c_longlong]),
    'cp_wallish_tail': (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    'cp_spline_operator': (ctypes.c_int, [ctypes.c_int, _c_double_p, ctypes.c_int, _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_double_p,
                                         _c_int_p]),
}


class cp_param(ctypes.Structure):
    """A per-cosmology parameter: device array (ptr) or broadcast value (include/cosmoprimo_amd.h)."""
    _fields_ = [('ptr', ctypes.c_void_p), ('value', ctypes.c_double)]


class cp_ncdm(ctypes.Structure):
    """Massive-neutrino spline tables of the background kernels (include/cosmoprimo_amd.h)."""
    _fields_ = [('nspecies', ctypes.c_int), ('species', ctypes.c_int), ('tab', ctypes.c_void_p)]


SIGNATURES['cp_ncdm_tables'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, cp_param, cp_param, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                               _c_double_p, _c_double_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
SIGNATURES['cp_kirkby2013_rows'] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_void_p, ctypes.c_longlong, _c_double_p, _c_double_p, ctypes.c_int, ctypes.c_void_p])
SIGNATURES['cp_spline_tables_build'] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_int, ctypes.c_void_p])
for _name in ('cp_spline_tables_apply', 'cp_spline_tables_apply_f32'):
    SIGNATURES[_name] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, _c_int_p, ctypes.c_int, ctypes.c_void_p])
# the leading arguments that the emulator entry points share, and their last two
_TAYLOR_HEAD = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]      # d_x, B, d_center, d_powers, ndim, T, max_power, d_derivatives, M
_MLP_HEAD = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _c_int_p, _c_int_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int]      # d_x, B, ndim, nlayers, widths, activations, M, d_params, the four operations, yfunction
_RANGE = [ctypes.c_longlong, ctypes.c_longlong]            # col0, ncols
_ARRAY = [ctypes.c_void_p, ctypes.c_longlong]              # a device array and its row stride
_WHERE = [ctypes.c_int, ctypes.c_void_p]                   # device, stream
# the run that the entry points taking a batch of cosmologies share (_device.pack_cosmologies makes it): ncosmo, bg_params, second_is_omega_m, ncdm -- and pk_params
_BG_BATCH = [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
_BATCH = _BG_BATCH + [ctypes.c_void_p]
_ENGINE_BATCH = [ctypes.c_int] + _BATCH                    # engine in front
_MARGINS = [ctypes.c_int] * 4                              # margin_first, margin_second, offset_first, offset_second
SIGNATURES['cp_power_eval'] = (ctypes.c_int, [ctypes.c_int] + _ENGINE_BATCH + [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong] +
                               [ctypes.c_void_p] * 3 + _WHERE)      # engine, what; nk, d_k, d_kscale, nz, d_z, d_out, d_work
SIGNATURES['cp_power_eval_variants'] = (ctypes.c_int, [ctypes.c_int, ctypes.c_int] + _BATCH + [ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p,
                                                                                               ctypes.c_void_p] + _WHERE)      # what, of; nk, d_k, nz, d_z, d_out
SIGNATURES['cp_eh_scalars'] = SIGNATURES['cp_variants_scalars'] = (ctypes.c_int, _BG_BATCH + [ctypes.c_void_p] + _WHERE)
_SIGMA_HEAD = _ENGINE_BATCH + [ctypes.c_int, ctypes.c_void_p]      # ... nk, d_k
_SIGMA_TAIL = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3      # d_growth_sq, nz, d_out, d_pk_out, d_work
SIGNATURES['cp_sigma_rz_analytic'] = (ctypes.c_int, _SIGMA_HEAD + [ctypes.c_void_p, ctypes.c_void_p] + _SIGMA_TAIL + [ctypes.c_int] + _WHERE)      # fftlog, spline; nblocks
SIGNATURES['cp_sigma_rz_analytic_prefiltered'] = (ctypes.c_int, _SIGMA_HEAD + [ctypes.c_void_p] + _SIGMA_TAIL + _WHERE)      # spline
SIGNATURES['cp_sigma_rz_functional'] = (ctypes.c_int, _SIGMA_HEAD + [ctypes.c_void_p, ctypes.c_int] + _SIGMA_TAIL + _WHERE)      # d_functional, nq
SIGNATURES['cp_sigma8_normalise'] = (ctypes.c_int, _SIGMA_HEAD + [ctypes.c_void_p, cp_param] + [ctypes.c_void_p] * 4 + _WHERE)      # d_functional, sigma8; d_rsigma8, d_amplitude, d_pk_out, d_work
SIGNATURES['cp_dst_forward_analytic'] = (ctypes.c_int, [ctypes.c_void_p] + _ENGINE_BATCH + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])      # plan; d_out, d_work, flags, stream
SIGNATURES['cp_dst_forward_analytic_box'] = (ctypes.c_int, [ctypes.c_void_p] + _ENGINE_BATCH + [ctypes.c_void_p] * 3 + _MARGINS + [ctypes.c_void_p])      # plan; d_out, d_work, d_box
SIGNATURES['cp_wallish_full'] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p] + _ENGINE_BATCH + [ctypes.c_void_p, ctypes.c_int] + _MARGINS +
                                 [ctypes.c_void_p] * 6)      # plans; d_pk, npk; d_tophat, d_box, d_coef, d_out, d_work, stream
SIGNATURES['cp_taylor_predict'] = (ctypes.c_int, _TAYLOR_HEAD + [ctypes.c_void_p] + _WHERE)
SIGNATURES['cp_taylor_predict_columns'] = (ctypes.c_int, _TAYLOR_HEAD + _RANGE + _ARRAY + _WHERE)
SIGNATURES['cp_taylor_jacobian'] = (ctypes.c_int, _TAYLOR_HEAD + _RANGE + _ARRAY + _WHERE)
SIGNATURES['cp_taylor_vjp'] = (ctypes.c_int, _TAYLOR_HEAD + _RANGE + _ARRAY + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong] + _WHERE)      # d_cot, ldc; d_grad, d_work, work_doubles
SIGNATURES['cp_taylor_vjp2'] = SIGNATURES['cp_taylor_vjp']      # d_hess in the place of d_grad
SIGNATURES['cp_taylor_jvp'] = (ctypes.c_int, _TAYLOR_HEAD + _RANGE + _ARRAY + _ARRAY + _WHERE)      # d_tan, K; d_out, ldo
SIGNATURES['cp_taylor_jvp2'] = (ctypes.c_int, _TAYLOR_HEAD + _RANGE + [ctypes.c_void_p] + _ARRAY + _ARRAY + _WHERE)      # d_tan_u; d_tan_v, K; d_out, ldo
_GN_TAIL = _ARRAY + _ARRAY + _ARRAY + [ctypes.c_void_p] * 4 + [ctypes.c_longlong]      # d_weights, ldw; d_data, ldd; d_value, ldv; d_fisher, d_grad, d_chi2, d_work, work_doubles
SIGNATURES['cp_taylor_gauss_newton'] = (ctypes.c_int, _TAYLOR_HEAD + _RANGE + _GN_TAIL + _WHERE)
SIGNATURES['cp_taylor_gauss_newton_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong])
SIGNATURES['cp_mlp_gauss_newton'] = (ctypes.c_int, _MLP_HEAD + _RANGE + _GN_TAIL + _WHERE)
SIGNATURES['cp_mlp_gauss_newton_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int, ctypes.c_longlong])
SIGNATURES['cp_lm_layout'] = (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)])
# B, ndim; the state x, fisher, grad, chi2, lambda, status, naccepted; the trial xt, fisher_t, grad_t, chi2_t; lo, hi; up, down, lmin, lmax, ftol; next
SIGNATURES['cp_lm_step'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 13 + [ctypes.c_double] * 5 + [ctypes.c_void_p] + _WHERE)
SIGNATURES['cp_lm_step_velocity'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 13 + [ctypes.c_double] * 5 + [ctypes.c_void_p] * 2 + _WHERE)
# B, ndim; the state x, fisher, grad, lambda, status; lo, hi; velocity, h; alpha; next, naccelerated
SIGNATURES['cp_lm_accelerate'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 9 + [ctypes.c_double] + [ctypes.c_void_p] * 2 + _WHERE)
SIGNATURES['cp_spd_inverse'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 3 + _WHERE)
SIGNATURES['cp_hmc_factor'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 3 + _WHERE)      # B, ndim; metric, factor, status
# B, ndim, t_close, t_open; the state x, grad, chi2, status, naccepted, nout; the trajectory z, h0, eps, out; the trial xt, grad_t, chi2_t; factor, lo, hi, step;
# jitter, seed; next, sample, sample_chi2
SIGNATURES['cp_hmc_step'] = (ctypes.c_int, [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong] + [ctypes.c_void_p] * 17 +
                             [ctypes.c_double, ctypes.c_ulonglong] + [ctypes.c_void_p] * 3 + _WHERE)
SIGNATURES['cp_gauss_newton_dense_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong])
# d_jac, ldj; B, ndim, ncols; d_value, ldv; d_data, ldd; d_precision, ldp; d_fisher, d_grad, d_chi2, d_work, work_doubles
SIGNATURES['cp_gauss_newton_dense'] = (ctypes.c_int, _ARRAY + [ctypes.c_longlong, ctypes.c_int, ctypes.c_longlong] + _ARRAY + _ARRAY + _ARRAY + [ctypes.c_void_p] * 4 +
                                       [ctypes.c_longlong] + _WHERE)
SIGNATURES['cp_mlp_predict'] =(ctypes.c_int, _MLP_HEAD + [ctypes.c_void_p] + _WHERE)
SIGNATURES['cp_mlp_predict_columns'] = (ctypes.c_int, _MLP_HEAD + _RANGE + _ARRAY + _WHERE)
SIGNATURES['cp_mlp_jacobian'] = (ctypes.c_int, _MLP_HEAD + _RANGE + _ARRAY + _ARRAY + _WHERE)      # d_value, ldv; d_jac, ldj
SIGNATURES['cp_mlp_vjp'] = (ctypes.c_int, _MLP_HEAD + _RANGE + _ARRAY + _ARRAY + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong] + _WHERE)      # d_cot, ldc; d_value, ldv; d_grad, d_work, work_doubles
SIGNATURES['cp_mlp_vjp2'] = SIGNATURES['cp_mlp_vjp']      # d_hess in the place of d_grad
SIGNATURES['cp_mlp_jvp'] = (ctypes.c_int, _MLP_HEAD + _RANGE + _ARRAY + _ARRAY + _ARRAY + _WHERE)      # d_tan, K; d_value, ldv; d_out, ldo
# d_tan_u; d_tan_v, K; d_value, ldv; d_first_u; d_first_v, ldf; d_out, ldo
SIGNATURES['cp_mlp_jvp2'] = (ctypes.c_int, _MLP_HEAD + _RANGE + [ctypes.c_void_p] + _ARRAY + _ARRAY + [ctypes.c_void_p] + _ARRAY + _ARRAY + _WHERE)
SIGNATURES['cp_taylor_fit'] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
SIGNATURES['cp_mlp_param_count'] = (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int])
SIGNATURES['cp_mlp_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int])
SIGNATURES['cp_taylor_vjp_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int])
SIGNATURES['cp_taylor_vjp2_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int])
SIGNATURES['cp_mlp_vjp2_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_int])
SIGNATURES['cp_mlp_vjp_workspace_doubles'] = (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int, ctypes.c_longlong])
SIGNATURES['cp_mlp_loss_grad'] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int, ctypes.c_int, _c_int_p, _c_int_p, ctypes.c_int,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p])
SIGNATURES['cp_mlp_adam'] = (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_longlong] + [ctypes.c_double] * 6 + [ctypes.c_int, ctypes.c_void_p])
MLP_ACTIVATIONS = {'silu': 0, 'relu': 1, 'tanh': 2, 'identity-silu': 3}
MLP_YFUNCTIONS = {None: 0, 'log10': 1, 'arcsinh': 2}      # enum cp_mlp_yfunction: the inverse applied, 10^v / sinh(v)
NCDM_NKNOTS = 119
GROWTH_NKNOTS = 201

BG_PARAMS = ('h', 'Omega_cdm', 'Omega_b', 'Omega_k', 'T_cmb', 'N_ur', 'w0_fld', 'wa_fld')
SPLINE_BC = {'natural': 0, 'clamped': 1, 'not-a-knot': 2}
PK_PARAMS = ('A_s', 'n_s', 'alpha_s', 'beta_s', 'k_pivot')
ENGINES = {'eisenstein_hu': 0, 'eisenstein_hu_nowiggle': 1, 'bbks': 2}
PK_WHAT = {'matter': 0, 'transfer': 1, 'primordial': 2, 'log_k_matter': 3}
DERIVED_VALUES = ('_h2', 'H0', 'Omega_g', 'T_ur', 'Omega_ur', 'Omega_r', 'Omega_m', 'Omega_de', 'K', 'omega_b', 'omega_cdm', 'omega_m', 'omega_g', 'omega_ur',
                  'omega_r', 'omega_k', 'omega_de')      # enum cp_derived_value
VARIANTS_SCALARS = ('omega_b', 'omega_m', 'frac_b', 'frac_cdm', 'frac_cb', 'frac_ncdm', 'theta_cmb', 'z_eq', 'k_eq', 'z_drag', 'rs_drag', 'p_c', 'p_cb',
                    'gamma_ncdm', 'beta_c')      # enum cp_variants_scalar
MATH_FUNCTIONS = {'exp_mid': 0, 'exp_tab': 1, 'log_pos': 2, 'log_tab': 3, 'exp10_mid': 4, 'exp10_tab': 5, 'sin_bounded': 6, 'recip': 7, 'rsqrt_pos': 8}      # enum cp_math_function
EH_SCALARS = ('rs_drag', 'z_drag', 'z_eq', 'k_eq', 'r_drag', 'r_eq', 'k_silk', 'alpha_c', 'beta_c', 'alpha_b', 'beta_node', 'beta_b', 'alpha_gamma',
              'gamma')
BG_KINDS = {'comoving_radial_distance': 0, 'comoving_transverse_distance': 1, 'angular_diameter_distance': 2, 'luminosity_distance': 3,
            'efunc': 4, 'hubble_function': 5, 'growth_cpt': 6, 'growth_rate': 7, 'rho_crit': 8, 'Omega_m': 9, 'Omega_de': 10,
            'rho_g': 11, 'rho_b': 12, 'rho_ur': 13, 'rho_cdm': 14, 'rho_k': 15, 'rho_Lambda': 16, 'rho_fld': 17, 'rho_de': 18, 'rho_tot': 19,
            'rho_m': 20, 'rho_r': 21, 'T_cmb': 22, 'time': 23, 'age': 24, 'rho_ncdm': 25, 'p_ncdm': 26, 'rs': 27, 'rs_cosmomc': 28}
BG_AS_FRACTION = 32
for _name in ('g', 'b', 'ur', 'cdm', 'k', 'Lambda', 'fld', 'r', 'ncdm'):     # Omega_x(z) = rho_x(z) / rho_crit(z)
    BG_KINDS['Omega_' + _name] = BG_KINDS['rho_' + _name] | BG_AS_FRACTION
BG_KINDS['pfrac_ncdm'] = BG_KINDS['p_ncdm'] | BG_AS_FRACTION     # p_ncdm(z) / rho_crit(z)

_lib = None


class LibraryError(RuntimeError):
    """The HIP library is missing or unusable."""


def load():
    """Load (once) and return the shared library; raise :class:`LibraryError` if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = LIB_PATH
    variant = os.environ.get('COSMOPRIMO_AMD_LIBRARY')      # measurements only (tools/variant_lib.sh: a variant of ONE source linked beside the shipped library,
    if variant:                                             # which is never rebuilt in place): an explicit path, which must exist
        if not os.path.isfile(variant):
            raise LibraryError('COSMOPRIMO_AMD_LIBRARY = {} does not exist'.format(variant))
        path = variant
    if not os.path.isfile(path):
        raise LibraryError('{} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` or '
                           '`make -C cosmoprimo_amd/csrc -j8` (hipcc, gfx950). There is no CPU fallback.'.format(LIB_PATH))
    try:
        # torch ships its own libamdhip64.so.7; import it first so the HIP runtime is shared with torch's allocator/streams
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise LibraryError('{} does not export {} (stale build?)'.format(path, name))
        fn.restype = restype
        fn.argtypes = argtypes
    if lib.cp_abi_version() != ABI_VERSION:
        raise LibraryError('ABI version mismatch: library {}, bindings {}'.format(lib.cp_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


_background_ready = set()


def background_init(device_index):
    """The knot tables of the background kernels on device ``device_index`` (``cp_background_init``: one allocation and synchronous uploads, once per
    device), so that the entry points that read them stay asynchronous and allocation-free from their first call on."""
    if device_index not in _background_ready:
        check(load().cp_background_init(int(device_index)))
        _background_ready.add(device_index)


def check(status):
    """Map a status code onto the exception class the reference raises for the same condition."""
    if status == CP_OK:
        return
    msg = load().cp_last_error().decode('utf-8', 'replace')
    if status == CP_EINVAL:
        raise ValueError(msg)
    if status == CP_EUNSUPPORTED:
        raise NotImplementedError(msg)
    if status == CP_ENOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def as_double_p(array):
    return array.ctypes.data_as(_c_double_p)


def _complex_map(fn_name, z, *head):
    z = np.ascontiguousarray(z, dtype='c16')
    out = np.empty_like(z)
    fn = getattr(load(), fn_name)
    check(fn(*head, as_double_p(z.view('f8')), as_double_p(out.view('f8')), z.size))
    return out


def loggamma(z):
    """Principal branch of log Gamma on complex ``z`` (host; replaces scipy.special.loggamma in table setup)."""
    return _complex_map('cp_loggamma', z)


def gamma(z):
    return _complex_map('cp_gamma', z)


def kernel_eval(kind, param, z):
    """Mellin kernel U_K(z) (reference cosmoprimo/fftlog.py:666-766) on complex ``z``."""
    return _complex_map('cp_kernel_eval', z, int(kind), float(param))
