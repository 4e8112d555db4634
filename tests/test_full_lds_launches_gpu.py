"""GPU: launches that ask for more than 64 KB of dynamic LDS.  Above 65 536 bytes a kernel symbol must have been allowed the LDS on the device it is
launched on; ``cp::Launches::run`` (csrc/cp_internal.h) does that for exactly the instantiation it launches.  A lost opt-in shows only where a launch
really crosses 64 KB, so every kernel family that can cross is launched there once: by an existing test where its shapes cross already, by a case
of this file otherwise.  A launch that fails raises from ``_lib.check`` or leaves the output unwritten; either fails the comparison.

Family (file): dynamic LDS in bytes; smallest shape above 65 536; the test that launches it there.

- fftlog_kernel (cp_fftlog_kernel.h): Fftlog<NP, P>::LDS_BYTES = 34 960 at NP = 2048, 69 920 at 4096, 139 872 at 8192; padded size 4096;
  test_row_transform_bits_gpu.py and test_fftlog_gpu.py (padded sizes 4096 and 8192).
- sigma_rz_kernel (cp_sigma.hip): 34 960 + 16 (nq + nz); nq + nz >= 1912; ``test_sigma_rz_band_route`` below (nq = 2048, nz = 2: 67 760).
- fftlog_spline_kernel (cp_sigma.hip): 34 960 + 16 nq; nq >= 1912; ``test_fftlog_spline_execute`` below (nq = 2304: 71 824).
- fftlog_geospline_kernel (cp_sigma.hip): 34 960 + 16 (ne + 2) with ne <= 512 knots of the stretch: at most 43 184, cannot cross.
- sigma_functional_kernel, sigma8_normalise_kernel (cp_sigma.hip): no dynamic LDS.
- spline_apply_kernel<R> (cp_spline.hip): R x span_max x 8 with R halved down to 4 while above 64 KB; span_max > 2048 knots under a tile of
  queries; ``test_spline_apply_vector_route`` below (dense operator, n = 2304, R = 4: 73 728).
- spline_outer_kernel<R> (cp_spline.hip): R x (span_max + 256 + nz) x 8 with R halved down to 2; span_max + 256 + nz > 4096; ``test_spline_outer_epilogue``
  below (nz = 4096 factors per row, 2 rows: above 69 632).
- linop_mfma_kernel, linop_mid_mfma_kernel, tables_rows*_kernel, gap_spline_kernel, wallish_box_kernel, column_spline_kernel (cp_spline.hip): none.
- spline_points_lds_kernel (cp_interp.hip): (5 n - 4) x 8, n <= 2048; n >= 1640; test_fiducial_gpu.py::test_spline_points_of_a_catalogue (n = 2048
  knots, 202 049 queries: 81 888).  interp_linear_kernel, spline_points_kernel: 8 x at most 4096 coarse knots, cannot cross.
- spline_tables_lds_kernel (cp_spline_tables.hip): (5 n - 4) x 8, n <= 2048; n >= 1640; test_spline_tables_edges_gpu.py (n = 2048: 81 888).
- spline_tables_build_kernel (cp_spline_tables.hip): 32 n, n <= 4096; n >= 2049; test_spline_tables_edges_gpu.py (n = 2049: 65 568, n = 4096: 131 072).
- mlp_forward_kernel (cp_mlp.hip): 1280 nr, nr the widest layer rounded up to 8 (at most 64); widest layer >= 49 (nr = 56: 71 680);
  test_predict_columns_gpu.py (widths (64,): 81 920).
- mlp_tangent_kernel (cp_mlp_tangent.h): 1152 nr, or the Gauss-Newton epilogue's 32 (1216 + 48 floor(64 / ndim) + 64 ndim) where that is more; nr = 64
  (73 728), and every ndim of the Gauss-Newton variant (at least 67 584); test_mlp_jacobian_gpu.py (widths (5, 64)), test_mlp_gauss_newton_gpu.py.
- mlp_input_grad_kernel (cp_mlp.hip): 1024 nr <= 65 536 exactly, cannot cross.  The other kernels of cp_mlp.hip: none.
- taylor_gemm_kernel (cp_taylor_gemm.h): 40 960 + 512 f ndim, f = 0 (fit), 1 (predict, jacobian), 2 (jvp), ndim <= 32, or the Gauss-Newton epilogue as
  above; the jvp from ndim = 25 (ndim = 32: 73 728) and every Gauss-Newton call; test_taylor_jvp_gpu.py (ndim = 32), test_taylor_gauss_newton_gpu.py.
- taylor_input_grad_kernel (cp_taylor.hip): 512 (64 + ndim) + 2048 <= 51 200, cannot cross.
- dst_kernel<N> (cp_dst.hip): WorkgroupFft<N, 16>::lds_bytes() = 4 352, 17 472, 69 888 for N = 256, 1024, 4096; N = 4096; test_row_transform_bits_gpu.py,
  test_dst_rows_gpu.py.
- dst_generate_kernel, wallish_tail_kernel, wallish_full_kernel (cp_dst.hip, cp_wallish_tail.h): 69 888 + 640 always; test_row_transform_bits_gpu.py,
  test_bao_gpu.py (wallish2018 of batches).
- rfft_kernel<M> (cp_rfft.hip): WorkgroupFft<M, P>::lds_bytes(), 34 944 at M = 2048, 69 888 at 4096, 139 808 at 8192; real size 8192;
  test_row_transform_bits_gpu.py, test_rfft_rows_gpu.py (sizes 8192 and 16 384).
- wallish_dd_box_kernel (cp_bao.hip): 32 (n + 64) + 640; n = 2048 (68 224; n = 1024: 35 456); test_bao_gpu.py, test_fused_kernels_gpu.py (2048 coefficients).
- brieden_resample_kernel (cp_bao.hip): 88 n + 512 with four waves (n <= 512: cannot cross), or 216 n + 1536 + 8 np n with twelve waves and the
  np columns of the peaks' operator in LDS; n >= 297 samples whatever np; test_brieden_edges_gpu.py (cp_brieden_smooth at n = 129 .. 512).
- splice_kernel, splice_uniform_kernel (cp_bao.hip, cp_splice_uniform.h), spline_rows_kernel (cp_spline_rows.hip): the plan's lds_bytes; the uniform
  scheme from 32 (64 S + 130) = 71 744 at S = 33 always, the others with the plan's knots; test_splice_edges_gpu.py, test_spline_rows_edges_gpu.py,
  test_bao_gpu.py.
- every kernel of cp_background.hip, cp_power.hip, cp_fftlog_large.hip, cp_xi_filter.hip, cp_lm.hip, cp_gauss_newton.hip, cp_math_eval.hip,
  cp_pairs.hip, cp_rows.hip: no dynamic LDS.
"""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_sigma_rz_band_route(monkeypatch):
    """cp_sigma_rz_analytic's one-kernel route with the banded spline operator at 2048 radii x 2 redshifts (67 760 bytes of LDS) against the same radii as
    two calls of 1024 (51 376 bytes each).  A radius' weights do not depend on the other radii of its operator: the tolerance is that of
    test_sigma_fused_gpu.py for two evaluations with the same arithmetic."""
    import cosmoprimo_amd as cp
    from cosmoprimo_amd import interpolator as itp
    warnings.simplefilter('ignore')
    monkeypatch.setattr(itp, '_SIGMA_RZ_PREFILTERED', False)
    rng = np.random.default_rng(3)
    par = dict(Omega_m=rng.uniform(.25, .40, 3), Omega_b=rng.uniform(.04, .06, 3), h=rng.uniform(.6, .8, 3), n_s=rng.uniform(.92, 1., 3))
    interp = cp.Cosmology(engine='eisenstein_hu', sigma8=0.8, **par).get_fourier().pk_interpolator()
    monkeypatch.setattr(type(interp), '_two_stream_min_bytes', 0)
    r, z = np.geomspace(0.5, 150., 2048), np.array([0., 1.5])
    whole = np.asarray(interp.sigma_rz(r, z))
    halves = np.concatenate([np.asarray(interp.sigma_rz(r[:1024], z)), np.asarray(interp.sigma_rz(r[1024:], z))], axis=1)
    assert whole.shape == (3, 2048, 2) and np.isfinite(whole).all()
    np.testing.assert_allclose(whole, halves, rtol=1e-13, atol=0)


def test_fftlog_spline_execute():
    """cp_fftlog_spline_execute at 2304 queries (71 824 bytes of LDS), 3 rows, against the transform and the spline as two kernels, as
    test_fused_kernels_gpu.py::test_fftlog_spline_execute compares them."""
    import torch
    import cosmoprimo_amd as cp
    from cosmoprimo_amd import _lib, _device as dv
    from cosmoprimo_amd.spline import LinearOperator
    dev = torch.device('cuda:0')
    lib = _lib.load()
    nrows, nq = 3, 2304
    k = np.geomspace(1e-7, 1e2, 1024)
    fft = cp.TophatVariance(k, device=dev)
    r = np.geomspace(0.7, 150., nq)
    r[0], r[-1] = 1e-5, 1e9                                                       # outside the output grid of the transform: NaN
    op = LinearOperator.spline(fft.y[0], r, bc='natural', device=dev)
    plan = fft._get_plan(dev)
    assert lib.cp_sigma_rz_fused_available(plan.handle, op._handle) == 1
    rng = np.random.default_rng(nrows)
    rows = torch.as_tensor(rng.uniform(0.5, 2., (nrows, 1)) * (k / 0.05)**rng.uniform(-2.2, -1.8, (nrows, 1)) * 1e4, device=dev).contiguous()
    for post in (0, 1):
        out = torch.full((nrows, nq), -3., dtype=torch.float64, device=dev)
        _lib.check(lib.cp_fftlog_spline_execute(plan.handle, op._handle, rows.data_ptr(), out.data_ptr(), nrows, post, dv.stream_of(dev)))
        ref = op(fft(rows)[1], sqrt=bool(post)).cpu().numpy()
        got = out.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isfinite(got[:, 1:-1]).all()
        np.testing.assert_allclose(got[np.isfinite(ref)], ref[np.isfinite(ref)], rtol=2e-11)


def test_spline_apply_vector_route():
    """cp_spline_apply on the vector route for an operator whose queries couple to 2304 knots (4 rows x 2304 knots staged: 73 728 bytes of LDS), 3 rows,
    against the matrix-core route (no dynamic LDS) and numpy, at the tolerance of test_linop_gpu.py::test_dense_operator_paths."""
    import torch
    from cosmoprimo_amd.spline import LinearOperator
    n, nq, nrows = 2304, 2, 3
    rng = np.random.default_rng(n + nq)
    w = rng.normal(size=(nq, n)) / np.sqrt(n)
    y = rng.normal(size=(nrows, n))
    op = LinearOperator.dense(w)
    ty = torch.as_tensor(y, device=op.device)
    ref = y.dot(w.T)
    scale = np.abs(y).max() * np.abs(w).max() * n
    valu, mfma = op(ty, path='valu').cpu().numpy(), op(ty, path='mfma').cpu().numpy()
    assert valu.shape == ref.shape and np.isfinite(valu).all()
    assert np.abs(valu - ref).max() < 1e-14 * scale and np.abs(valu - mfma).max() < 1e-14 * scale


def test_spline_outer_epilogue():
    """cp_spline_apply_outer with 4096 factors per row (2 rows x (knots under a tile + 256 + 4096) doubles staged: more than 69 632 bytes of LDS) against its
    two-step form, as test_linop_gpu.py::test_outer_epilogue compares them."""
    import torch
    from cosmoprimo_amd.spline import LinearOperator
    rng = np.random.default_rng(3)
    x = np.geomspace(1e-2, 1e2, 1024)
    op = LinearOperator.spline(np.log(x), np.log(np.geomspace(0.1, 50., 8)), bc='natural')
    nrows, nz = 2, 4096
    y = torch.as_tensor(rng.uniform(0.5, 2., size=(nrows, 1024)) * x**-0.7, device=op.device)
    g = torch.as_tensor(rng.uniform(0.1, 1., size=(nrows, nz)), device=op.device)
    two_steps = (op(y)[:, :, None] * g[:, None, :]).sqrt()
    fused = op.outer(y, g, sqrt=True)
    assert fused.shape == (nrows, 8, nz)
    assert torch.equal(fused, two_steps) or float(((fused - two_steps) / two_steps).abs().max()) < 1e-14
