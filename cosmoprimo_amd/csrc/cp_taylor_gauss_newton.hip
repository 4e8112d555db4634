// cp_taylor_gauss_newton.hip -- Fisher matrices and Gauss-Newton normal equations of the Taylor emulator (cp_taylor.hip) for batches of parameter points
// (gfx950) + C ABI: per point b over a range of output columns, fisher = J W J^T, grad = J W (data - value), chi2 = (data - value)^T W (data - value), J the
// Jacobian of cp_taylor_jacobian, W diagonal.  No (B, ndim, .) array exists anywhere: the tile of J that the jacobian front end of taylor_gemm_kernel would
// store is contracted over its columns in registers and LDS instead (cp_gauss_newton.h: the epilogue, the partial sums, the summing kernel).
// Launches.  taylor_gemm_kernel<predict> through cp::taylor_predict_launch where data or d_value is given (the value on the range, to d_value or to the
// workspace: what cp_taylor_predict_columns writes), taylor_gemm_kernel with its Gauss-Newton front end, gn_sum_kernel.
// This file holds the entry points only.  The kernel is the one __global__ template of cp_taylor_gemm.h, instantiated here for TaylorGnArgs: the entries of
// the jacobian front end with the rows of cp_gauss_newton.h -- a row tile holds P = floor(64 / ndim) whole points, row t = p ndim + i -- and its epilogue;
// a J formed here has the bits of cp_taylor_jacobian.  Every kernel is still held to its instructions: the template's variants differ under `if constexpr`
// only, and share no device function for the body.
// LDS: the larger of 2 x 32 x 80 + ndim x 64 doubles (at most 56 KB) and the epilogue's (cp_gauss_newton.h), which reuses it.
#include "cp_taylor_gemm.h"

extern "C" long long cp_taylor_gauss_newton_workspace_doubles(long long B, int ndim, int T, int M, long long ncols) {
    const char* who = "cp_taylor_gauss_newton_workspace_doubles";
    const int status = cp::taylor_front_checks(who, B, ndim, T, 0, M, 0, ncols, ncols, "value");
    if (status != CP_OK) return -(long long)status;
    cpgn::Plan plan;
    const int planned = cpgn::plan(who, B, ndim, ncols, &plan);
    return planned == CP_OK ? plan.total : -(long long)planned;
}

extern "C" int cp_taylor_gauss_newton(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                                      const double* d_derivatives, int M, long long col0, long long ncols, const double* d_weights, long long ldw,
                                      const double* d_data, long long ldd, double* d_value, long long ldv, double* d_fisher, double* d_grad, double* d_chi2,
                                      double* d_work, long long work_doubles, int device, void* stream) {
    const char* who = "cp_taylor_gauss_newton";
    int status = cp::taylor_front_checks(who, B, ndim, T, max_power, M, col0, ncols, d_value ? ldv : ncols, "value");
    if (status != CP_OK) return status;
    status = cpgn::check_operands(who, ncols, ldw, d_data, ldd, d_value, ldv);
    if (status != CP_OK) return status;
    cpgn::Plan plan;
    status = cpgn::plan(who, B, ndim, ncols, &plan);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    status = cpgn::check_pointers(who, d_weights, d_data, d_fisher, d_grad, d_chi2, d_work, work_doubles, plan, "cp_taylor_gauss_newton_workspace_doubles");
    if (status != CP_OK) return status;
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    // the value on the range: to the caller's buffer, else to the workspace, if anything reads it
    double* value = d_value ? d_value : d_work + plan.value;
    const long long ldvalue = d_value ? ldv : ncols;
    cp::Launches on(who, stream);
    if (d_value || d_data) {
        status = cp::taylor_predict_launch(on, d_x, B, d_center, d_powers, ndim, T, d_derivatives, M, col0, ncols, value, ldvalue);
        if (status != CP_OK) return status;
    }
    TaylorGnArgs A{d_x, d_center, d_powers, d_derivatives, T, M,
                   cpgn::Tail{d_weights, d_data, value, d_work + plan.part, ldw, ldd, ldvalue, B, ndim, plan.P, (int)col0, (int)(col0 + ncols)}};
    taylor_gemm_launch<TY_GAUSS_NEWTON>(on, A, dim3((unsigned)plan.nrt, (unsigned)plan.nct), ndim, cpgn::epilogue_lds_doubles(plan.P, ndim));
    cpgn::sum_launch(on, plan, A.tail, d_fisher, d_grad, d_chi2);
    return on.status();
}
