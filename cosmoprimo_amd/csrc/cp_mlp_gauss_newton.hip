// cp_mlp_gauss_newton.hip -- Fisher matrices and Gauss-Newton normal equations of the MLP emulator (cp_mlp.hip) for batches of parameter points (gfx950)
// + C ABI: per point b over a range of output columns, fisher = J W J^T, grad = J W (data - value), chi2 = (data - value)^T W (data - value), J the
// Jacobian of cp_mlp_jacobian, W diagonal.  No (B, ndim, .) array exists anywhere: the tile of J that mlp_tangent_kernel would store is contracted over its
// columns in registers and LDS instead (cp_gauss_newton.h: the epilogue, the partial sums, the summing kernel).
// Launches.  mlp_forward_kernel through cp::mlp_predict_launch (the value on the range, to d_value or to the workspace: what cp_mlp_predict_columns
// writes, bit for bit; skipped when nothing reads it: no data, no d_value, no y function), mlp_tangent_kernel in its Gauss-Newton variant, gn_sum_kernel.
// This file holds the entry points and cpgn::mlp_launch (the last two launches, which cp_mlp_vjp2 runs with weights of its own) only.  The kernel is the one __global__ template of cp_mlp_tangent.h, instantiated here for MlpGnArgs: a row tile holds
// P = floor(64 / ndim) whole points, row t = p ndim + i, and the epilogue is cp_gauss_newton.h's; a J formed here has the bits of cp_mlp_jacobian.  Every
// kernel is still held to its instructions: the template's variants differ under `if constexpr` only, and share no device function for the body.
// LDS: the larger of the hidden layers' nr x (80 + 64) doubles (at most 72 KB) and the epilogue's (cp_gauss_newton.h), which reuses it.
#include "cp_mlp_tangent.h"

void cpgn::mlp_launch(cp::Launches& on, const double* d_x, const double* d_params, const double* d_xoffset, const double* d_xscale, const double* d_yscale,
                      const cp::MlpLayout& net, int yfunction, const Plan& plan, const Tail& tail, double* d_fisher, double* d_grad, double* d_chi2) {
    MlpGnArgs A{};
    A.x = d_x, A.params = d_params, A.xoff = d_xoffset, A.xscale = d_xscale, A.yscale = d_yscale;
    A.net = net, A.tail = tail;
    const dim3 grid((unsigned)plan.nrt, (unsigned)plan.nct);
    const size_t epilogue = epilogue_lds_doubles(plan.P, tail.ndim);
    if (yfunction == CP_MLP_Y_NONE) mlp_tangent_launch<GN_Y_NONE>(on, A, grid, epilogue);
    else if (yfunction == CP_MLP_Y_EXP10) mlp_tangent_launch<GN_Y_EXP10>(on, A, grid, epilogue);
    else mlp_tangent_launch<GN_Y_SINH>(on, A, grid, epilogue);
    sum_launch(on, plan, tail, d_fisher, d_grad, d_chi2);
}

extern "C" long long cp_mlp_gauss_newton_workspace_doubles(long long B, int ndim, int nlayers, const int* widths, int M, long long ncols) {
    const char* who = "cp_mlp_gauss_newton_workspace_doubles";
    if (B < 0) return -(long long)cp::fail(CP_EINVAL, "%s: negative count of points", who);
    const long long total = cp_mlp_param_count(ndim, nlayers, widths, M);      // the network's checks
    if (total < 0) return total;
    if (ncols < 1 || ncols > M) return -(long long)cp::fail(CP_EINVAL, "%s: %lld columns of %d", who, ncols, M);
    cpgn::Plan plan;
    const int status = cpgn::plan(who, B, ndim, ncols, &plan);
    return status == CP_OK ? plan.total : -(long long)status;
}

extern "C" int cp_mlp_gauss_newton(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                                   const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                                   long long ncols, const double* d_weights, long long ldw, const double* d_data, long long ldd, double* d_value, long long ldv,
                                   double* d_fisher, double* d_grad, double* d_chi2, double* d_work, long long work_doubles, int device, void* stream) {
    const char* who = "cp_mlp_gauss_newton";
    cp::MlpLayout net{};
    int status = cp::mlp_front_layout(who, B, ndim, nlayers, widths, activations, M, yfunction, col0, ncols, &net);
    if (status != CP_OK) return status;
    status = cpgn::check_operands(who, ncols, ldw, d_data, ldd, d_value, ldv);
    if (status != CP_OK) return status;
    cpgn::Plan plan;
    status = cpgn::plan(who, B, ndim, ncols, &plan);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    status = cpgn::check_pointers(who, d_weights, d_data, d_fisher, d_grad, d_chi2, d_work, work_doubles, plan, "cp_mlp_gauss_newton_workspace_doubles");
    if (status != CP_OK) return status;
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    // the value on the range: to the caller's buffer, else to the workspace, if anything reads it
    double* value = d_value ? d_value : d_work + plan.value;
    const long long ldvalue = d_value ? ldv : ncols;
    cp::Launches on(who, stream);
    if (d_value || d_data || yfunction != CP_MLP_Y_NONE) {
        status = cp::mlp_predict_launch(on, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols,
                                        value, ldvalue);
        if (status != CP_OK) return status;
    }
    const cpgn::Tail tail{d_weights, d_data, value, d_work + plan.part, ldw, ldd, ldvalue, B, ndim, plan.P, (int)col0, (int)(col0 + ncols)};
    cpgn::mlp_launch(on, d_x, d_params, d_xoffset, d_xscale, d_yscale, net, yfunction, plan, tail, d_fisher, d_grad, d_chi2);
    return on.status();
}
