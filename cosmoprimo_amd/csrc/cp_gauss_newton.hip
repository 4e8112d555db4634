// cp_gauss_newton.hip -- the part of cp_mlp_gauss_newton and cp_taylor_gauss_newton that does not depend on the engine (cp_gauss_newton.h): the tiles and
// the workspace, the entry points' own checks, and the kernel that adds the column tiles' partial sums in tile order and mirrors the triangle.
#include "cp_gauss_newton.h"

namespace cpgn {

namespace {

// out[b] = sum over the column tiles ct, in order, of part[ct][b]: a thread per entry q of a point's S = ndim^2 + ndim + 1.  fisher[b][i][j] is read at
// (max(i, j), min(i, j)) -- the triangle the main kernel's rows hold with the weighted factor first -- so that it is symmetric bit for bit.
__global__ __launch_bounds__(256) void gn_sum_kernel(const double* part, const long long B, const int ndim, const int nct, double* fisher, double* grad, double* chi2) {
    const int S = ndim * ndim + ndim + 1;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * S) return;
    const long long b = e / S;
    const int q = (int)(e - b * S);
    int from = q;
    if (q < ndim * ndim) {
        const int i = q / ndim, j = q - i * ndim;
        from = i >= j ? q : j * ndim + i;
    } else if (!grad) {
        return;
    }
    double s = 0.;
    for (int ct = 0; ct < nct; ++ct) s += part[((long long)ct * B + b) * S + from];
    if (q < ndim * ndim) fisher[b * ndim * ndim + q] = s;
    else if (q < ndim * ndim + ndim) grad[b * ndim + (q - ndim * ndim)] = s;
    else chi2[b] = s;
}

}  // namespace

int plan(const char* who, long long B, int ndim, long long ncols, Plan* plan) {
    const int P = GN_ROWS / ndim;
    const long long S = (long long)ndim * ndim + ndim + 1, nct = (ncols + GN_COLS - 1) / GN_COLS;
    // the grids: 2^31 - 1 row tiles of P points, column tiles along y, 2^31 - 1 workgroups of 256 entries in the summing kernel; with them the workspace
    // stays below 2^62 doubles
    if (B > 0x7fffffffLL * P || nct > 65535 || B > 0x7fffffffLL * 256 / S)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld points of %d parameters over %lld columns (at most 2^31 - 1 row tiles of %d points, 2^39 sums B (ndim^2 + ndim + 1), 2^24 - 256 columns)",
                        who, B, ndim, ncols, P);
    plan->P = P, plan->S = S, plan->nct = nct, plan->nrt = (B + P - 1) / P;
    plan->value = 0, plan->part = B * ncols, plan->total = plan->part + nct * B * S;
    return CP_OK;
}

int check_operands(const char* who, long long ncols, long long ldw, const double* d_data, long long ldd, const double* d_value, long long ldv) {
    if (ldw != 0 && ldw < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the weights is neither 0 (one shared row) nor at least their %lld columns", who, ldw, ncols);
    if (d_data && ldd != 0 && ldd < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the data is neither 0 (one shared row) nor at least their %lld columns", who, ldd, ncols);
    if (d_value && ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    return CP_OK;
}

int check_pointers(const char* who, const double* d_weights, const double* d_data, const double* d_fisher, const double* d_grad, const double* d_chi2,
                   const double* d_work, long long work_doubles, const Plan& plan, const char* sizer) {
    if (!d_weights || !d_fisher || !d_work) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    if (!d_data && (d_grad || d_chi2)) return cp::fail(CP_EINVAL, "%s: a gradient or chi2 is asked for without data", who);
    if (d_data && (!d_grad || !d_chi2)) return cp::fail(CP_EINVAL, "%s: null pointer (data is given: the gradient and chi2 are written)", who);
    if (work_doubles < plan.total) return cp::fail(CP_EINVAL, "%s: workspace of %lld doubles, %lld needed (%s)", who, work_doubles, plan.total, sizer);
    return CP_OK;
}

void sum_launch(cp::Launches& on, const Plan& plan, const Tail& tail, double* d_fisher, double* d_grad, double* d_chi2) {
    const long long entries = tail.B * plan.S;
    on.run<gn_sum_kernel>((unsigned)((entries + 255) / 256), 256, 0, tail.part, tail.B, tail.ndim, (int)plan.nct, d_fisher, d_grad, d_chi2);
}

}  // namespace cpgn
