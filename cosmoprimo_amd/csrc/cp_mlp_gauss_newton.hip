// cp_mlp_gauss_newton.hip -- Fisher matrices and Gauss-Newton normal equations of the MLP emulator (cp_mlp.hip) for batches of parameter points (gfx950)
// + C ABI: per point b over a range of output columns, fisher = J W J^T, grad = J W (data - value), chi2 = (data - value)^T W (data - value), J the
// Jacobian of cp_mlp_jacobian, W diagonal.  No (B, ndim, .) array exists anywhere: the tile of J that mlp_tangent_kernel stores is contracted over its
// columns in registers and LDS instead (cp_gauss_newton.h: the epilogue, the partial sums, the summing kernel).
// Launches.  mlp_forward_kernel through cp::mlp_predict_launch (the value on the range, to d_value or to the workspace: what cp_mlp_predict_columns
// writes, bit for bit; skipped when nothing reads it: no data, no d_value, no y function), mlp_gn_kernel, gn_sum_kernel.
// mlp_gn_kernel.  mlp_tangent_kernel up to its epilogue, operation for operation -- the hidden layers' primal and tangent in LDS updated in place, the last
// tangent times the output kernel on the matrix cores with the operand fetch, masking and prefetch of the forward kernel -- with the rows of
// cp_gauss_newton.h: a row tile holds P = floor(64 / ndim) whole points, row t = p ndim + i.  The device functions it shares with mlp_tangent_kernel are
// restated here, so that every kernel of cp_mlp.hip keeps its instructions; a J formed here has the bits of cp_mlp_jacobian.
// LDS: the larger of the hidden layers' nr x (80 + 64) doubles (at most 72 KB) and the epilogue's (cp_gauss_newton.h), which reuses it.
#include "cp_gauss_newton.h"
#include "cp_math.h"

namespace {

using cpgn::v4d;

constexpr int MG_RS = 80, MG_PS = 64;      // row strides of the tangent and the primal buffer (mlp_tangent_kernel)
enum { ACT_SILU = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_IDENTITY_SILU = 3 };

struct MlpGnArgs {
    const double* x;          // (B, ndim) raw parameters
    const double* params;
    const double* xoff;
    const double* xscale;
    const double* yscale;
    cp::MlpLayout net;
    cpgn::Tail tail;
};

// activate_tangent of cp_mlp.hip
__device__ __forceinline__ void gn_activate_tangent(int act, double v, double alpha, double beta, double& h, double& d) {
    switch (act) {
        case ACT_SILU: {
            const double e = 1. + cpmath::exp_mid(-v), s = 1. / e;
            h = v / e;
            d = s * (1. + v * (1. - s));
            break;
        }
        case ACT_RELU:
            h = v > 0. ? v : (v != v ? v : 0.);
            d = v > 0. ? 1. : (v != v ? v : 0.);
            break;
        case ACT_TANH: {
            const double t = tanh(v);
            h = t;
            d = 1. - t * t;
            break;
        }
        default: {
            const double e = 1. + cpmath::exp_mid(-alpha * v), s = 1. / e;
            h = ((1. - beta) + beta / e) * v;
            d = (1. - beta) + beta * (s + alpha * v * (s * (1. - s)));
        }
    }
}

// mlp_load and mlp_mask of cp_mlp.hip: the operands of two MFMA steps; a row of the right operand past K is never read (row 0 in its place, masked)
__device__ __forceinline__ void gn_load(const double* B, const int K, const int M, const double* buf, const int p, const int l15, const int g, const int (&colj)[4],
                                        double (&a)[2][4], double (&b)[2][4], bool (&keep)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = 8 * p + 4 * h + g;
        const bool inside = k < K;
        const double* br = B + (long long)(inside ? k : 0) * M;
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = br[colj[j]];
        keep[h] = inside;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[h][i] = buf[k * MG_RS + 16 * i + l15];
    }
}

__device__ __forceinline__ void gn_mask(double (&b)[2][4], const bool (&keep)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = keep[h] ? b[h][j] : 0.;
}

template <int YF>
__global__ __launch_bounds__(256, 2) void mlp_gn_kernel(const MlpGnArgs A) {
    extern __shared__ double mg_lds[];
    const cp::MlpLayout& N = A.net;
    const cpgn::Tail& G = A.tail;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const long long b0 = (long long)blockIdx.x * G.P;      // the tile's first point: row t is point b0 + t / ndim, parameter t % ndim
    const int c0 = G.c0, cend = G.cend;
    const int col0 = c0 + (int)blockIdx.y * cpgn::GN_COLS + wave * 64;
    double* const curt = mg_lds;                      // tangents, nr x MG_RS
    double* const curp = mg_lds + N.nr * MG_RS;       // primal activations, nr x MG_PS
    {      // the inputs of the tile's rows and their tangents, k-major; idle rows and points past the end: finite, never stored
        const int p = lane / N.ndim, mine = lane - p * N.ndim;
        const bool inside = p < G.P && b0 + p < G.B;
        for (int i = wave; i < N.ndim; i += 4) {
            double v = 0., t = 0.;
            if (inside) {
                const double xs = A.xscale[i];
                v = (A.x[(b0 + p) * N.ndim + i] - A.xoff[i]) / xs;
                t = i == mine ? 1. / xs : 0.;
            }
            curp[i * MG_PS + lane] = v;
            curt[i * MG_RS + lane] = t;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < N.L; ++l) {
        const int nin = N.d[l], nout = N.d[l + 1], act = N.act[l];
        const double* W = A.params + N.off[l];
        const double* bias = W + nin * nout;
        const double alpha = bias[nout], beta = bias[nout + 1];
        // the layer in place: a wave's neurons j = wave + 4 q (at most 16: four groups of four) stay in registers until every wave has read the inputs
        double hn[4][4], tn[4][4];
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            const int j0 = wave + 16 * grp;
#pragma unroll
            for (int q = 0; q < 4; ++q) hn[grp][q] = tn[grp][q] = 0.;
            if (j0 >= nout) continue;      // (wave-uniform)
            int jq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) jq[q] = j0 + 4 * q < nout ? j0 + 4 * q : j0;
            double accz[4] = {0., 0., 0., 0.}, acct[4] = {0., 0., 0., 0.};
#pragma unroll 2
            for (int k = 0; k < nin; ++k) {
                const double hv = curp[k * MG_PS + lane], tv = curt[k * MG_RS + lane];
                const double* wr = W + k * nout;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double w = wr[jq[q]];
                    accz[q] = fma(hv, w, accz[q]);
                    acct[q] = fma(tv, w, acct[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double dval;
                gn_activate_tangent(act, accz[q] + bias[jq[q]], alpha, beta, hn[grp][q], dval);
                tn[grp][q] = dval * acct[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int grp = 0; grp < 4; ++grp)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = wave + 16 * grp + 4 * q;
                if (j < nout) {
                    curp[j * MG_PS + lane] = hn[grp][q];
                    curt[j * MG_RS + lane] = tn[grp][q];
                }
            }
        for (int j = nout + wave; j < ((nout + 7) & ~7); j += 4) curt[j * MG_RS + lane] = 0.;      // the left operand's rows up to the next pair of MFMA steps
        __syncthreads();
    }
    // the output layer on the matrix cores: acc = dh_L . W_out[:, columns]
    const int K = N.d[N.L], M = N.M;
    const double* Wo = A.params + N.off[N.L];
    v4d acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4d{0., 0., 0., 0.};
    int colj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        colj[j] = col < cend ? col : cend - 1;      // columns past the end of the range repeat its last one (their weight is 0 in the epilogue)
    }
    {
        const int npairs = (K + 7) / 8;
        double a0[2][4], b0r[2][4];
        bool keep[2];
        gn_load(Wo, K, M, curt, 0, l15, g, colj, a0, b0r, keep);
        gn_mask(b0r, keep);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            gn_load(Wo, K, M, curt, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1, keep);
            __builtin_amdgcn_sched_barrier(0);      // the loads are issued here, not moved below the MFMAs
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h][i], b0r[h][j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i) a0[h][i] = a1[h][i], b0r[h][i] = b1[h][i];
            __builtin_amdgcn_sched_barrier(0);
            gn_mask(b0r, keep);
        }
    }
    __syncthreads();      // every wave has read the last tangent: the epilogue takes the LDS over
    cpgn::gn_contract<YF>(G, A.yscale, acc, mg_lds + wave * (cpgn::epilogue_lds_doubles(G.P, N.ndim) / 4), lane, b0, col0);
    cpgn::gn_combine(G, mg_lds, b0, (int)blockIdx.y);
}

template <int YF>
int mlp_gn_launch(const char* who, const MlpGnArgs& A, const cpgn::Plan& plan, void* stream) {
    const size_t hidden = (size_t)A.net.nr * (MG_RS + MG_PS), epilogue = cpgn::epilogue_lds_doubles(plan.P, A.net.ndim);
    const size_t lds = (hidden > epilogue ? hidden : epilogue) * sizeof(double);
    if (lds > 64 * 1024) {
        const hipError_t e = cp::allow_full_lds<mlp_gn_kernel<YF>>();
        if (e != hipSuccess) return cp::launch_status(who, e);
    }
    hipLaunchKernelGGL((mlp_gn_kernel<YF>), dim3((unsigned)plan.nrt, (unsigned)plan.nct), dim3(256), lds, static_cast<hipStream_t>(stream), A);
    return CP_OK;
}

}  // namespace

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
    MlpGnArgs A{};
    int status = cp::mlp_front_layout(who, B, ndim, nlayers, widths, activations, M, yfunction, col0, ncols, &A.net);
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
    if (d_value || d_data || yfunction != CP_MLP_Y_NONE) {
        status = cp::mlp_predict_launch(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols,
                                        value, ldvalue, stream);
        if (status != CP_OK) return status;
    }
    A.x = d_x, A.params = d_params, A.xoff = d_xoffset, A.xscale = d_xscale, A.yscale = d_yscale;
    A.tail = cpgn::Tail{d_weights, d_data, value, d_work + plan.part, ldw, ldd, ldvalue, B, ndim, plan.P, (int)col0, (int)(col0 + ncols)};
    if (yfunction == CP_MLP_Y_NONE) status = mlp_gn_launch<cpgn::GN_Y_NONE>(who, A, plan, stream);
    else if (yfunction == CP_MLP_Y_EXP10) status = mlp_gn_launch<cpgn::GN_Y_EXP10>(who, A, plan, stream);
    else status = mlp_gn_launch<cpgn::GN_Y_SINH>(who, A, plan, stream);
    if (status != CP_OK) return status;
    cpgn::sum_launch(plan, A.tail, d_fisher, d_grad, d_chi2, stream);
    return cp::launch_status(who);
}
