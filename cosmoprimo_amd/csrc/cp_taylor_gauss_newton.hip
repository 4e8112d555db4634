// cp_taylor_gauss_newton.hip -- Fisher matrices and Gauss-Newton normal equations of the Taylor emulator (cp_taylor.hip) for batches of parameter points
// (gfx950) + C ABI: per point b over a range of output columns, fisher = J W J^T, grad = J W (data - value), chi2 = (data - value)^T W (data - value), J the
// Jacobian of cp_taylor_jacobian, W diagonal.  No (B, ndim, .) array exists anywhere: the tile of J that the jacobian front end of taylor_gemm_kernel stores
// is contracted over its columns in registers and LDS instead (cp_gauss_newton.h: the epilogue, the partial sums, the summing kernel).
// Launches.  taylor_gemm_kernel<predict> through cp::taylor_predict_launch where data or d_value is given (the value on the range, to d_value or to the
// workspace: what cp_taylor_predict_columns writes), taylor_gn_kernel, gn_sum_kernel.
// taylor_gn_kernel.  The jacobian front end of taylor_gemm_kernel up to its store, operation for operation -- the derivatives of the monomials formed in LDS
// chunk by chunk of 32 terms (powers wave-uniform, factors of power 0 skipped, a term without the row's parameter exactly 0), two buffers in turn, the
// product with the derivatives on the matrix cores -- with the rows of cp_gauss_newton.h: a row tile holds P = floor(64 / ndim) whole points, row
// t = p ndim + i.  The two device functions it shares with taylor_gemm_kernel are restated here, so that every kernel of cp_taylor.hip keeps its
// instructions; a J formed here has the bits of cp_taylor_jacobian.
// LDS: the larger of 2 x 32 x 80 + ndim x 64 doubles (at most 56 KB) and the epilogue's (cp_gauss_newton.h), which reuses it.
#include "cp_gauss_newton.h"

namespace {

using cpgn::v4d;

constexpr int TG_KC = 32, TG_RS = 80, TG_MAX_POWER = 15;

struct TaylorGnArgs {
    const double* x;          // (B, ndim)
    const double* center;     // (ndim)
    const int* powers;        // (T, ndim)
    const double* b;          // (T, M) derivatives
    int K, M;                 // T terms, M columns of b
    cpgn::Tail tail;
};

// taylor_load and taylor_mask of cp_taylor.hip: the operands of two MFMA steps; a row of the right operand past K is never read (row 0 in its place, masked)
__device__ __forceinline__ void tg_load(const TaylorGnArgs& A, const double* buf, const int k0, const int p, const int l15, const int g, const int (&colj)[4],
                                        double (&a)[2][4], double (&b)[2][4], bool (&keep)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int kk = 8 * p + 4 * h + g, k = k0 + kk;
        const bool inside = k < A.K;
        const double* br = A.b + (long long)(inside ? k : 0) * A.M;
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = br[colj[j]];
        keep[h] = inside;
#pragma unroll
        for (int i = 0; i < 4; ++i) a[h][i] = buf[kk * TG_RS + 16 * i + l15];
    }
}

__device__ __forceinline__ void tg_mask(double (&b)[2][4], const bool (&keep)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = keep[h] ? b[h][j] : 0.;
}

__global__ __launch_bounds__(256, 2) void taylor_gn_kernel(const TaylorGnArgs A) {
    extern __shared__ double tg_lds[];
    const cpgn::Tail& G = A.tail;
    const int ndim = G.ndim;
    double* const abuf = tg_lds;                       // 2 x TG_KC x TG_RS
    double* const dl = tg_lds + 2 * TG_KC * TG_RS;     // (ndim, 64) x - center of the tile's rows
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int nchunk = (A.K + TG_KC - 1) / TG_KC;
    const long long b0 = (long long)blockIdx.x * G.P;      // the tile's first point: row t is point b0 + t / ndim, parameter t % ndim
    const int c0 = G.c0, cend = G.cend;
    const int col0 = c0 + (int)blockIdx.y * cpgn::GN_COLS + wave * 64;
    const int mine = lane % ndim;
    for (int e = threadIdx.x; e < ndim * cpgn::GN_ROWS; e += 256) {
        const int i = e >> 6, p = (e & 63) / ndim;
        dl[e] = p < G.P && b0 + p < G.B ? A.x[(b0 + p) * ndim + i] - A.center[i] : 0.;      // idle rows and points past the end: finite, never stored
    }
    __syncthreads();
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
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        double* const buf = abuf + (c & 1) * TG_KC * TG_RS;
        const int k0 = c * TG_KC;
        // d / dx_mine of the monomial: the factor of this lane's parameter is p d^(p - 1) -- exactly 0 for p = 0 whatever the other factors hold, and
        // without d for p = 1 --, the others d^p as in predict; the powers are wave-uniform, the lane's parameter a select
        for (int tt = wave; tt < TG_KC; tt += 4) {
            const int t = k0 + tt;
            double m = 0.;
            if (t < A.K) {
                m = 1.;
                bool zero = false;
                const int* pw = A.powers + (long long)t * ndim;
                for (int i = 0; i < ndim; ++i) {
                    int p = __builtin_amdgcn_readfirstlane(pw[i]);
                    if (p <= 0) {
                        zero = zero || mine == i;
                        continue;
                    }
                    p = p < TG_MAX_POWER ? p : TG_MAX_POWER;
                    const double d = dl[i * cpgn::GN_ROWS + lane];
                    if (p == 1) {
                        m *= mine == i ? 1. : d;
                        continue;
                    }
                    double v = d;      // d^(p - 1)
                    for (int q = 2; q < p; ++q) v *= d;
                    m *= mine == i ? (double)p * v : v * d;
                }
                m = zero ? 0. : m;
            }
            buf[tt * TG_RS + lane] = m;
        }
        __syncthreads();      // one barrier per chunk: the buffer written next was last read before this barrier
        const int npairs = A.K - k0 >= TG_KC ? TG_KC / 8 : (A.K - k0 + 7) / 8;
        double a0[2][4], b0r[2][4];
        bool keep[2];
        tg_load(A, buf, k0, 0, l15, g, colj, a0, b0r, keep);
        tg_mask(b0r, keep);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            tg_load(A, buf, k0, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1, keep);
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
            tg_mask(b0r, keep);
        }
    }
    __syncthreads();      // every wave has read the last chunk: the epilogue takes the LDS over
    cpgn::gn_contract<cpgn::GN_Y_PLAIN>(G, nullptr, acc, tg_lds + wave * (cpgn::epilogue_lds_doubles(G.P, ndim) / 4), lane, b0, col0);
    cpgn::gn_combine(G, tg_lds, b0, (int)blockIdx.y);
}

int taylor_gn_launch(const char* who, const TaylorGnArgs& A, const cpgn::Plan& plan, void* stream) {
    const size_t gemm = (size_t)2 * TG_KC * TG_RS + (size_t)A.tail.ndim * cpgn::GN_ROWS, epilogue = cpgn::epilogue_lds_doubles(plan.P, A.tail.ndim);
    const size_t lds = (gemm > epilogue ? gemm : epilogue) * sizeof(double);
    if (lds > 64 * 1024) {
        const hipError_t e = cp::allow_full_lds<taylor_gn_kernel>();
        if (e != hipSuccess) return cp::launch_status(who, e);
    }
    hipLaunchKernelGGL(taylor_gn_kernel, dim3((unsigned)plan.nrt, (unsigned)plan.nct), dim3(256), lds, static_cast<hipStream_t>(stream), A);
    return CP_OK;
}

}  // namespace

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
    if (d_value || d_data) {
        status = cp::taylor_predict_launch(who, d_x, B, d_center, d_powers, ndim, T, d_derivatives, M, col0, ncols, value, ldvalue, stream);
        if (status != CP_OK) return status;
    }
    TaylorGnArgs A{d_x, d_center, d_powers, d_derivatives, T, M,
                   cpgn::Tail{d_weights, d_data, value, d_work + plan.part, ldw, ldd, ldvalue, B, ndim, plan.P, (int)col0, (int)(col0 + ncols)}};
    status = taylor_gn_launch(who, A, plan, stream);
    if (status != CP_OK) return status;
    cpgn::sum_launch(plan, A.tail, d_fisher, d_grad, d_chi2, stream);
    return cp::launch_status(who);
}
