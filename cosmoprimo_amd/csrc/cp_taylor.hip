// cp_taylor.hip -- Taylor-expansion emulator of a calculator (reference emulators/tools/taylor.py:211-247) for batches of parameter points (gfx950)
// + C ABI.  One GEMM kernel in float64 on the matrix cores (v_mfma_f64_16x16x4_f64), taylor_gemm_kernel of cp_taylor_gemm.h -- its tile, LDS layout and
// monomials are described there --, with five of its front ends for the left operand launched from here:
//   predict : out (B, M) = monomials (B, T) . derivatives (T, M); the monomials of a tile of rows are formed in LDS, chunk of terms by chunk of terms,
//             from x - center and the integer powers -- the (B, T) matrix never exists in memory
//   fit     : derivatives (T, M) = S (T, npoints) . Y (npoints, M); S (the finite-difference weights of every term, built on the host) is staged
//             through the same LDS tiles
//   jacobian: jac (B ndim, M) = d monomials / d x_i (B ndim, T) . derivatives; a row is a (point, parameter) pair r = b ndim + i, its entry for term t the
//             derivative of the monomial, p_ti (x_i - c_i)^(p_ti - 1) prod_{j != i} (x_j - c_j)^p_tj, formed in LDS chunk by chunk as the monomials are
//   jvp     : out (B K, M) = [tan . d monomials / d x] (B K, T) . derivatives along K directions per point (cp_taylor_jvp, one launch); a row is a
//             (point, direction) pair r = b K + k.  No (B, ndim, .) array exists anywhere
//   jvp2    : out (B K, M) = [u . d^2 monomials / d x d x . v] (B K, T) . derivatives along K pairs of directions per point (cp_taylor_jvp2, one launch)
// (the fifth, Gauss-Newton, from cp_taylor_gauss_newton.hip).  Every kernel is held to its instructions; the front ends share their source by being
// variants of the one __global__ template, chosen at compile time, not by device functions for the body and not by copies.
// Vector-Jacobian product (cp_taylor_vjp: G (B, ndim) = cot . d predict / d x).  Two launches: S (B, T) = cot (B, ncols) . D[:, columns]^T is the GEMM with
// the front end of the fit -- both operands are then contiguous as that front end wants them, the left one (cot, row stride lda) along the contraction
// and the right one, rows [col0, col0 + ncols) of a TRANSPOSED copy (M, T) of the derivatives that the caller keeps, along the terms -- and
// taylor_input_grad_kernel contracts S with the derivatives of the monomials, which it forms as the jacobian front end does.  No (B, ndim, .) array exists.
// Contracted second derivative (cp_taylor_vjp2: hess (B, ndim, ndim) = sum_c cot d^2 predict / d x d x).  The S GEMM of cp_taylor_vjp, then
// taylor_curvature_kernel contracts S with the second derivatives of the monomials, a row per (point, pair i <= j), and writes both mirror entries.
#include "cp_taylor_gemm.h"

namespace {

// G[b][i] = sum_t S[b][t] d mono_t / d x_i for cp_taylor_vjp: a row per (point, parameter) pair r = b ndim + i, 64 rows per workgroup, a row per lane of
// each of its four waves.  The derivative of a monomial as the jacobian front end of the GEMM forms it (the powers wave-uniform, the lane's own parameter a
// select; factors of power 0 skipped), a wave the terms tt = wave (mod 4) of a chunk of TY_KC, into one of two LDS buffers m[tt][row] with a bit per term for
// "the term holds no factor of the row's parameter"; wave 0 then adds the chunk to its rows' sums, S[b][t] m over the terms IN THEIR ORDER, while all waves
// form the next chunk (one barrier per chunk) -- forming a term is a chain of scalar loads, branches and LDS reads that one wave per row tile left unhidden
// (profiles/vjp.txt).  A flagged term is SKIPPED, not added as 0 x S: neither a NaN under power 0 nor a NaN of S in such a term reaches G.
// LDS: 2 x 32 x 64 x 8 + ndim x 64 x 8 + 2 x 4 x 64 x 4 bytes, at most 50 KB.
__global__ __launch_bounds__(256) void taylor_input_grad_kernel(const double* x, const double* center, const int* powers, const double* S, const long long R,
                                                                const int ndim, const int T, double* grad) {
    extern __shared__ double ty_lds[];
    double* const mbuf = ty_lds;                                                   // 2 x TY_KC x 64
    double* const dl = ty_lds + 2 * TY_KC * TY_ROWS;                               // (ndim, 64) x - center of the point of each row
    unsigned* const skip = reinterpret_cast<unsigned*>(dl + ndim * TY_ROWS);       // 2 x 4 x 64: bit q of [wave][row] for the term tt = wave + 4 q
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * TY_ROWS + lane;
    const long long point = (r < R ? r : R - 1) / ndim;      // rows past the end repeat the last one (never stored)
    const int mine = (int)((r < R ? r : R - 1) - point * ndim);
    for (int i = wave; i < ndim; i += 4) dl[i * TY_ROWS + lane] = x[point * ndim + i] - center[i];
    __syncthreads();
    const double* Sr = S + point * T;
    const int nchunk = (T + TY_KC - 1) / TY_KC;
    double g = 0.;
#pragma unroll 1
    for (int c = -1; c < nchunk; ++c) {
        if (c + 1 < nchunk) {      // this wave's terms of chunk c + 1
            double* const buf = mbuf + ((c + 1) & 1) * TY_KC * TY_ROWS;
            unsigned flags = 0;
#pragma unroll 1
            for (int q = 0; q < TY_KC / 4; ++q) {
                const int tt = wave + 4 * q, t = (c + 1) * TY_KC + tt;
                double m = 0.;
                bool zero = true;      // terms past T
                if (t < T) {
                    m = 1., zero = false;
                    const int* pw = powers + (long long)t * ndim;
                    for (int i0 = 0; i0 < ndim; i0 += 4) {      // four powers requested at a time (scalar loads: one wait for the four, not one each)
                        int p4[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) p4[k] = __builtin_amdgcn_readfirstlane(pw[i0 + k < ndim ? i0 + k : ndim - 1]);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int i = i0 + k;
                            int p = i < ndim ? p4[k] : 0;      // (past the last parameter: a factor of power 0 of nobody's parameter)
                            if (p <= 0) {
                                zero = zero || mine == i;
                                continue;
                            }
                            p = p < TY_MAX_POWER ? p : TY_MAX_POWER;
                            const double d = dl[i * TY_ROWS + lane];
                            if (p == 1) {
                                m *= mine == i ? 1. : d;
                                continue;
                            }
                            double v = d;      // d^(p - 1)
                            for (int e = 2; e < p; ++e) v *= d;
                            m *= mine == i ? (double)p * v : v * d;
                        }
                    }
                }
                buf[tt * TY_ROWS + lane] = m;
                flags |= zero ? 1u << q : 0u;
            }
            skip[(((c + 1) & 1) * 4 + wave) * TY_ROWS + lane] = flags;
        }
        if (c >= 0 && wave == 0) {      // chunk c, formed before the last barrier, in term order
            const double* const buf = mbuf + (c & 1) * TY_KC * TY_ROWS;
            unsigned flags[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) flags[w] = skip[((c & 1) * 4 + w) * TY_ROWS + lane];
            const int t0 = c * TY_KC, n = T - t0 < TY_KC ? T - t0 : TY_KC;
            for (int tt = 0; tt < n; ++tt) {
                const double m = buf[tt * TY_ROWS + lane], s = Sr[t0 + tt];
                const bool zero = (flags[tt & 3] >> (tt >> 2)) & 1u;
                g = zero ? g : fma(s, m, g);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && r < R) grad[r] = g;
}

// hess[b][i][j] = hess[b][j][i] = sum_t S[b][t] d^2 mono_t / d x_i d x_j for cp_taylor_vjp2: a row per (point, pair i <= j), r = b npairs + p over the pairs in
// the order (0, 0), (0, 1), ..., (1, 1), ...; 64 rows per workgroup, a row per lane of each of its four waves, the chunks, the two buffers, the flags and
// the summing wave of taylor_input_grad_kernel.  The second derivative of a monomial as the jvp2 front end of the GEMM forms its pair terms: the product
// over the parameters of power p > 0 IN THEIR ORDER of p (p - 1) d^(p - 2) (the parameter is i = j), p d^(p - 1) (it is i or j) or d^p, a power formed by
// repeated multiplication and a factor whose exponent is 0 its coefficient alone (the powers wave-uniform, the lane's pair a select; factors of power 0
// skipped).  A term without a factor of x_i or of x_j, or with p < 2 on the diagonal, is flagged and SKIPPED, not added as 0 x S: neither a NaN under
// power 0 nor a NaN of S in such a term reaches the result; an expansion of order 1 gives exactly 0.
// LDS: 2 x 32 x 64 x 8 + ndim x 64 x 8 + 2 x 4 x 64 x 4 bytes, at most 50 KB.
__global__ __launch_bounds__(256) void taylor_curvature_kernel(const double* x, const double* center, const int* powers, const double* S, const long long R,
                                                               const int ndim, const int npairs, const int T, double* hess) {
    extern __shared__ double ty_lds[];
    double* const mbuf = ty_lds;                                                   // 2 x TY_KC x 64
    double* const dl = ty_lds + 2 * TY_KC * TY_ROWS;                               // (ndim, 64) x - center of the point of each row
    unsigned* const skip = reinterpret_cast<unsigned*>(dl + ndim * TY_ROWS);       // 2 x 4 x 64: bit q of [wave][row] for the term tt = wave + 4 q
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * TY_ROWS + lane;
    const long long point = (r < R ? r : R - 1) / npairs;      // rows past the end repeat the last one (never stored)
    int pi = 0, pj = (int)((r < R ? r : R - 1) - point * npairs);
    for (int n = ndim; pj >= n; --n) pj -= n, ++pi;      // parameter i holds the n = ndim - i pairs (i, i) .. (i, ndim - 1)
    pj += pi;
    for (int i = wave; i < ndim; i += 4) dl[i * TY_ROWS + lane] = x[point * ndim + i] - center[i];
    __syncthreads();
    const double* Sr = S + point * T;
    const int nchunk = (T + TY_KC - 1) / TY_KC;
    double g = 0.;
#pragma unroll 1
    for (int c = -1; c < nchunk; ++c) {
        if (c + 1 < nchunk) {      // this wave's terms of chunk c + 1
            double* const buf = mbuf + ((c + 1) & 1) * TY_KC * TY_ROWS;
            unsigned flags = 0;
#pragma unroll 1
            for (int q = 0; q < TY_KC / 4; ++q) {
                const int tt = wave + 4 * q, t = (c + 1) * TY_KC + tt;
                double m = 0.;
                bool zero = true;      // terms past T
                if (t < T) {
                    m = 1., zero = false;
                    const int* pw = powers + (long long)t * ndim;
                    for (int i0 = 0; i0 < ndim; i0 += 4) {      // four powers requested at a time (scalar loads: one wait for the four, not one each)
                        int p4[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) p4[k] = __builtin_amdgcn_readfirstlane(pw[i0 + k < ndim ? i0 + k : ndim - 1]);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int i = i0 + k;
                            int p = i < ndim ? p4[k] : 0;      // (past the last parameter: a factor of power 0 of nobody's parameter)
                            const int times = (pi == i) + (pj == i);      // how often this lane differentiates the factor
                            if (p <= 0) {
                                zero = zero || times > 0;
                                continue;
                            }
                            p = p < TY_MAX_POWER ? p : TY_MAX_POWER;
                            zero = zero || times > p;
                            const double d = dl[i * TY_ROWS + lane];
                            double v2 = 1., v1 = 1., v0 = d;      // d^(p - 2), d^(p - 1), d^p; an exponent of 0 (or less) is 1: the coefficient alone
                            for (int e = 2; e <= p; ++e) v2 = v1, v1 = v0, v0 *= d;
                            m *= times == 0 ? v0 : times == 1 ? (double)p * v1 : (double)(p * (p - 1)) * v2;
                        }
                    }
                }
                buf[tt * TY_ROWS + lane] = m;
                flags |= zero ? 1u << q : 0u;
            }
            skip[(((c + 1) & 1) * 4 + wave) * TY_ROWS + lane] = flags;
        }
        if (c >= 0 && wave == 0) {      // chunk c, formed before the last barrier, in term order
            const double* const buf = mbuf + (c & 1) * TY_KC * TY_ROWS;
            unsigned flags[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) flags[w] = skip[((c & 1) * 4 + w) * TY_ROWS + lane];
            const int t0 = c * TY_KC, n = T - t0 < TY_KC ? T - t0 : TY_KC;
            for (int tt = 0; tt < n; ++tt) {
                const double m = buf[tt * TY_ROWS + lane], s = Sr[t0 + tt];
                const bool zero = (flags[tt & 3] >> (tt >> 2)) & 1u;
                g = zero ? g : fma(s, m, g);
            }
        }
        __syncthreads();
    }
    if (wave == 0 && r < R) {
        double* const hb = hess + point * ndim * ndim;
        hb[pi * ndim + pj] = g;
        hb[pj * ndim + pi] = g;
    }
}

// The GEMM among the launches of the entry point that calls it: its grid's check; the launch status is the entry point's to read
template <int FRONT>
int taylor_launch(cp::Launches& on, const TaylorArgs& A) {
    // the row tiles along x: workgroups are dispatched x first, so those in flight share their 256 columns of the right operand in L2
    const long long nrt = (A.R + TY_ROWS - 1) / TY_ROWS, nct = (A.cend - A.c0 + TY_COLS - 1) / TY_COLS;
    if (nrt > 0x7fffffffLL || nct > 65535) return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d results (at most 2^37 rows, 2^24 - 256 columns)", on.who(), A.R, A.M);
    taylor_gemm_launch<FRONT>(on, A, dim3((unsigned)nrt, (unsigned)nct), A.ndim, 0);
    return CP_OK;
}

// What cp_taylor_predict, cp_taylor_predict_columns, cp_taylor_jacobian, cp_taylor_vjp and cp_taylor_jvp share: their checks, in that order, up to the caps of ndim and
// of the powers; ``ld`` is the entry point's one row stride (of ``what``), which is checked between the range of columns and the caps.  What follows is
// the entry point's own: its grid cap, the empty batch, its null pointers, its workspace, the device.
int taylor_front(const char* who, long long B, int ndim, int T, int max_power, int M, long long col0, long long ncols, long long ld, const char* what) {
    if (B < 0 || ndim < 1 || T < 1 || M < 1) return cp::fail(CP_EINVAL, "%s: need ndim, T, M >= 1 and a non-negative count of points", who);
    if (max_power < 0) return cp::fail(CP_EINVAL, "%s: max_power %d is negative", who, max_power);
    if (col0 < 0 || ncols < 1 || ncols > (long long)M - col0) return cp::fail(CP_EINVAL, "%s: columns [%lld, %lld + %lld) of %d", who, col0, col0, ncols, M);
    if (ld < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the %s is less than its %lld columns", who, ld, what, ncols);
    if (ndim > TY_MAX_NDIM) return cp::fail(CP_EUNSUPPORTED, "%s: %d parameters (at most %d)", who, ndim, TY_MAX_NDIM);
    if (max_power > TY_MAX_POWER) return cp::fail(CP_EUNSUPPORTED, "%s: power %d (at most %d)", who, max_power, TY_MAX_POWER);
    return CP_OK;
}

}  // namespace

// For cp_taylor_gauss_newton (cp_taylor_gauss_newton.hip; declared in cp_internal.h): the checks of taylor_front under its name, and the GEMM of
// cp_taylor_predict_columns on a range inside its device scope.
int cp::taylor_front_checks(const char* who, long long B, int ndim, int T, int max_power, int M, long long col0, long long ncols, long long ld, const char* what) {
    return taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ld, what);
}

int cp::taylor_predict_launch(Launches& on, const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T,
                              const double* d_derivatives, int M, long long col0, long long ncols, double* d_out, long long ldo) {
    const TaylorArgs A{d_x, d_center, d_powers, d_derivatives, d_out, B, ldo, T, M, ndim, (int)col0, (int)(col0 + ncols), 0};
    return taylor_launch<TY_PREDICT>(on, A);
}

// cp_taylor_predict is the range [0, M) with row stride M of the same call
static int taylor_predict(const char* who, const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                          const double* d_derivatives, int M, long long col0, long long ncols, double* d_out, long long ldo, int device, void* stream) {
    const int status = taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ldo, "result");
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    const TaylorArgs A{d_x, d_center, d_powers, d_derivatives, d_out, B, ldo, T, M, ndim, (int)col0, (int)(col0 + ncols), 0};
    cp::Launches on(who, stream);
    const int launched = taylor_launch<TY_PREDICT>(on, A);
    return launched != CP_OK ? launched : on.status();
}

extern "C" int cp_taylor_predict(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                                 const double* d_derivatives, int M, double* d_out, int device, void* stream) {
    return taylor_predict("cp_taylor_predict", d_x, B, d_center, d_powers, ndim, T, max_power, d_derivatives, M, 0, M, d_out, M, device, stream);
}

extern "C" int cp_taylor_predict_columns(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                                         const double* d_derivatives, int M, long long col0, long long ncols, double* d_out, long long ldo, int device,
                                         void* stream) {
    return taylor_predict("cp_taylor_predict_columns", d_x, B, d_center, d_powers, ndim, T, max_power, d_derivatives, M, col0, ncols, d_out, ldo, device, stream);
}

extern "C" int cp_taylor_jacobian(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                                  const double* d_derivatives, int M, long long col0, long long ncols, double* d_jac, long long ldj, int device, void* stream) {
    const char* who = "cp_taylor_jacobian";
    const int status = taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ldj, "Jacobian");
    if (status != CP_OK) return status;
    if (B > 0x7fffffffLL * TY_ROWS / ndim || (ncols + TY_COLS - 1) / TY_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d x %lld results (at most 2^37 rows B ndim, 2^24 - 256 columns)", who, B, ndim, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives || !d_jac) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    const TaylorArgs A{d_x, d_center, d_powers, d_derivatives, d_jac, B * ndim, ldj, T, M, ndim, (int)col0, (int)(col0 + ncols), 0};
    cp::Launches on(who, stream);
    const int launched = taylor_launch<TY_JACOBIAN>(on, A);
    return launched != CP_OK ? launched : on.status();
}

// One launch: the GEMM with the jvp front end on the B K rows (b, k)
extern "C" int cp_taylor_jvp(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                             const double* d_derivatives, int M, long long col0, long long ncols, const double* d_tan, long long K, double* d_out,
                             long long ldo, int device, void* stream) {
    const char* who = "cp_taylor_jvp";
    const int status = taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ldo, "result");
    if (status != CP_OK) return status;
    if (K < 1) return cp::fail(CP_EINVAL, "%s: %lld directions per point (at least 1)", who, K);
    if (K > 0x7fffffffLL || B > 0x7fffffffLL * TY_ROWS / K || (ncols + TY_COLS - 1) / TY_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld x %lld results (at most 2^37 rows B K, 2^31 - 1 directions, 2^24 - 256 columns)", who, B, K, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives || !d_tan || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    const TaylorJvpArgs A{{d_x, d_center, d_powers, d_derivatives, d_out, B * K, ldo, T, M, ndim, (int)col0, (int)(col0 + ncols), 0}, d_tan, (int)K};
    const long long nrt = (B * K + TY_ROWS - 1) / TY_ROWS, nct = (ncols + TY_COLS - 1) / TY_COLS;
    cp::Launches on(who, stream);
    taylor_gemm_launch<TY_JVP>(on, A, dim3((unsigned)nrt, (unsigned)nct), ndim, 0);
    return on.status();
}

// One launch: the GEMM with the jvp2 front end on the B K rows (b, k); d_tan_v NULL: the second directional derivative along d_tan_u
extern "C" int cp_taylor_jvp2(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                              const double* d_derivatives, int M, long long col0, long long ncols, const double* d_tan_u, const double* d_tan_v, long long K,
                              double* d_out, long long ldo, int device, void* stream) {
    const char* who = "cp_taylor_jvp2";
    const int status = taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ldo, "result");
    if (status != CP_OK) return status;
    if (K < 1) return cp::fail(CP_EINVAL, "%s: %lld directions per point (at least 1)", who, K);
    if (K > 0x7fffffffLL || B > 0x7fffffffLL * TY_ROWS / K || (ncols + TY_COLS - 1) / TY_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld x %lld results (at most 2^37 rows B K, 2^31 - 1 directions, 2^24 - 256 columns)", who, B, K, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives || !d_tan_u || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    const TaylorJvp2Args A{{d_x, d_center, d_powers, d_derivatives, d_out, B * K, ldo, T, M, ndim, (int)col0, (int)(col0 + ncols), 0}, d_tan_u, d_tan_v ? d_tan_v : d_tan_u, (int)K};
    const long long nrt = (B * K + TY_ROWS - 1) / TY_ROWS, nct = (ncols + TY_COLS - 1) / TY_COLS;
    cp::Launches on(who, stream);
    taylor_gemm_launch<TY_JVP2>(on, A, dim3((unsigned)nrt, (unsigned)nct), ndim, 0);
    return on.status();
}

extern "C" long long cp_taylor_vjp_workspace_doubles(long long B, int T) {
    if (B < 0 || T < 1) return -(long long)cp::fail(CP_EINVAL, "cp_taylor_vjp_workspace_doubles: need T >= 1 and a non-negative count of points");
    if (B > 0x7fffffffLL * TY_ROWS / TY_MAX_NDIM) return -(long long)cp::fail(CP_EUNSUPPORTED, "cp_taylor_vjp_workspace_doubles: %lld points (at most 2^32)", B);
    return B * T;
}

extern "C" int cp_taylor_vjp(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                             const double* d_derivatives_t, int M, long long col0, long long ncols, const double* d_cot, long long ldc, double* d_grad,
                             double* d_work, long long work_doubles, int device, void* stream) {
    const char* who = "cp_taylor_vjp";
    const int status = taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ldc, "cotangent");
    if (status != CP_OK) return status;
    if (B > 0x7fffffffLL * TY_ROWS / ndim || (T + TY_COLS - 1) / TY_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d gradients of %d terms (at most 2^37 rows B ndim, 2^24 - 256 terms)", who, B, ndim, T);
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives_t || !d_cot || !d_grad || !d_work) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    if (work_doubles < B * T) return cp::fail(CP_EINVAL, "%s: workspace of %lld doubles, %lld needed (cp_taylor_vjp_workspace_doubles)", who, work_doubles, B * T);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    // S (B, T) = cot (B, ncols) . Dt[col0 : col0 + ncols] (ncols, T)
    const TaylorArgs A{d_cot, nullptr, nullptr, d_derivatives_t + col0 * T, d_work, B, T, (int)ncols, T, 0, 0, T, ldc};
    cp::Launches on(who, stream);
    const int launched = taylor_launch<TY_FIT>(on, A);
    if (launched != CP_OK) return launched;
    const long long R = B * ndim;
    on.run<taylor_input_grad_kernel>((unsigned)((R + TY_ROWS - 1) / TY_ROWS), 256, (size_t)(2 * TY_KC + ndim) * TY_ROWS * sizeof(double) + 2 * 4 * TY_ROWS * sizeof(unsigned),
                                     d_x, d_center, d_powers, d_work, R, ndim, T, d_grad);
    return on.status();
}

extern "C" long long cp_taylor_vjp2_workspace_doubles(long long B, int T) {
    if (B < 0 || T < 1) return -(long long)cp::fail(CP_EINVAL, "cp_taylor_vjp2_workspace_doubles: need T >= 1 and a non-negative count of points");
    if (B > 0x7fffffffLL * TY_ROWS / (TY_MAX_NDIM * (TY_MAX_NDIM + 1) / 2))
        return -(long long)cp::fail(CP_EUNSUPPORTED, "cp_taylor_vjp2_workspace_doubles: %lld points (at most 2^28)", B);
    return B * T;
}

// Two launches: the S GEMM of cp_taylor_vjp, then taylor_curvature_kernel on the B ndim (ndim + 1) / 2 rows (b, i <= j)
extern "C" int cp_taylor_vjp2(const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, int max_power,
                              const double* d_derivatives_t, int M, long long col0, long long ncols, const double* d_cot, long long ldc, double* d_hess,
                              double* d_work, long long work_doubles, int device, void* stream) {
    const char* who = "cp_taylor_vjp2";
    const int status = taylor_front(who, B, ndim, T, max_power, M, col0, ncols, ldc, "cotangent");
    if (status != CP_OK) return status;
    const int npairs = ndim * (ndim + 1) / 2;
    if (B > 0x7fffffffLL * TY_ROWS / npairs || (T + TY_COLS - 1) / TY_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d x %d second derivatives of %d terms (at most 2^37 rows B ndim (ndim + 1) / 2, 2^24 - 256 terms)", who, B, ndim, ndim, T);
    if (B == 0) return CP_OK;
    if (!d_x || !d_center || !d_powers || !d_derivatives_t || !d_cot || !d_hess || !d_work) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    if (work_doubles < B * T) return cp::fail(CP_EINVAL, "%s: workspace of %lld doubles, %lld needed (cp_taylor_vjp2_workspace_doubles)", who, work_doubles, B * T);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    // S (B, T) = cot (B, ncols) . Dt[col0 : col0 + ncols] (ncols, T)
    const TaylorArgs A{d_cot, nullptr, nullptr, d_derivatives_t + col0 * T, d_work, B, T, (int)ncols, T, 0, 0, T, ldc};
    cp::Launches on(who, stream);
    const int launched = taylor_launch<TY_FIT>(on, A);
    if (launched != CP_OK) return launched;
    const long long R = B * npairs;
    on.run<taylor_curvature_kernel>((unsigned)((R + TY_ROWS - 1) / TY_ROWS), 256, (size_t)(2 * TY_KC + ndim) * TY_ROWS * sizeof(double) + 2 * 4 * TY_ROWS * sizeof(unsigned),
                                    d_x, d_center, d_powers, d_work, R, ndim, npairs, T, d_hess);
    return on.status();
}

extern "C" int cp_taylor_fit(const double* d_S, int T, int npoints, const double* d_Y, int M, double* d_derivatives, int device, void* stream) {
    if (T < 1 || npoints < 1 || M < 1) return cp::fail(CP_EINVAL, "cp_taylor_fit: need T, npoints, M >= 1");
    if (!d_S || !d_Y || !d_derivatives) return cp::fail(CP_EINVAL, "cp_taylor_fit: null pointer");
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_taylor_fit: cannot select device %d", device);
    const TaylorArgs A{d_S, nullptr, nullptr, d_Y, d_derivatives, T, M, npoints, M, 0, 0, M, npoints};
    cp::Launches on("cp_taylor_fit", stream);
    const int launched = taylor_launch<TY_FIT>(on, A);
    return launched != CP_OK ? launched : on.status();
}
