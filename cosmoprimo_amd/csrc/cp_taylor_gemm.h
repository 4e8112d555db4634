// cp_taylor_gemm.h -- the GEMM kernel of the Taylor emulator, written ONCE as a __global__ template for the five front ends of its left operand (included by
// cp_taylor.hip: fit, predict, jacobian, jvp; and by cp_taylor_gauss_newton.hip: Gauss-Newton), with the device functions, tile constants and argument
// structs that go with it.  out (R, M) = left (R, K) . b (K, M) in float64 on the matrix cores; the front end says what a row is and how its entries of the
// left operand are formed in LDS, chunk of 32 inner indices by chunk -- the left operand never exists in memory but for the fit:
//   TY_FIT           TaylorArgs     the left operand is read from memory (the fit's weights; the cotangent of cp_taylor_vjp)
//   TY_PREDICT       TaylorArgs     a row is a point, its entries the monomials prod_j (x_j - c_j)^p_tj
//   TY_JACOBIAN      TaylorArgs     a row is a (point, parameter) pair r = b ndim + i (64 is no multiple of most ndim: a point's rows may lie in two
//                                   workgroups, every lane finds its own b and i), its entries d mono_t / d x_i = p_ti (x_i - c_i)^(p_ti - 1) prod_{j != i} ...
//   TY_JVP           TaylorJvpArgs  a row is a (point, direction) pair r = b K + k, its entries sum_i tan[b][k][i] d mono_t / d x_i (details at the front end)
//   TY_JVP2          TaylorJvp2Args a row is a (point, pair of directions) r = b K + k, its entries sum_ij u_i v_j d^2 mono_t / d x_i d x_j (details at the front end;
//                                   three (ndim, 64) arrays beside the operand buffers, at most 88 KB: one workgroup per CU above ndim = 26)
//   TY_GAUSS_NEWTON  TaylorGnArgs   the entries of the jacobian front end with the rows of cp_gauss_newton.h -- a row tile holds P = floor(64 / ndim) whole
//                                   points, row t = p ndim + i -- and its epilogue in the place of the store: the tile of the Jacobian is never stored
// Every kernel is held to its instructions (tools/compare_device_code.py).  Source is shared by writing one __global__ template whose variants differ under
// `if constexpr` only: a device function holding the shared body changed the instructions of its callers, and copies of the body were three bodies to keep
// equal by hand.  DESIGN.md section 4 ('One source for the forward-mode derivative kernels') has the comparison.
//
// Mapping.  A workgroup of four waves owns 64 rows x 256 columns of the result; the waves sit side by side in the columns on the same rows, each with
// a tile of 64 x 64 (4 x 4 accumulator tiles of 16 x 16, 128 registers: the tile of linop_mfma_kernel, cp_spline.hip).  Fragments of the f64 form
// (cdna_hip_programming.md): lane l supplies A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15], and holds D[row = (l >> 4) + 4 r][col = l & 15]
// in register r.  The right operand is row-major with the columns contiguous, so the 16 lanes of a k read 128 contiguous bytes; it is read straight
// from L1 / L2 (a wave fetches 2 KB per 16 MFMAs = 8 B per matrix-core cycle, half of what linop_mfma_kernel needs, because the left operand comes
// from LDS).  The row tiles run along grid x, which is dispatched first: the workgroups in flight share their 256 columns of the right operand in L2.
// LDS.  The left operand of a chunk of TY_KC = 32 inner indices is stored k-major, a[k][row], with a row stride of 80 doubles: ds_read_b64 banks 32-lane
// halves over 64 dwords, and a half holds two values of k (lanes l and l + 16), which a stride of 16 mod 32 doubles puts on opposite halves of the
// bank row -- conflict-free reads; the writes of a term go to 64 consecutive doubles.  Two such buffers alternate, so a chunk costs one barrier;
// 2 x 32 x 80 x 8 = 40 KB plus ndim x 64 x 8 (at most 16 KB) for x - center, and as much again for the tangents of the jvp (at most 72 KB in all): two
// workgroups per CU at any T.  The Gauss-Newton epilogue reuses the buffers; where it needs more (cp_gauss_newton.h), the launch asks for that.
// Monomials.  A wave forms whole terms, lane = row: the powers of a term are wave-uniform (scalar loads, uniform branches), factors with power 0 are
// skipped -- they contribute exactly 1 whatever x - center holds (NaN, Inf: the reference's `where`, taylor.py:246) -- and a power is formed by repeated
// multiplication.
#pragma once
#include "cp_gauss_newton.h"

namespace {

typedef double ty_v4d __attribute__((ext_vector_type(4)));

constexpr int TY_ROWS = 64, TY_COLS = 256, TY_KC = 32, TY_RS = 80, TY_MAX_NDIM = 32, TY_MAX_POWER = 15;
enum { TY_FIT = 0, TY_PREDICT = 1, TY_JACOBIAN = 2, TY_JVP = 3, TY_GAUSS_NEWTON = 4, TY_JVP2 = 5 };      // the front end of the left operand

struct TaylorArgs {
    const double* a;        // predict: x (R, ndim); jacobian: x (R / ndim, ndim), row r the point r / ndim and the parameter r % ndim; fit: the left operand (R, K)
                            // with row stride lda
    const double* center;   // (ndim)
    const int* powers;      // (K, ndim)
    const double* b;        // (K, M)
    double* out;            // (R, ncols) with row stride ldo: the columns [c0, cend) of the (R, M) product
    long long R, ldo;
    int K, M, ndim;
    int c0, cend;           // the column tiles start at c0 (any value: the fragments are fetched with 8-byte loads); nothing outside [c0, cend) of b is read
    long long lda;          // fit
};

struct TaylorJvpArgs : TaylorArgs {      // a: x (B, ndim); R = B K rows of the result
    const double* tan;      // (B, K, ndim)
    int Kdir;               // K directions per point
};

struct TaylorJvp2Args : TaylorArgs {     // a: x (B, ndim); R = B K rows of the result
    const double* tan_u;    // (B, K, ndim)
    const double* tan_v;    // (B, K, ndim); tan_u again for the second directional derivative
    int Kdir;               // K pairs of directions per point
};

struct TaylorGnArgs {
    const double* x;          // (B, ndim)
    const double* center;     // (ndim)
    const int* powers;        // (T, ndim)
    const double* b;          // (T, M) derivatives
    int K, M;                 // T terms, M columns of b
    cpgn::Tail tail;
};

// The operands of the eight inner indices k0 + 8 p .. + 7 of one chunk for one wave: two MFMA steps.  A row of the right operand past K is never read:
// its place in the left operand is 0, and 0 x NaN would not be (row 0 is fetched in its place and masked by taylor_mask).
template <class Args>
__device__ __forceinline__ void taylor_load(const Args& A, const double* buf, const int k0, const int p, const int l15, const int g, const int (&colj)[4],
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
        for (int i = 0; i < 4; ++i) a[h][i] = buf[kk * TY_RS + 16 * i + l15];
    }
}

// ... and what was fetched for rows past K set to zero; kept apart from the loads so that nothing waits for them before the MFMAs they are to hide behind
__device__ __forceinline__ void taylor_mask(double (&b)[2][4], const bool (&keep)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = keep[h] ? b[h][j] : 0.;
}

// u_i v_j + u_j v_i of the jvp2 front end, both products and the sum rounded on their own (no fused multiply-add): the same bits with u and v exchanged
__device__ __forceinline__ double taylor_pair(double ui, double vj, double uj, double vi) {
#pragma clang fp contract(off)
    return ui * vj + uj * vi;
}

template <int FRONT, class Args>
__global__ __launch_bounds__(256, 2) void taylor_gemm_kernel(const Args A) {
    constexpr bool GEN = FRONT != TY_FIT, JVP = FRONT == TY_JVP, JVP2 = FRONT == TY_JVP2, GN = FRONT == TY_GAUSS_NEWTON, DER = FRONT == TY_JACOBIAN || GN;
    extern __shared__ double ty_lds[];
    // ndim is read from the argument where a variant first uses it, not once up here for all: the place of that one scalar load decided the register
    // allocation of the predict, jacobian and Gauss-Newton instantiations, and every kernel is held to its instructions
    int ndim = 0;
    if constexpr (GN) ndim = A.tail.ndim;
    double* const abuf = ty_lds;                       // 2 x TY_KC x TY_RS
    double* const dl = ty_lds + 2 * TY_KC * TY_RS;     // GEN: (ndim, 64) x - center of the point of each of the tile's rows
    double* tl = nullptr;                              // jvp: (ndim, 64) the tangent of each row
    if constexpr (JVP || JVP2) tl = dl + A.ndim * TY_ROWS;
    [[maybe_unused]] double* tl2 = nullptr;            // jvp2: (ndim, 64) the second tangent of each row
    if constexpr (JVP2) tl2 = tl + A.ndim * TY_ROWS;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int nchunk = (A.K + TY_KC - 1) / TY_KC;
    // One tile per workgroup (a loop over tiles here made the compiler keep the 64 store addresses of a lane alive through the MFMAs: spills).
    // jacobian, jvp: the tile's first row, its point and the parameter or direction it stands for: row0 + t is point b0 + (i0 + t) / nd, and (jacobian)
    // this lane's parameter.  Gauss-Newton: the tile's first point: row t is point b0 + t / ndim, parameter t % ndim.
    // The range of columns and the row stride of the result; the fit takes every column, known at compile time.
    long long row0 = 0, b0 = 0, ldo = 0;
    int c0, cend, i0 = 0, mine = 0;
    if constexpr (GN) {
        b0 = (long long)blockIdx.x * A.tail.P;
        c0 = A.tail.c0, cend = A.tail.cend;
    } else {
        row0 = (long long)blockIdx.x * TY_ROWS;
        c0 = GEN ? A.c0 : 0, cend = GEN ? A.cend : A.M;
        ldo = GEN ? A.ldo : (long long)A.M;
    }
    const int col0 = c0 + (int)blockIdx.y * TY_COLS + wave * 64;
    [[maybe_unused]] const bool active = col0 < cend;      // (wave-uniform; an idle wave forms its share of the left operand and multiplies the last column: no branch round the MFMAs)
    if constexpr (GN) {
        mine = lane % ndim;
    } else if constexpr (JVP || JVP2) {
        b0 = row0 / A.Kdir;
        i0 = (int)(row0 - b0 * A.Kdir);
    } else if constexpr (DER) {
        ndim = A.ndim;
        b0 = row0 / ndim;
        i0 = (int)(row0 - b0 * ndim);
        mine = (i0 + lane) % ndim;
    }
    if constexpr (!GN) ndim = A.ndim;
    if constexpr (GEN) {
        for (int e = threadIdx.x; e < ndim * TY_ROWS; e += 256) {
            const int i = e >> 6;
            if constexpr (GN) {
                const int p = (e & 63) / ndim;
                dl[e] = p < A.tail.P && b0 + p < A.tail.B ? A.x[(b0 + p) * ndim + i] - A.center[i] : 0.;      // idle rows and points past the end: finite, never stored
            } else if constexpr (JVP2) {
                const long long row = row0 + (e & 63);
                const long long point = b0 + (i0 + (e & 63)) / A.Kdir;
                const bool inside = row < A.R;      // rows past the end: finite, never stored
                dl[e] = inside ? A.a[point * ndim + i] - A.center[i] : 0.;
                tl[e] = inside ? A.tan_u[row * ndim + i] : 0.;
                tl2[e] = inside ? A.tan_v[row * ndim + i] : 0.;
            } else if constexpr (JVP) {
                const long long row = row0 + (e & 63);
                const long long point = b0 + (i0 + (e & 63)) / A.Kdir;
                const bool inside = row < A.R;      // rows past the end: finite, never stored
                dl[e] = inside ? A.a[point * ndim + i] - A.center[i] : 0.;
                tl[e] = inside ? A.tan[row * ndim + i] : 0.;
            } else {
                const long long row = row0 + (e & 63);
                const long long point = DER ? b0 + (i0 + (e & 63)) / ndim : row;
                dl[e] = row < A.R ? A.a[point * ndim + i] - A.center[i] : 0.;      // rows past the end: finite, never stored
            }
        }
        __syncthreads();
    }
    ty_v4d acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = ty_v4d{0., 0., 0., 0.};
    int colj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        colj[j] = col < cend ? col : cend - 1;      // columns past the end of the range repeat its last one (never stored; their weight is 0 in the Gauss-Newton epilogue)
    }
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        double* const buf = abuf + (c & 1) * TY_KC * TY_RS;
        const int k0 = c * TY_KC;
        if constexpr (JVP2) {
            // The entry of term t is sum over the marked parameters i <= j in parameter order, i outer and j inner, of
            //   c_ij d^2 mono_t / d x_i d x_j,   c_ii = u_i v_i,   c_ij = u_i v_j + u_j v_i  (each product and the sum rounded on its own: exchanging u and v
            // gives the same bits) -- the full double sum over (i, j) with the two equal mixed derivatives taken together.  The derivative is the product
            // over the marked q IN THEIR ORDER of p (p - 1) d^(p - 2) (q = i = j; the pair is skipped for p < 2), p d^(p - 1) (q = i or j) or d^p; a factor
            // whose exponent is 0 is its coefficient alone.  Parameters of power 0 are skipped, not multiplied: neither they nor their tangent components
            // are read.  A term of total order < 2 has no pair: exactly 0.
            for (int tt = wave; tt < TY_KC; tt += 4) {      // a term per wave and step, a row per lane
                const int t = k0 + tt;
                double s = 0.;      // terms past T: zero columns of the left operand
                if (t < A.K) {
                    const int* pw = A.powers + (long long)t * ndim;
                    unsigned marked = 0;
                    unsigned long long plo = 0, phi = 0;
                    for (int i0 = 0; i0 < ndim; i0 += 4) {
                        int p4[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) p4[k] = __builtin_amdgcn_readfirstlane(pw[i0 + k < ndim ? i0 + k : ndim - 1]);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int i = i0 + k;
                            int p = i < ndim ? p4[k] : 0;
                            if (p <= 0) continue;
                            p = p < TY_MAX_POWER ? p : TY_MAX_POWER;
                            marked |= 1u << i;
                            if (i < 16) plo |= (unsigned long long)p << (4 * i);
                            else phi |= (unsigned long long)p << (4 * (i - 16));
                        }
                    }
                    for (unsigned mi = marked; mi; mi &= mi - 1) {
                        const int i = __builtin_ctz(mi);
                        const int pi = (int)((i < 16 ? plo >> (4 * i) : phi >> (4 * (i - 16))) & 15);
                        const double ui = tl[i * TY_ROWS + lane], vi = tl2[i * TY_ROWS + lane];
                        for (unsigned mj = mi; mj; mj &= mj - 1) {      // j >= i
                            const int j = __builtin_ctz(mj);
                            if (j == i && pi < 2) continue;
                            double m = 1.;
                            for (unsigned mq = marked; mq; mq &= mq - 1) {
                                const int q = __builtin_ctz(mq);
                                const int p = (int)((q < 16 ? plo >> (4 * q) : phi >> (4 * (q - 16))) & 15);
                                const int r = (q == i) + (q == j);      // how often this factor is differentiated
                                const int e = p - r;
                                const double c = (double)(r == 0 ? 1 : r == 1 ? p : p * (p - 1));
                                if (e == 0) {
                                    if (r) m *= c;
                                    continue;
                                }
                                const double d = dl[q * TY_ROWS + lane];
                                double v = d;      // d^e
                                for (int x = 1; x < e; ++x) v *= d;
                                m *= r ? c * v : v;
                            }
                            const double cij = j == i ? ui * vi : taylor_pair(ui, tl2[j * TY_ROWS + lane], tl[j * TY_ROWS + lane], vi);
                            s = fma(cij, m, s);
                        }
                    }
                }
                buf[tt * TY_RS + lane] = s;
            }
        } else if constexpr (JVP) {
            // A wave forms whole terms, lane = row: one pass over the powers of the term (wave-uniform) marks the parameters with p_ti > 0 in a mask and packs
            // their powers into scalar registers; then, per marked i in parameter order, d mono_t / d x_i is the product over the marked j IN THEIR ORDER of
            // p d^(p - 1) (j = i) or d^p (else), each factor formed as the jacobian front end forms it, and is added as fma(tan_i, ., sum).  A parameter with
            // p_ti = 0 is skipped, not added as 0 x: a NaN or Inf in a parameter, or in its tangent component, that only ever has power 0 never reaches the
            // result; with K = ndim identity tangents the entry is fma(1, m_i, 0 + 0 x m_j ...) = the jacobian front end's m_i, bit for bit on finite inputs.
            for (int tt = wave; tt < TY_KC; tt += 4) {      // a term per wave and step, a row per lane
                const int t = k0 + tt;
                double s = 0.;      // terms past T: zero columns of the left operand
                if (t < A.K) {
                    const int* pw = A.powers + (long long)t * ndim;
                    // one pass over the powers, four scalar loads in flight: bit i of marked for p_ti > 0 (ndim <= 32), the powers themselves (at most 15) in four
                    // bits each of two scalar registers -- the loops below read no memory but the lanes' LDS
                    unsigned marked = 0;
                    unsigned long long plo = 0, phi = 0;
                    for (int i0 = 0; i0 < ndim; i0 += 4) {
                        int p4[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) p4[k] = __builtin_amdgcn_readfirstlane(pw[i0 + k < ndim ? i0 + k : ndim - 1]);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int i = i0 + k;
                            int p = i < ndim ? p4[k] : 0;
                            if (p <= 0) continue;
                            p = p < TY_MAX_POWER ? p : TY_MAX_POWER;
                            marked |= 1u << i;
                            if (i < 16) plo |= (unsigned long long)p << (4 * i);
                            else phi |= (unsigned long long)p << (4 * (i - 16));
                        }
                    }
                    for (unsigned mi = marked; mi; mi &= mi - 1) {
                        const int i = __builtin_ctz(mi);
                        double m = 1.;
                        for (unsigned mj = marked; mj; mj &= mj - 1) {
                            const int j = __builtin_ctz(mj);
                            const int p = (int)((j < 16 ? plo >> (4 * j) : phi >> (4 * (j - 16))) & 15);
                            const double d = dl[j * TY_ROWS + lane];
                            if (p == 1) {
                                if (j != i) m *= d;
                                continue;
                            }
                            double v = d;      // d^(p - 1)
                            for (int q = 2; q < p; ++q) v *= d;
                            m *= j == i ? (double)p * v : v * d;
                        }
                        s = fma(tl[i * TY_ROWS + lane], m, s);
                    }
                }
                buf[tt * TY_RS + lane] = s;
            }
        } else if constexpr (DER) {
            // d / dx_mine of the monomial: the factor of this lane's parameter is p d^(p - 1) -- exactly 0 for p = 0 whatever the other factors hold, and
            // without d for p = 1 --, the others d^p as in predict; the powers are wave-uniform, the lane's parameter a select
            for (int tt = wave; tt < TY_KC; tt += 4) {
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
                        p = p < TY_MAX_POWER ? p : TY_MAX_POWER;
                        const double d = dl[i * TY_ROWS + lane];
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
                buf[tt * TY_RS + lane] = m;
            }
        } else if constexpr (GEN) {
            for (int tt = wave; tt < TY_KC; tt += 4) {      // a term per wave and step, a row per lane
                const int t = k0 + tt;
                double m = 0.;      // terms past T: zero columns of the left operand
                if (t < A.K) {
                    m = 1.;
                    const int* pw = A.powers + (long long)t * ndim;
                    for (int i = 0; i < ndim; ++i) {
                        int p = __builtin_amdgcn_readfirstlane(pw[i]);
                        if (p <= 0) continue;
                        p = p < TY_MAX_POWER ? p : TY_MAX_POWER;
                        const double d = dl[i * TY_ROWS + lane];
                        double v = d;
                        for (int q = 1; q < p; ++q) v *= d;
                        m *= v;
                    }
                }
                buf[tt * TY_RS + lane] = m;
            }
        } else {
            for (int e = threadIdx.x; e < TY_ROWS * TY_KC; e += 256) {
                const int r = e / TY_KC, kk = e % TY_KC;      // k along the lanes: the rows of S are contiguous in k
                const long long row = row0 + r;
                const int k = k0 + kk;
                buf[kk * TY_RS + r] = (row < A.R && k < A.K) ? A.a[row * A.lda + k] : 0.;
            }
        }
        __syncthreads();      // one barrier per chunk: the buffer written next was last read before this barrier
        // One loop for full and partial chunks, and no branch round it: with the MFMAs on two paths the compiler kept two sets of accumulators and
        // spilled.  Pairs of steps, the operands of the next pair fetched before the 32 MFMAs of this one (the last pair fetches itself again).
        const int npairs = A.K - k0 >= TY_KC ? TY_KC / 8 : (A.K - k0 + 7) / 8;
        double a0[2][4], b0r[2][4];
        bool keep[2];
        taylor_load(A, buf, k0, 0, l15, g, colj, a0, b0r, keep);
        taylor_mask(b0r, keep);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            taylor_load(A, buf, k0, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1, keep);
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
            taylor_mask(b0r, keep);
        }
    }
    if constexpr (GN) {
        __syncthreads();      // every wave has read the last chunk: the epilogue takes the LDS over
        cpgn::gn_contract<cpgn::GN_Y_PLAIN>(A.tail, nullptr, acc, ty_lds + wave * (cpgn::epilogue_lds_doubles(A.tail.P, ndim) / 4), lane, b0, col0);
        cpgn::gn_combine(A.tail, ty_lds, b0, (int)blockIdx.y);
    } else {
        if (!active) return;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = col0 + 16 * j + l15;
            if (col >= cend) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long row = row0 + 16 * i + g + 4 * r;
                    if (row < A.R) A.out[row * ldo + (col - c0)] = acc[i][j][r];
                }
        }
    }
}

// The GEMM on the stream for the front end FRONT, inside the caller's device scope.  LDS: the two operand buffers, x - center, the jvp's tangents (at most
// 72 KB), or the Gauss-Newton epilogue's `epilogue` doubles where those are more.
template <int FRONT, class Args>
void taylor_gemm_launch(cp::Launches& on, const Args& A, const dim3 grid, const int ndim, const size_t epilogue) {
    const size_t gemm = (size_t)2 * TY_KC * TY_RS + (size_t)(FRONT == TY_FIT ? 0 : FRONT == TY_JVP2 ? 3 : FRONT == TY_JVP ? 2 : 1) * ndim * TY_ROWS;
    on.run<taylor_gemm_kernel<FRONT, Args>>(grid, 256, (gemm > epilogue ? gemm : epilogue) * sizeof(double), A);
}

}  // namespace
