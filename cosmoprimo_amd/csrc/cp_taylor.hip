// cp_taylor.hip -- Taylor-expansion emulator of a calculator (reference emulators/tools/taylor.py:211-247) for batches of parameter points (gfx950)
// + C ABI.  One GEMM kernel in float64 on the matrix cores (v_mfma_f64_16x16x4_f64) with three front ends for its left operand:
//   predict : out (B, M) = monomials (B, T) . derivatives (T, M); the monomials of a tile of rows are formed in LDS, chunk of terms by chunk of terms,
//             from x - center and the integer powers -- the (B, T) matrix never exists in memory
//   fit     : derivatives (T, M) = S (T, npoints) . Y (npoints, M); S (the finite-difference weights of every term, built on the host) is staged
//             through the same LDS tiles
//   jacobian: jac (B ndim, M) = d monomials / d x_i (B ndim, T) . derivatives; a row is a (point, parameter) pair r = b ndim + i (64 is no multiple of
//             most ndim: a point's rows may lie in two workgroups, every lane finds its own b and i), its entry for term t the derivative of the
//             monomial, p_ti (x_i - c_i)^(p_ti - 1) prod_{j != i} (x_j - c_j)^p_tj, formed in LDS chunk by chunk as the monomials are
// Mapping.  A workgroup of four waves owns 64 rows x 256 columns of the result; the waves sit side by side in the columns on the same rows, each with
// a tile of 64 x 64 (4 x 4 accumulator tiles of 16 x 16, 128 registers: the tile of linop_mfma_kernel, cp_spline.hip).  Fragments of the f64 form
// (cdna_hip_programming.md): lane l supplies A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15], and holds D[row = (l >> 4) + 4 r][col = l & 15]
// in register r.  The right operand is row-major with the columns contiguous, so the 16 lanes of a k read 128 contiguous bytes; it is read straight
// from L1 / L2 (a wave fetches 2 KB per 16 MFMAs = 8 B per matrix-core cycle, half of what linop_mfma_kernel needs, because the left operand comes
// from LDS).  The row tiles run along grid x, which is dispatched first: the workgroups in flight share their 256 columns of the right operand in L2.
// LDS.  The left operand of a chunk of TY_KC = 32 inner indices is stored k-major, a[k][row], with a row stride of 80 doubles: ds_read_b64 banks 32-lane
// halves over 64 dwords, and a half holds two values of k (lanes l and l + 16), which a stride of 16 mod 32 doubles puts on opposite halves of the
// bank row -- conflict-free reads; the writes of a term go to 64 consecutive doubles.  Two such buffers alternate, so a chunk costs one barrier;
// 2 x 32 x 80 x 8 = 40 KB plus ndim x 64 x 8 (at most 16 KB) for x - center: two workgroups per CU at any T.
// Monomials.  A wave forms whole terms, lane = row: the powers of a term are wave-uniform (scalar loads, uniform branches), factors with power 0 are
// skipped -- they contribute exactly 1 whatever x - center holds (NaN, Inf: the reference's `where`, taylor.py:246) -- and a power is formed by repeated
// multiplication.
// Vector-Jacobian product (cp_taylor_vjp: G (B, ndim) = cot . d predict / d x).  Two launches: S (B, T) = cot (B, ncols) . D[:, columns]^T is the GEMM with
// the front end of the fit -- both operands are then contiguous as that front end wants them, the left one (cot, row stride lda) along the contraction
// and the right one, rows [col0, col0 + ncols) of a TRANSPOSED copy (M, T) of the derivatives that the caller keeps, along the terms -- and
// taylor_input_grad_kernel contracts S with the derivatives of the monomials, which it forms as the jacobian front end does.  No (B, ndim, .) array exists.
// Jacobian-vector product (cp_taylor_jvp: out (B K, M) = [tan . d monomials / d x] (B K, T) . derivatives along K directions per point).  One launch of
// taylor_jvp_kernel, the GEMM with a fourth front end of its left operand as a kernel of its own; details above it.  No (B, ndim, .) array exists.
#include "cp_internal.h"

namespace {

typedef double ty_v4d __attribute__((ext_vector_type(4)));

constexpr int TY_ROWS = 64, TY_COLS = 256, TY_KC = 32, TY_RS = 80, TY_MAX_NDIM = 32, TY_MAX_POWER = 15;
enum { TY_FIT = 0, TY_PREDICT = 1, TY_JACOBIAN = 2 };      // the front end of the left operand

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

// The operands of the eight inner indices k0 + 8 p .. + 7 of one chunk for one wave: two MFMA steps.  A row of the right operand past K is never read:
// its place in the left operand is 0, and 0 x NaN would not be (row 0 is fetched in its place and masked by taylor_mask).
__device__ __forceinline__ void taylor_load(const TaylorArgs& A, const double* buf, const int k0, const int p, const int l15, const int g, const int (&colj)[4],
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

template <int FRONT>
__global__ __launch_bounds__(256, 2) void taylor_gemm_kernel(const TaylorArgs A) {
    constexpr bool GEN = FRONT != TY_FIT, DER = FRONT == TY_JACOBIAN;
    extern __shared__ double ty_lds[];
    double* const abuf = ty_lds;                       // 2 x TY_KC x TY_RS
    double* const dl = ty_lds + 2 * TY_KC * TY_RS;     // GEN: (ndim, 64) x - center of the tile's rows
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int nchunk = (A.K + TY_KC - 1) / TY_KC;
    {      // one tile per workgroup (a loop over tiles here made the compiler keep the 64 store addresses of a lane alive through the MFMAs: spills)
        const long long row0 = (long long)blockIdx.x * TY_ROWS;
        // the range of columns and the row stride of the result; the fit takes every column, known at compile time (its code is what it was)
        const int c0 = GEN ? A.c0 : 0, cend = GEN ? A.cend : A.M;
        const long long ldo = GEN ? A.ldo : (long long)A.M;
        const int col0 = c0 + (int)blockIdx.y * TY_COLS + wave * 64;
        const bool active = col0 < cend;      // (wave-uniform; an idle wave forms its share of the left operand and multiplies the last column: no branch round the MFMAs)
        // jacobian: the tile's first point and the parameter its first row stands for (row0 + t is point b0 + (i0 + t) / ndim), and this lane's parameter
        const long long b0 = DER ? row0 / A.ndim : 0;
        const int i0 = DER ? (int)(row0 - b0 * A.ndim) : 0;
        const int mine = DER ? (i0 + lane) % A.ndim : 0;
        if (GEN) {
            for (int e = threadIdx.x; e < A.ndim * TY_ROWS; e += 256) {
                const int i = e >> 6;
                const long long row = row0 + (e & 63);
                const long long point = DER ? b0 + (i0 + (e & 63)) / A.ndim : row;
                dl[e] = row < A.R ? A.a[point * A.ndim + i] - A.center[i] : 0.;      // rows past the end: finite, never stored
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
            colj[j] = col < cend ? col : cend - 1;      // columns past the end of the range repeat its last one (never stored)
        }
#pragma unroll 1
        for (int c = 0; c < nchunk; ++c) {
            double* const buf = abuf + (c & 1) * TY_KC * TY_RS;
            const int k0 = c * TY_KC;
            if (DER) {
                // d / dx_mine of the monomial: the factor of this lane's parameter is p d^(p - 1) -- exactly 0 for p = 0 whatever the other factors hold, and
                // without d for p = 1 --, the others d^p as in predict; the powers are wave-uniform, the lane's parameter a select
                for (int tt = wave; tt < TY_KC; tt += 4) {
                    const int t = k0 + tt;
                    double m = 0.;
                    if (t < A.K) {
                        m = 1.;
                        bool zero = false;
                        const int* pw = A.powers + (long long)t * A.ndim;
                        for (int i = 0; i < A.ndim; ++i) {
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
            } else if (GEN) {
                for (int tt = wave; tt < TY_KC; tt += 4) {      // a term per wave and step, a row per lane
                    const int t = k0 + tt;
                    double m = 0.;      // terms past T: zero columns of the left operand
                    if (t < A.K) {
                        m = 1.;
                        const int* pw = A.powers + (long long)t * A.ndim;
                        for (int i = 0; i < A.ndim; ++i) {
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
            double a0[2][4], b0[2][4];
            bool keep[2];
            taylor_load(A, buf, k0, 0, l15, g, colj, a0, b0, keep);
            taylor_mask(b0, keep);
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
                        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[h][i], b0[h][j], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < 4; ++i) a0[h][i] = a1[h][i], b0[h][i] = b1[h][i];
                __builtin_amdgcn_sched_barrier(0);
                taylor_mask(b0, keep);
            }
        }
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

// Directional derivatives (cp_taylor_jvp): out (B K, M) = [sum_i tan[b][k][i] d mono_t / d x_i] (B K, T) . derivatives -- the tile, chunks, operand fetch and
// MFMA sequence of taylor_gemm_kernel with one more front end of its left operand (a kernel of its own: TaylorArgs, and with it every symbol of the GEMM,
// stays what it is).  A row is a (point, direction) pair r = b K + k; 64 is no multiple of most K, so a point's rows may lie in two workgroups and every
// lane finds its own b.  A wave forms whole terms, lane = row: one pass over the powers of the term (wave-uniform) marks the parameters with p_ti > 0 in
// a mask and packs their powers into scalar registers; then, per marked i in parameter order, d mono_t / d x_i is the product over the marked j IN THEIR ORDER of p d^(p - 1) (j = i) or d^p (else),
// each factor formed as the jacobian front end forms it, and is added as fma(tan_i, ., sum).  A parameter with p_ti = 0 is skipped, not added as 0 x: a
// NaN or Inf in a parameter, or in its tangent component, that only ever has power 0 never reaches the result; with K = ndim identity tangents the
// entry is fma(1, m_i, 0 + 0 x m_j ...) = the jacobian front end's m_i, bit for bit on finite inputs.
// LDS: the two operand buffers, x - center (ndim, 64) and the tangents (ndim, 64): 40 KB + 2 x ndim x 512 bytes, at most 72 KB -- two workgroups per CU.
struct TaylorJvpArgs {
    TaylorArgs G;           // a: x (B, ndim); R = B K rows of the result
    const double* tan;      // (B, K, ndim)
    int Kdir;               // K directions per point
};

__global__ __launch_bounds__(256, 2) void taylor_jvp_kernel(const TaylorJvpArgs P) {
    const TaylorArgs& A = P.G;
    extern __shared__ double ty_lds[];
    double* const abuf = ty_lds;                       // 2 x TY_KC x TY_RS
    double* const dl = ty_lds + 2 * TY_KC * TY_RS;     // (ndim, 64) x - center of the point of each row
    double* const tl = dl + A.ndim * TY_ROWS;          // (ndim, 64) the tangent of each row
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int nchunk = (A.K + TY_KC - 1) / TY_KC;
    const long long row0 = (long long)blockIdx.x * TY_ROWS;
    const int c0 = A.c0, cend = A.cend;
    const int col0 = c0 + (int)blockIdx.y * TY_COLS + wave * 64;
    const bool active = col0 < cend;      // (wave-uniform; an idle wave forms its share of the left operand and multiplies the last column: no branch round the MFMAs)
    // the tile's first point and the direction its first row stands for: row0 + t is point b0 + (k0 + t) / K
    const long long b0 = row0 / P.Kdir;
    const int kd0 = (int)(row0 - b0 * P.Kdir);
    for (int e = threadIdx.x; e < A.ndim * TY_ROWS; e += 256) {
        const int i = e >> 6;
        const long long row = row0 + (e & 63);
        const long long point = b0 + (kd0 + (e & 63)) / P.Kdir;
        const bool inside = row < A.R;      // rows past the end: finite, never stored
        dl[e] = inside ? A.a[point * A.ndim + i] - A.center[i] : 0.;
        tl[e] = inside ? P.tan[row * A.ndim + i] : 0.;
    }
    __syncthreads();
    ty_v4d acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = ty_v4d{0., 0., 0., 0.};
    int colj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        colj[j] = col < cend ? col : cend - 1;      // columns past the end of the range repeat its last one (never stored)
    }
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        double* const buf = abuf + (c & 1) * TY_KC * TY_RS;
        const int k0 = c * TY_KC;
        for (int tt = wave; tt < TY_KC; tt += 4) {      // a term per wave and step, a row per lane
            const int t = k0 + tt;
            double s = 0.;      // terms past T: zero columns of the left operand
            if (t < A.K) {
                const int* pw = A.powers + (long long)t * A.ndim;
                // one pass over the powers, four scalar loads in flight: bit i of marked for p_ti > 0 (ndim <= 32), the powers themselves (at most 15) in four
                // bits each of two scalar registers -- the loops below read no memory but the lanes' LDS
                unsigned marked = 0;
                unsigned long long plo = 0, phi = 0;
                for (int i0 = 0; i0 < A.ndim; i0 += 4) {
                    int p4[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) p4[k] = __builtin_amdgcn_readfirstlane(pw[i0 + k < A.ndim ? i0 + k : A.ndim - 1]);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int i = i0 + k;
                        int p = i < A.ndim ? p4[k] : 0;
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
        __syncthreads();      // one barrier per chunk: the buffer written next was last read before this barrier
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
                if (row < A.R) A.out[row * A.ldo + (col - c0)] = acc[i][j][r];
            }
    }
}

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

// The GEMM on the stream, inside the device scope of the entry point that calls it
template <int FRONT>
int taylor_launch(const char* who, const TaylorArgs& A, void* stream) {
    // the row tiles along x: workgroups are dispatched x first, so those in flight share their 256 columns of the right operand in L2
    const long long nrt = (A.R + TY_ROWS - 1) / TY_ROWS, nct = (A.cend - A.c0 + TY_COLS - 1) / TY_COLS;
    if (nrt > 0x7fffffffLL || nct > 65535) return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d results (at most 2^37 rows, 2^24 - 256 columns)", who, A.R, A.M);
    const dim3 grid((unsigned)nrt, (unsigned)nct);
    const size_t lds = (size_t)(2 * TY_KC * TY_RS + (FRONT != TY_FIT ? A.ndim * TY_ROWS : 0)) * sizeof(double);      // at most 56 KB
    hipLaunchKernelGGL(taylor_gemm_kernel<FRONT>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), A);
    return cp::launch_status(who);
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

int cp::taylor_predict_launch(const char* who, const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T,
                              const double* d_derivatives, int M, long long col0, long long ncols, double* d_out, long long ldo, void* stream) {
    const TaylorArgs A{d_x, d_center, d_powers, d_derivatives, d_out, B, ldo, T, M, ndim, (int)col0, (int)(col0 + ncols), 0};
    return taylor_launch<TY_PREDICT>(who, A, stream);
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
    return taylor_launch<TY_PREDICT>(who, A, stream);
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
    return taylor_launch<TY_JACOBIAN>(who, A, stream);
}

// One launch: taylor_jvp_kernel on the B K rows (b, k)
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
    const size_t lds = (size_t)(2 * TY_KC * TY_RS + 2 * ndim * TY_ROWS) * sizeof(double);      // at most 72 KB
    if (lds > 64 * 1024) {
        const hipError_t e = cp::allow_full_lds<taylor_jvp_kernel>();
        if (e != hipSuccess) return cp::launch_status(who, e);
    }
    hipLaunchKernelGGL(taylor_jvp_kernel, dim3((unsigned)nrt, (unsigned)nct), dim3(256), lds, static_cast<hipStream_t>(stream), A);
    return cp::launch_status(who);
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
    const int launched = taylor_launch<TY_FIT>(who, A, stream);
    if (launched != CP_OK) return launched;
    const long long R = B * ndim;
    hipLaunchKernelGGL(taylor_input_grad_kernel, dim3((unsigned)((R + TY_ROWS - 1) / TY_ROWS)), dim3(256), (size_t)(2 * TY_KC + ndim) * TY_ROWS * sizeof(double) + 2 * 4 * TY_ROWS * sizeof(unsigned), static_cast<hipStream_t>(stream), d_x, d_center,
                       d_powers, d_work, R, ndim, T, d_grad);
    return cp::launch_status(who);
}

extern "C" int cp_taylor_fit(const double* d_S, int T, int npoints, const double* d_Y, int M, double* d_derivatives, int device, void* stream) {
    if (T < 1 || npoints < 1 || M < 1) return cp::fail(CP_EINVAL, "cp_taylor_fit: need T, npoints, M >= 1");
    if (!d_S || !d_Y || !d_derivatives) return cp::fail(CP_EINVAL, "cp_taylor_fit: null pointer");
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_taylor_fit: cannot select device %d", device);
    const TaylorArgs A{d_S, nullptr, nullptr, d_Y, d_derivatives, T, M, npoints, M, 0, 0, M, npoints};
    return taylor_launch<TY_FIT>("cp_taylor_fit", A, stream);
}
