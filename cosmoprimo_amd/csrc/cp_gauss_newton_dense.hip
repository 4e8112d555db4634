// cp_gauss_newton_dense.hip -- Fisher matrices and Gauss-Newton normal equations under a DENSE precision matrix, for batches of parameter points (gfx950)
// + C ABI, on an explicit Jacobian whatever produced it (cp_mlp_jacobian, cp_taylor_jacobian, a caller's own).  Per point b, with J_b (ndim, N) the
// Jacobian, r_b = data_b - value_b, A_b = [J_b ; r_b] (ndim + 1, N) and P (N, N) symmetric, shared by all points:  G_b = A_b P A_b^T,
//   fisher[b] = G_b[:ndim, :ndim],  grad[b] = G_b[:ndim, ndim],  chi2[b] = G_b[ndim, ndim].
// Launches.  dense_keep_kernel (the mask of the columns, once), dense_kernel, gn_sum_kernel (cp_gauss_newton.hip: the column tiles' partial sums added in
// tile order, the triangle mirrored).  Nothing is read back, nothing waits on the device, no atomics: two calls give the same bits.
// Tile.  One GEMM Y = A P on the matrix cores in the idiom of cp_taylor_gemm.h (v_mfma_f64_16x16x4_f64; a workgroup of four waves owns 64 rows x 256
// columns, a wave 64 x 64 in 4 x 4 accumulator tiles; lane l supplies A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15] and holds
// D[row = 16 i + 4 r + (l >> 4)][col = 16 j + (l & 15)] in acc[i][j][r]) with the rows of cp_gauss_newton.h for ndim + 1: a row tile holds
// PT = floor(64 / (ndim + 1)) WHOLE points, row t = p (ndim + 1) + i: i < ndim the rows of J, i = ndim the residual, formed as data - value while the tile
// is loaded (exactly 0 without data); the last 64 - PT (ndim + 1) rows idle (exactly 0, never stored).  The K loop runs over the N rows of P in chunks of 32:
// the chunk of A goes to LDS k-major (row stride 80 doubles: conflict-free ds_read_b64 of the fragments; two buffers, one barrier per chunk; a thread's entries of the next chunk are fetched under the MFMAs of this one), P is read
// straight from L1 / L2, 128 contiguous bytes per k (row tiles run along grid x: the workgroups in flight share their 256 columns of P in L2).
// Mask.  A column c with P[c][c] == 0 is dropped: its column of A is SELECTED to exactly 0 wherever it is loaded -- as the GEMM's left operand and in the
// epilogue -- so a NaN or Inf in the Jacobian, the value or the data at c reaches none of the sums.  P is taken as finite and symmetric and is read in
// full: row c of P meets the zeros of A, column c of Y the zeros of the epilogue.
// Epilogue, per wave and per half slab of 8 columns, in the wave's own LDS, no workgroup barrier: the 64 x 8 block of A at those columns is read again
// (At[c][row], row stride 68 doubles), the block of Y leaves the accumulators (Yt[c][row]; the 8 columns x 4 row groups of a write fall on distinct
// banks), and lane = row t = (p, i) adds f[k] += Yt[c][t] At[c][p (ndim + 1) + k] for k <= ndim over the 8 columns in order -- one LDS read (a broadcast
// within the point) and one FMA each, eight k at a time in registers, the row's sums in the wave's LDS F[k][lane].  Of the rows i < ndim the triangle
// k <= i is used (the summing kernel mirrors it: fisher[b] is symmetric bit for bit); row i = ndim holds grad (k < ndim) and chi2 (k = ndim).  Nothing of the
// residual row enters a row i < ndim, so a call without data gives the fisher bits of one with.  The four waves are added in wave order and the tile's
// partial sums stored in the layout of cp_gauss_newton.h, PT x (ndim^2 + ndim + 1) doubles per (column tile, row tile).
// LDS: 96 doubles of row table, then the larger of the GEMM's 2 x 32 x 80 doubles (40 KB) and the epilogue's 4 x (2 x 8 x 68 + (ndim + 1) x 64): 53 KB at
// ndim = 8 (two workgroups per CU up to ndim = 16), 101 KB at ndim = 32 (one).
#include "cp_gauss_newton.h"

namespace {

using cpgn::v4d;

constexpr int GD_ROWS = 64, GD_COLS = 256, GD_KC = 32, GD_RS = 80, GD_SLAB = 8, GD_JS = 68, GD_TABLE = 96, GD_MAX_NDIM = 32;

struct DenseArgs {
    const double* jac;        // row b ndim + i at stride ldj
    const double* value;      // (B, N) with row stride ldv (read where data is given)
    const double* data;       // (B, N) with row stride ldd, one row (ldd = 0), or null: Fisher matrix only
    const double* prec;       // (N, N) with row stride ldp
    const double* keep;       // (N) 1 or 0: the mask of the columns
    double* part;             // (column tiles, B, S) partial sums
    long long ldj, ldv, ldd, ldp, B;
    int ndim, P, N;           // P points per row tile
};

constexpr size_t dense_epilogue_doubles(int ndim) { return (size_t)4 * (2 * GD_SLAB * GD_JS + (ndim + 1) * GD_ROWS); }
constexpr size_t dense_lds_doubles(int ndim) {
    return GD_TABLE + (dense_epilogue_doubles(ndim) > (size_t)2 * GD_KC * GD_RS ? dense_epilogue_doubles(ndim) : (size_t)2 * GD_KC * GD_RS);
}

// keep[c] = 1 where the diagonal of P is not exactly 0 (a NaN there is kept: it reaches the sums)
__global__ __launch_bounds__(256) void dense_keep_kernel(const double* prec, const long long ldp, const int N, double* keep) {
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < N) keep[c] = prec[c * ldp + c] != 0. ? 1. : 0.;
}

// entry (row r of the tile, column k) of A: the row table says what the row is -- kind 0: idle (a point past the end, a residual without data), 1: a row of
// J that starts at jac + off, 2: the residual of point off
__device__ __forceinline__ double dense_entry(const DenseArgs& A, const long long* roff, const int* rkind, const int r, const int k) {
    const int kind = rkind[r];
    double v = 0.;
    if (kind != 0 && k < A.N) {      // the mask and the entry are fetched side by side, and the entry SELECTED: a dropped column may hold anything
        const double kept = A.keep[k];
        const long long off = roff[r];
        const double x = kind == 1 ? A.jac[off + k] : A.data[off * A.ldd + k] - A.value[off * A.ldv + k];
        v = kept != 0. ? x : 0.;
    }
    return v;
}

// the operands of the eight inner indices k0 + 8 p .. + 7 of one chunk for one wave: two MFMA steps.  A row of P past N is never read (row 0 in its place:
// its entries of A are exactly 0 in LDS)
__device__ __forceinline__ void dense_load(const DenseArgs& A, const double* buf, const int k0, const int p, const int l15, const int g, const int (&colj)[4],
                                           double (&a)[2][4], double (&b)[2][4]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int kk = 8 * p + 4 * h + g, k = k0 + kk;
        const double* br = A.prec + (long long)(k < A.N ? k : 0) * A.ldp;
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = br[colj[j]];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[h][i] = buf[kk * GD_RS + 16 * i + l15];
    }
}

__global__ __launch_bounds__(256, 2) void dense_kernel(const DenseArgs A) {
    extern __shared__ double gd_lds[];
    long long* const roff = reinterpret_cast<long long*>(gd_lds);      // 64
    int* const rkind = reinterpret_cast<int*>(gd_lds + GD_ROWS);        // 64
    double* const abuf = gd_lds + GD_TABLE;                             // 2 x GD_KC x GD_RS; the epilogue takes it over
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int n = A.ndim, n1 = n + 1, N = A.N;
    const long long b0 = (long long)blockIdx.x * A.P;
    const int colw = (int)blockIdx.y * GD_COLS + wave * 64;      // (an idle wave, colw >= N, forms its share of the left operand and multiplies the last column)
    if (threadIdx.x < GD_ROWS) {
        const int r = threadIdx.x, p = r / n1, i = r - p * n1;
        const long long b = b0 + p;
        const bool live = p < A.P && b < A.B;
        rkind[r] = !live ? 0 : i < n ? 1 : A.data ? 2 : 0;
        roff[r] = !live ? 0 : i < n ? (b * n + i) * A.ldj : b;
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
        const int col = colw + 16 * j + l15;
        colj[j] = col < N ? col : N - 1;      // columns past the end repeat the last one (their entries of A are 0 in the epilogue)
    }
    const int nchunk = (N + GD_KC - 1) / GD_KC;
    const int ek = threadIdx.x & 7, er = threadIdx.x >> 3;      // this thread's entries of a chunk: 8 consecutive k of a row per 8 lanes (64-byte reads)
    double ahead[8];      // this thread's entries of the next chunk, fetched under the MFMAs of this one
#pragma unroll
    for (int s = 0; s < 8; ++s) ahead[s] = dense_entry(A, roff, rkind, er + 32 * (s & 1), ek + 8 * (s >> 1));
#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
        double* const buf = abuf + (c & 1) * GD_KC * GD_RS;
        const int k0 = c * GD_KC;
#pragma unroll
        for (int s = 0; s < 8; ++s) buf[(ek + 8 * (s >> 1)) * GD_RS + er + 32 * (s & 1)] = ahead[s];
#pragma unroll
        for (int s = 0; s < 8; ++s) ahead[s] = dense_entry(A, roff, rkind, er + 32 * (s & 1), k0 + GD_KC + ek + 8 * (s >> 1));      // (past the last chunk: k >= N, zeros, no load)
        __syncthreads();      // one barrier per chunk: the buffer written next was last read before this barrier
        const int npairs = N - k0 >= GD_KC ? GD_KC / 8 : (N - k0 + 7) / 8;
        double a0[2][4], b0r[2][4];
        dense_load(A, buf, k0, 0, l15, g, colj, a0, b0r);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            dense_load(A, buf, k0, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1);
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
        }
    }
    __syncthreads();      // every wave has read the last chunk: the epilogue takes the buffers over

    const int region = (int)(dense_epilogue_doubles(n) / 4);
    double* const wl = abuf + wave * region;
    double* const Yt = wl;
    double* const At = wl + GD_SLAB * GD_JS;
    double* const F0 = At + GD_SLAB * GD_JS;
    double* const F = F0 + lane;
    const int mine = lane / n1 < A.P ? lane / n1 : A.P - 1;      // this lane's point of the tile (an idle row: the last one, never stored)
    const double* const other = At + mine * n1;
    for (int k = 0; k < n1; ++k) F[k * GD_ROWS] = 0.;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int cs = colw + 16 * j + GD_SLAB * h;
            if (cs >= N) continue;      // (wave-uniform)
#pragma unroll
            for (int s = 0; s < GD_SLAB; ++s) {
                const int e = lane + 64 * s, c = e & 7, r = e >> 3;
                At[c * GD_JS + r] = dense_entry(A, roff, rkind, r, cs + c);
            }
            if ((l15 >> 3) == h) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) Yt[(l15 & 7) * GD_JS + 16 * i + 4 * r + g] = acc[i][j][r];
            }
            cp::wave_lds_phase();
#pragma unroll 1
            for (int k0 = 0; k0 < n1; k0 += 8) {      // eight entries of the row at a time in registers, then into F
                int at[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) at[k] = k0 + k < n1 ? k0 + k : n1 - 1;      // (past ndim: the last one again, never stored)
                double t[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
#pragma unroll 2
                for (int c = 0; c < GD_SLAB; ++c) {
                    const double y = Yt[c * GD_JS + lane];
#pragma unroll
                    for (int k = 0; k < 8; ++k) t[k] = fma(y, other[c * GD_JS + at[k]], t[k]);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k0 + k < n1) F[(k0 + k) * GD_ROWS] += t[k];
            }
            cp::wave_lds_phase();
        }

    // the four waves' sums added in wave order, and the tile's partial sums stored: per point the ndim rows of f, g, chi
    __syncthreads();
    const int S = n * n + n + 1;
    const double* const Fw = abuf + 2 * GD_SLAB * GD_JS;
    double* const out = A.part + ((long long)blockIdx.y * A.B + b0) * S;      // the tile's points are contiguous
    for (int e = threadIdx.x; e < A.P * S; e += 256) {
        const int p = e / S, q = e - p * S;
        if (b0 + p >= A.B) break;
        int at;
        if (q < n * n) at = (q % n) * GD_ROWS + p * n1 + q / n;
        else if (q < n * n + n) at = (q - n * n) * GD_ROWS + p * n1 + n;
        else at = n * GD_ROWS + p * n1 + n;
        out[e] = ((Fw[at] + Fw[region + at]) + Fw[2 * region + at]) + Fw[3 * region + at];
    }
}

// what the entry points check first, in this order, and the tiles and the workspace (in doubles: the mask (ncols), then the partial sums (nct, B, S))
int dense_front(const char* who, long long B, int ndim, long long ncols, long long ldj, long long ldv, long long ldd, long long ldp, cpgn::Plan* plan) {
    if (B < 0 || ndim < 1 || ncols < 0) return cp::fail(CP_EINVAL, "%s: %lld points of %d parameters over %lld columns", who, B, ndim, ncols);
    if (ldj < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the Jacobian is less than its %lld columns", who, ldj, ncols);
    if (ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    if (ldd != 0 && ldd < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the data is neither 0 (one shared row) nor at least their %lld columns", who, ldd, ncols);
    if (ldp < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the precision matrix is less than its %lld columns", who, ldp, ncols);
    if (ndim > GD_MAX_NDIM) return cp::fail(CP_EUNSUPPORTED, "%s: %d parameters (at most %d)", who, ndim, GD_MAX_NDIM);
    const int P = GD_ROWS / (ndim + 1);
    const long long S = (long long)ndim * ndim + ndim + 1, nct = (ncols + GD_COLS - 1) / GD_COLS;
    // the grids: 2^31 - 1 row tiles of P points, column tiles along y, 2^31 - 1 workgroups of 256 entries in the summing kernel; with them the workspace
    // stays below 2^62 doubles
    if (B > 0x7fffffffLL * P || nct > 65535 || B > 0x7fffffffLL * 256 / S)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld points of %d parameters over %lld columns (at most 2^31 - 1 row tiles of %d points, 2^39 sums B (ndim^2 + ndim + 1), 2^24 - 256 columns)",
                        who, B, ndim, ncols, P);
    plan->P = P, plan->S = S, plan->nct = nct, plan->nrt = (B + P - 1) / P;
    plan->value = 0, plan->part = ncols, plan->total = plan->part + nct * B * S;
    return CP_OK;
}

}  // namespace

extern "C" long long cp_gauss_newton_dense_workspace_doubles(long long B, int ndim, long long ncols) {
    cpgn::Plan plan;
    const int status = dense_front("cp_gauss_newton_dense_workspace_doubles", B, ndim, ncols, ncols, ncols, 0, ncols, &plan);
    return status == CP_OK ? plan.total : -(long long)status;
}

extern "C" int cp_gauss_newton_dense(const double* d_jac, long long ldj, long long B, int ndim, long long ncols, const double* d_value, long long ldv,
                                     const double* d_data, long long ldd, const double* d_precision, long long ldp, double* d_fisher, double* d_grad,
                                     double* d_chi2, double* d_work, long long work_doubles, int device, void* stream) {
    const char* who = "cp_gauss_newton_dense";
    cpgn::Plan plan;
    int status = dense_front(who, B, ndim, ncols, ldj, d_value ? ldv : ncols, d_data ? ldd : 0, ldp, &plan);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    // without columns nothing but the results is touched: zeros
    if (ncols > 0 && (!d_jac || (d_data && !d_value))) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    status = cpgn::check_pointers(who, ncols > 0 ? d_precision : d_fisher, d_data, d_fisher, d_grad, d_chi2, ncols > 0 ? d_work : d_fisher, work_doubles, plan,
                                  "cp_gauss_newton_dense_workspace_doubles");
    if (status != CP_OK) return status;
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    cp::Launches on(who, stream);
    cpgn::Tail tail{};
    tail.part = ncols > 0 ? d_work + plan.part : nullptr, tail.B = B, tail.ndim = ndim;
    if (ncols > 0) {
        double* const keep = d_work + plan.value;
        on.run<dense_keep_kernel>((unsigned)((ncols + 255) / 256), 256, 0, d_precision, ldp, (int)ncols, keep);
        const DenseArgs A{d_jac, d_value, d_data, d_precision, keep, tail.part, ldj, ldv, ldd, ldp, B, ndim, plan.P, (int)ncols};
        on.run<dense_kernel>(dim3((unsigned)plan.nrt, (unsigned)plan.nct), 256, dense_lds_doubles(ndim) * sizeof(double), A);
    }
    cpgn::sum_launch(on, plan, tail, d_fisher, d_grad, d_chi2);      // (no column tile: zeros)
    return on.status();
}
