// cp_gauss_newton.h -- what cp_mlp_gauss_newton.hip and cp_taylor_gauss_newton.hip share: the Gram epilogue of their kernels and the host side behind the
// engines' fronts (cp_gauss_newton.hip).  Per point b over the columns c of a range, with J[b,i,c] the Jacobian of the prediction, w the weights and
// r = data - value:  fisher[b,i,j] = sum_c w J_i J_j,  grad[b,i] = sum_c w r J_i,  chi2[b] = sum_c w r^2.
// Tile.  The 64 x 256 tile of the tangent kernels (a wave 64 x 64 in 4 x 4 MFMA accumulator tiles; lane l holds D[row = 16 i + 4 r + (l >> 4)][col = 16 j +
// (l & 15)] in acc[i][j][r]) with ONE change of the rows: a row tile holds P = floor(64 / ndim) WHOLE points, row t = p ndim + i, and its last 64 - P ndim
// rows idle (finite inputs, never stored), so that every product J_i J_j of a point is formed inside one workgroup.
// Epilogue (gn_contract), per wave and per slab of 16 columns (one j), in the wave's own LDS, no workgroup barrier:
//   1. stage: a lane per (column, point) pair reads the weight, the value and the data once: W[c][p] = w, R[c][p] = data - value, D[c][p] = yscale f'(value)
//      (MLP; ln 10 value for 10^v, sqrt(1 + value^2) for sinh, as mlp_tangent_kernel forms it: J has the bits of cp_mlp_jacobian).  A weight of exactly 0,
//      and a column or a point past the end, gives W = R = D = 0;
//   2. the slab of J leaves the accumulators for LDS column-major, Jt[c][row] (row stride 68 doubles: the 16 columns x 4 row groups of a ds_write_b64 fall
//      on 2 x 32 distinct banks), as acc * D -- or exactly 0 where W is 0: a SELECT, since 0 x NaN is not 0, so a dropped column contributes exactly 0 to all
//      three sums whatever its data, value or derivative hold;
//   3. contract on the vector ALUs, lane = row t = (p, i): a = W[c][p] Jt[c][t], then f[j] += a Jt[c][p ndim + j] for j < ndim (one LDS read -- a
//      broadcast within the point -- and one FMA each), eight j at a time in registers over the slab's columns in order; g += a R[c][p], chi += (W R) R.
//      The row's sums live in the wave's LDS, F[k][lane] (a lane touches its own column only): eight accumulators in registers whatever ndim is (with
//      the whole row in registers the kernels spilled from ndim = 9 on).
// Only the triangle j <= i of f is used: the summing kernel mirrors it, so fisher[b] is symmetric bit for bit.  A row's sum runs over a slab's 16 columns
// in order, the wave's four slabs in order; gn_combine adds the four waves in wave order and stores the tile's partial sums, P x (ndim^2 + ndim + 1) doubles
// per (column tile, row tile) -- about 3 % of the Jacobian at ndim = 8 --; gn_sum_kernel (cp_gauss_newton.hip) adds the column tiles in tile order.
// No atomics anywhere: two calls give the same bits; and nothing of the residual enters f, so a call without data gives the fisher bits of one with.
// LDS per wave: 16 x 68 + 3 x 16 x P + (ndim + 2) x 64 doubles, 4 x that per workgroup: 67 KB at ndim = 8, under 80 KB (two workgroups per CU; the
// epilogue reuses the main loop's buffers) for 3 <= ndim <= 17, up to 108 KB at ndim = 32, 89 KB at ndim = 2 and 139 KB at ndim = 1 (one workgroup per CU).
#pragma once
#include "cp_internal.h"

namespace cpgn {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int GN_ROWS = 64, GN_COLS = 256, GN_SLAB = 16, GN_JS = 68;
enum { GN_Y_NONE = 0, GN_Y_EXP10 = 1, GN_Y_SINH = 2, GN_Y_PLAIN = 3 };      // the first three: CP_MLP_Y_*; plain: no yscale, no y function (Taylor)

// the operands of the epilogue; value is read where data is given or the y function needs it
struct Tail {
    const double* w;          // (B, ncols) with row stride ldw, or one row (ldw = 0)
    const double* data;       // the same with ldd, or null: Fisher matrix only
    const double* value;      // (B, ncols) with row stride ldv: the prediction on the range, written before the kernel runs (null if nobody reads it)
    double* part;             // (column tiles, B, S) partial sums, S = ndim^2 + ndim + 1: per point the rows of f (the triangle j <= i valid), g, chi
    long long ldw, ldd, ldv, B;
    int ndim, P;              // P = 64 / ndim points per row tile
    int c0, cend;
};

// what an entry point derives from (B, ndim, ncols): tiles and the workspace's layout, in doubles
struct Plan {
    int P;
    long long nrt, nct, S, value, part, total;      // value: (B, ncols) at this offset; part: (nct, B, S)
};

constexpr size_t epilogue_lds_doubles(int P, int ndim) { return (size_t)4 * (GN_SLAB * GN_JS + 3 * GN_SLAB * P + (ndim + 2) * GN_ROWS); }

// host side (cp_gauss_newton.hip)
int plan(const char* who, long long B, int ndim, long long ncols, Plan* plan);
int check_operands(const char* who, long long ncols, long long ldw, const double* d_data, long long ldd, const double* d_value, long long ldv);
int check_pointers(const char* who, const double* d_weights, const double* d_data, const double* d_fisher, const double* d_grad, const double* d_chi2,
                   const double* d_work, long long work_doubles, const Plan& plan, const char* sizer);
void sum_launch(cp::Launches& on, const Plan& plan, const Tail& tail, double* d_fisher, double* d_grad, double* d_chi2);
// cp_mlp_gauss_newton.hip: mlp_tangent_kernel in its Gauss-Newton variant for the y function, then the summing kernel -- the last two launches of
// cp_mlp_gauss_newton, for the entry points that contract a Jacobian with weights of their own (cp_mlp_vjp2); the value on the range is tail.value
void mlp_launch(cp::Launches& on, const double* d_x, const double* d_params, const double* d_xoffset, const double* d_xscale, const double* d_yscale,
                const cp::MlpLayout& net, int yfunction, const Plan& plan, const Tail& tail, double* d_fisher, double* d_grad, double* d_chi2);

#ifdef __HIPCC__
// the epilogue of one wave on its 64 x 64 accumulators: this lane's row of sums over the wave's columns colw .. colw + 63 into the wave's F[k][lane]
// (k < ndim: f; k = ndim: g; k = ndim + 1: chi), which only this lane touches until gn_combine
template <int YF>
__device__ __forceinline__ void gn_contract(const Tail& G, const double* yscale, const v4d (&acc)[4][4], double* wl, const int lane, const long long b0, const int colw) {
    const int n = G.ndim, P = G.P, l15 = lane & 15, g = lane >> 4;
    double* const Jt = wl;
    double* const Wt = wl + GN_SLAB * GN_JS;
    double* const Rt = Wt + GN_SLAB * P;
    double* const Dt = Rt + GN_SLAB * P;
    double* const F = Dt + GN_SLAB * P + lane;
    const int mine = lane / n < P ? lane / n : P - 1;      // this lane's point of the tile (an idle row: the last one, never stored)
    int pt[4][4];                                          // the points of the 16 rows this lane holds in the accumulators
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = (16 * i + 4 * r + g) / n;
            pt[i][r] = p < P ? p : P - 1;
        }
    for (int k = 0; k < n; ++k) F[k * GN_ROWS] = 0.;
    double gsum = 0., chi = 0.;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cs = colw + GN_SLAB * j;
        if (cs >= G.cend) break;      // (wave-uniform)
        for (int e = lane; e < GN_SLAB * P; e += 64) {
            const int c = e & 15, p = e >> 4;
            const int col = cs + c;
            const long long b = b0 + p;
            double wv = 0., rv = 0., dv = 0.;
            if (col < G.cend && b < G.B) wv = G.w[b * G.ldw + (col - G.c0)];
            if (wv != 0.) {      // (a NaN weight is kept: it reaches its point's sums)
                double y = 0.;
                if (G.data || YF == GN_Y_EXP10 || YF == GN_Y_SINH) y = G.value[b * G.ldv + (col - G.c0)];
                if (G.data) rv = G.data[b * G.ldd + (col - G.c0)] - y;
                if (YF != GN_Y_PLAIN) {
                    dv = yscale[col];
                    if (YF != GN_Y_NONE) dv *= YF == GN_Y_EXP10 ? 2.302585092994045684 * y : sqrt(fma(y, y, 1.));
                }
            }
            Wt[c * P + p] = wv, Rt[c * P + p] = rv, Dt[c * P + p] = dv;
        }
        cp::wave_lds_phase();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int at = l15 * P + pt[i][r];
                double jv = acc[i][j][r];
                if (YF != GN_Y_PLAIN) jv *= Dt[at];
                Jt[l15 * GN_JS + 16 * i + 4 * r + g] = Wt[at] == 0. ? 0. : jv;
            }
        cp::wave_lds_phase();
        const double* const other = Jt + mine * n;
#pragma unroll 1
        for (int k0 = 0; k0 < n; k0 += 8) {      // eight entries of the row at a time in registers, then into F
            int at[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) at[k] = k0 + k < n ? k0 + k : n - 1;      // (past ndim: the last one again, never stored)
            double t[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
#pragma unroll 2
            for (int c = 0; c < GN_SLAB; ++c) {
                const double a = Wt[c * P + mine] * Jt[c * GN_JS + lane];
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = fma(a, other[c * GN_JS + at[k]], t[k]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k0 + k < n) F[(k0 + k) * GN_ROWS] += t[k];
        }
        if (G.data) {
#pragma unroll 4
            for (int c = 0; c < GN_SLAB; ++c) {
                const double wv = Wt[c * P + mine], rv = Rt[c * P + mine];
                gsum = fma(wv * Jt[c * GN_JS + lane], rv, gsum);
                chi = fma(wv * rv, rv, chi);
            }
        }
        cp::wave_lds_phase();
    }
    F[n * GN_ROWS] = gsum, F[(n + 1) * GN_ROWS] = chi;
}

// The four waves' sums added in wave order, and the tile's partial sums stored: per point the ndim rows of f, g, chi.  Every wave of the workgroup comes here.
__device__ __forceinline__ void gn_combine(const Tail& G, const double* lds, const long long b0, const int ct) {
    const int n = G.ndim;
    const int region = (int)(epilogue_lds_doubles(G.P, n) / 4);
    const double* const F0 = lds + GN_SLAB * GN_JS + 3 * GN_SLAB * G.P;
    __syncthreads();
    const int S = n * n + n + 1;
    double* const out = G.part + ((long long)ct * G.B + b0) * S;      // the tile's points are contiguous
    for (int e = threadIdx.x; e < G.P * S; e += 256) {
        const int p = e / S, q = e - p * S;
        if (b0 + p >= G.B) break;
        int at;
        if (q < n * n) at = (q % n) * GN_ROWS + p * n + q / n;
        else if (q < n * n + n) at = n * GN_ROWS + p * n + (q - n * n);
        else at = (n + 1) * GN_ROWS + p * n;
        out[e] = ((F0[at] + F0[region + at]) + F0[2 * region + at]) + F0[3 * region + at];
    }
}
#endif

}  // namespace cpgn
