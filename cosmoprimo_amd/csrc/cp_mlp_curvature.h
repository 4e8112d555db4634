// cp_mlp_curvature.h -- the contracted second-order kernel of the MLP emulator (included by cp_mlp.hip: cp_mlp_vjp2), a __global__ of its own beside
// mlp_tangent2_kernel (cp_mlp_tangent2.h), whose hidden-layer recursion it repeats and whose instructions it leaves alone.
//   hess[b][i][j] = sum_c cot[b][c] d^2 predict[b][c] / d x[b][i] d x[b][j]        a row per (point, pair i <= j), both mirror entries written
// The output layer is linear and has no bias, so the contraction over the columns is done BEFORE the second-order pass: with the prediction y = f(v),
// v = yoffset + yscale n(x), n the network output and W_out its output kernel,
//   hess[b][i][j] = sum_k d2_ij[b][k] s[b][k]  +  sum_c omega[b][c] J[b][i][c] J[b][j][c]
//   s[b] = W_out[:, columns] . (cot yscale f'(v))     -- the dh of the last hidden layer that cp_mlp_vjp forms (forward kernel in its vjp mode, mlp_dh_kernel)
//   omega = cot f'' / f'^2                            -- y function only: cot / y for 10^v (0 where y = 0), cot y / (1 + y^2) for sinh (mlp_omega_kernel);
//                                                        the sum is a Gauss-Newton contraction with signed weights (cp_gauss_newton.h), added here
// and d2_ij[b] the second-order term of the last hidden layer along (e_i / xscale_i, e_j / xscale_j).
// The kernel.  64 rows per workgroup, row r = b npairs + p over the pairs i <= j in the order (0, 0), (0, 1), ..., (1, 1), ... (a point's rows may lie in
// two workgroups: every lane finds its own point and pair).  A lane carries h, du, dv and d2 of its row through the hidden layers on the vector ALUs as
// mlp_tangent2_kernel does -- the same operations in the same order, the product zu zv rounded on its own; on the diagonal dv is du bit for bit, which is
// that kernel's v = u form -- a workgroup of EIGHT waves on its 64 rows, a wave the neurons j = wave (mod 8), at most eight of them
// (h, du, dv, d2: 64 registers, where four waves with sixteen each spilled), the layer updated in place.  Then every lane sums its point's slices of dh in their order
// (as mlp_input_grad_kernel does) into the primal buffer, which nobody reads any more, and wave 0 takes sum_k d2[k] s[k] in ascending k, adds the
// y function's term where there is one and writes hess[b][i][j] and hess[b][j][i]: one writer per entry, symmetric bit for bit, no atomics.
// No MFMA, no output-layer operand: every buffer is read by the vector ALUs only (64 consecutive doubles per k), row stride 64.
// LDS: nr x 4 x 64 x 8 bytes, 64 KB at widths <= 32, 128 KB at widths up to 64; the launch helper opts in.  182 VGPRs: one workgroup (two waves per SIMD)
// per CU at every width (profiles/vjp2.txt).
#pragma once
#include "cp_mlp_tangent2.h"

namespace {

constexpr int ML_CW = 8;      // waves of mlp_curvature_kernel

struct MlpCurvArgs {
    const double* x;          // (B, ndim) raw parameters
    const double* params;
    const double* xoff;
    const double* xscale;
    const double* part;       // (nsl, B, H) the partial products of mlp_dh_kernel
    const double* add;        // y function: (B, ndim, ndim), symmetric bit for bit, added to the result; else null
    double* hess;             // (B, ndim, ndim)
    long long B, R;           // R = B npairs rows
    int npairs, nsl;
    cp::MlpLayout net;
};

// omega (B, ncols) = cot f'' / f'^2 from the cotangent and the value: the signed weights of the y function's term
template <int YF>
__global__ __launch_bounds__(256) void mlp_omega_kernel(const double* cot, const long long ldc, const double* value, const long long ldv, const long long B,
                                                        const long long ncols, double* omega) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= B * ncols) return;
    const long long b = e / ncols, c = e - b * ncols;
    const double q = cot[b * ldc + c], y = value[b * ldv + c];
    omega[e] = YF == CP_MLP_Y_EXP10 ? (y == 0. ? 0. : q / y) : q * y / fma(y, y, 1.);
}

__global__ __launch_bounds__(64 * ML_CW, 2) void mlp_curvature_kernel(const MlpCurvArgs A) {
    extern __shared__ double ml_lds[];
    const cp::MlpLayout& N = A.net;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * ML_ROWS + lane;
    const bool inside = row < A.R;
    // this lane's point and pair; rows past the end repeat the last one with zero inputs (finite, never stored)
    const long long rr = inside ? row : A.R - 1;
    const long long b = rr / A.npairs;
    int pi = 0, pj = (int)(rr - b * A.npairs);
    for (int n = N.ndim; pj >= n; --n) pj -= n, ++pi;      // parameter i holds the n = ndim - i pairs (i, i) .. (i, ndim - 1)
    pj += pi;
    double* const cur2 = ml_lds;                     // second-order terms, nr x ML_PS
    double* const curp = cur2 + N.nr * ML_PS;        // primal activations; at the end s
    double* const curu = curp + N.nr * ML_PS;        // tangents along e_i / xscale_i
    double* const curv = curu + N.nr * ML_PS;        // tangents along e_j / xscale_j
    for (int i = wave; i < N.ndim; i += ML_CW) {
        double v = 0., du = 0., dv = 0.;
        if (inside) {
            const double xs = A.xscale[i];
            v = (A.x[b * N.ndim + i] - A.xoff[i]) / xs;
            du = i == pi ? 1. / xs : 0.;
            dv = i == pj ? 1. / xs : 0.;
        }
        curp[i * ML_PS + lane] = v;
        curu[i * ML_PS + lane] = du;
        curv[i * ML_PS + lane] = dv;
        cur2[i * ML_PS + lane] = 0.;
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < N.L; ++l) {
        const int nin = N.d[l], nout = N.d[l + 1], act = N.act[l];
        const double* W = A.params + N.off[l];
        const double* bias = W + nin * nout;
        const double alpha = bias[nout], beta = bias[nout + 1];
        // the layer in place: a wave's neurons j = wave + 8 q (at most 8: two groups of four) stay in registers until every wave has read the inputs
        double hn[2][4], un[2][4], vn[2][4], sn[2][4];
#pragma unroll
        for (int grp = 0; grp < 2; ++grp) {
            const int j0 = wave + 4 * ML_CW * grp;
#pragma unroll
            for (int q = 0; q < 4; ++q) hn[grp][q] = un[grp][q] = vn[grp][q] = sn[grp][q] = 0.;
            if (j0 >= nout) continue;      // (wave-uniform)
            int jq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) jq[q] = j0 + ML_CW * q < nout ? j0 + ML_CW * q : j0;
            double accz[4] = {0., 0., 0., 0.}, accu[4] = {0., 0., 0., 0.}, accv[4] = {0., 0., 0., 0.}, acc2[4] = {0., 0., 0., 0.};
#pragma unroll 2
            for (int k = 0; k < nin; ++k) {
                const double hv = curp[k * ML_PS + lane], uv = curu[k * ML_PS + lane], vv = curv[k * ML_PS + lane], sv = cur2[k * ML_PS + lane];
                const double* wr = W + k * nout;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double w = wr[jq[q]];
                    accz[q] = fma(hv, w, accz[q]);
                    accu[q] = fma(uv, w, accu[q]);
                    accv[q] = fma(vv, w, accv[q]);
                    acc2[q] = fma(sv, w, acc2[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double d1, d2;
                activate_tangent2(act, accz[q] + bias[jq[q]], alpha, beta, hn[grp][q], d1, d2);
                un[grp][q] = d1 * accu[q];
                vn[grp][q] = d1 * accv[q];
                const double cross = accu[q] * accv[q];      // rounded on its own: symmetric in i and j
                sn[grp][q] = fma(d2, cross, d1 * acc2[q]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int grp = 0; grp < 2; ++grp)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = wave + 4 * ML_CW * grp + ML_CW * q;
                if (j < nout) {
                    curp[j * ML_PS + lane] = hn[grp][q];
                    curu[j * ML_PS + lane] = un[grp][q];
                    curv[j * ML_PS + lane] = vn[grp][q];
                    cur2[j * ML_PS + lane] = sn[grp][q];
                }
            }
        __syncthreads();
    }
    // s of this lane's point over the primal activations, which nobody reads any more: the slices of dh in their order
    const int H = N.d[N.L];
    for (int j = wave; j < H; j += ML_CW) {
        double s = 0.;
        for (int sl = 0; sl < A.nsl; ++sl) s += A.part[((long long)sl * A.B + b) * H + j];
        curp[j * ML_PS + lane] = s;
    }
    __syncthreads();
    if (wave != 0 || !inside) return;
    double c = 0.;
    for (int k = 0; k < H; ++k) c = fma(cur2[k * ML_PS + lane], curp[k * ML_PS + lane], c);
    double* const hb = A.hess + b * N.ndim * N.ndim;
    if (A.add) c += A.add[b * N.ndim * N.ndim + pi * N.ndim + pj];
    hb[pi * N.ndim + pj] = c;
    hb[pj * N.ndim + pi] = c;
}

}  // namespace
