// cp_mlp_tangent2.h -- the second-order forward-mode kernel of the MLP emulator (included by cp_mlp.hip: cp_mlp_jvp2), a __global__ of its own beside
// mlp_tangent_kernel (cp_mlp_tangent.h), whose tile scheme, operand fetch and constants it uses and whose instructions it leaves alone.
//   out[b K + k][c] = sum_ij u[b][k][i] v[b][k][j] d^2 predict[b][c] / d x[b][i] d x[b][j]        a row per (point, pair of directions)
// The kernel.  64 rows x 256 columns per workgroup, row r = b K + k (a point's rows may lie in two workgroups: every lane finds its own point).  A lane
// carries the primal activation h, the two tangents du, dv and the second-order term d2 of its row through the hidden layers on the vector ALUs:
//   z = h W + b, zu = du W, zv = dv W, z2 = d2 W;   h = act(z), du = act'(z) zu, dv = act'(z) zv, d2 = act''(z) (zu zv) + act'(z) z2
// from h_0 = (x - xoffset) / xscale, du_0 = u / xscale, dv_0 = v / xscale, d2_0 = 0 (four FMAs per weight).  The product zu zv is rounded before anything
// else touches it, so exchanging u and v gives the same bits.  The last d2 is multiplied by the output kernel on the matrix cores (no bias), and the
// epilogue applies the y function's chain rule with a = acc yscale[c], the value y and the first-order products y_u, y_v that the launches before this
// one stored (cp_mlp.hip: the forward kernel, then mlp_tangent_kernel's jvp variant once per tangent set):
//   none: a;   10^v: ln 10 y a + y_u y_v / y (0 where y = 0);   sinh: sqrt(1 + y^2) a + y (y_u y_v) / (1 + y^2)
// MIXED = false is v = u: the dv buffer and its FMAs are gone, zu zu in the place of zu zv, y_u y_u in the place of y_u y_v.
// LDS.  d2 k-major with the row stride of 80 doubles (after the last layer it is the MFMA's left operand); h, du, dv are read by the vector ALUs only
// (64 consecutive doubles per k), row stride 64.  A layer is updated in place as in mlp_tangent_kernel: a wave keeps its at most 16 neurons
// (h, du, dv, d2: 128 registers, free until the MFMA accumulators are needed) until every wave has read the layer's inputs.
// nr x (80 + 3 x 64) x 8 bytes: 70 KB at widths <= 32 (two workgroups per CU), 139 KB at widths up to 64 (one); v = u: 52 KB and 104 KB.
#pragma once
#include "cp_mlp_tangent.h"

namespace {

struct MlpJvp2Args {
    const double* x;          // (B, ndim) raw parameters
    const double* params;
    const double* xoff;
    const double* xscale;
    const double* yscale;
    const double* tan_u;      // (B, K, ndim), raw-parameter units
    const double* tan_v;      // MIXED: the second set
    const double* value;      // y function: (B, ncols) with row stride ldv, the prediction on [c0, cend)
    const double* first_u;    // y function: (R, ncols) with row stride ldf, the first-order products of cp_mlp_jvp along u ...
    const double* first_v;    // ... and along v (MIXED)
    double* out;              // (R, ncols) with row stride ldo
    long long R, ldv, ldf, ldo;      // R = B K rows
    int c0, cend, K;
    cp::MlpLayout net;
};

// act(z), act'(z) and act''(z) of one pre-activation, value and first derivative as activate_tangent forms them, the exponential or tanh taken once.
// relu: act'' is exactly 0, and a NaN stays one.
__device__ __forceinline__ void activate_tangent2(int act, double v, double alpha, double beta, double& h, double& d, double& d2) {
    switch (act) {
        case ACT_SILU: {
            const double e = 1. + cpmath::exp_mid(-v), s = 1. / e;
            h = v / e;
            d = s * (1. + v * (1. - s));
            d2 = (s * (1. - s)) * (2. + v * (1. - 2. * s));
            break;
        }
        case ACT_RELU:
            h = v > 0. ? v : (v != v ? v : 0.);
            d = v > 0. ? 1. : (v != v ? v : 0.);
            d2 = v != v ? v : 0.;
            break;
        case ACT_TANH: {
            const double t = tanh(v);
            h = t;
            d = 1. - t * t;
            d2 = -2. * t * d;
            break;
        }
        default: {
            const double av = alpha * v;
            const double e = 1. + cpmath::exp_mid(-av), s = 1. / e, s1 = s * (1. - s);
            h = ((1. - beta) + beta / e) * v;
            d = (1. - beta) + beta * (s + av * s1);
            d2 = (beta * alpha) * s1 * (2. + av * (1. - 2. * s));
        }
    }
}

// YF: the y function, CP_MLP_Y_*
template <int YF, bool MIXED>
__global__ __launch_bounds__(256, 2) void mlp_tangent2_kernel(const MlpJvp2Args A) {
    extern __shared__ double ml_lds[];
    const cp::MlpLayout& N = A.net;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    // the tile's first row, its point and direction: row0 + t is point b0 + (i0 + t) / K
    const int nd = A.K;
    const long long row0 = (long long)blockIdx.x * ML_ROWS, b0 = row0 / nd;
    const int i0 = (int)(row0 - b0 * nd);
    const int c0 = A.c0, cend = A.cend;
    const int col0 = c0 + (int)blockIdx.y * ML_COLS + wave * 64;
    double* const cur2 = ml_lds;                     // second-order terms, nr x ML_RS
    double* const curp = ml_lds + N.nr * ML_RS;      // primal activations, nr x ML_PS
    double* const curu = curp + N.nr * ML_PS;        // tangents along u
    double* const curv = curu + N.nr * ML_PS;        // tangents along v (MIXED; else outside the allocation and never touched)
    {      // the inputs of the tile's rows and their tangents, k-major; rows past the end: finite, never stored
        const bool inside = row0 + lane < A.R;
        const long long b = b0 + (i0 + lane) / nd;
        const double* tu = A.tan_u + (row0 + lane) * N.ndim;      // row r = b K + k: tan[b][k] is row r of the (B K, ndim) array
        [[maybe_unused]] const double* tv = nullptr;
        if constexpr (MIXED) tv = A.tan_v + (row0 + lane) * N.ndim;
        for (int i = wave; i < N.ndim; i += 4) {
            double v = 0., du = 0., dv = 0.;
            if (inside) {
                const double xs = A.xscale[i];
                v = (A.x[b * N.ndim + i] - A.xoff[i]) / xs;
                du = tu[i] / xs;
                if constexpr (MIXED) dv = tv[i] / xs;
            }
            curp[i * ML_PS + lane] = v;
            curu[i * ML_PS + lane] = du;
            if constexpr (MIXED) curv[i * ML_PS + lane] = dv;
            cur2[i * ML_RS + lane] = 0.;
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
        double hn[4][4], un[4][4], vn[4][4], sn[4][4];
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            const int j0 = wave + 16 * grp;
#pragma unroll
            for (int q = 0; q < 4; ++q) hn[grp][q] = un[grp][q] = vn[grp][q] = sn[grp][q] = 0.;
            if (j0 >= nout) continue;      // (wave-uniform)
            int jq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) jq[q] = j0 + 4 * q < nout ? j0 + 4 * q : j0;
            double accz[4] = {0., 0., 0., 0.}, accu[4] = {0., 0., 0., 0.}, accv[4] = {0., 0., 0., 0.}, acc2[4] = {0., 0., 0., 0.};
#pragma unroll 2
            for (int k = 0; k < nin; ++k) {
                const double hv = curp[k * ML_PS + lane], uv = curu[k * ML_PS + lane], sv = cur2[k * ML_RS + lane];
                [[maybe_unused]] double vv = 0.;
                if constexpr (MIXED) vv = curv[k * ML_PS + lane];
                const double* wr = W + k * nout;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double w = wr[jq[q]];
                    accz[q] = fma(hv, w, accz[q]);
                    accu[q] = fma(uv, w, accu[q]);
                    if constexpr (MIXED) accv[q] = fma(vv, w, accv[q]);
                    acc2[q] = fma(sv, w, acc2[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double d1, d2;
                activate_tangent2(act, accz[q] + bias[jq[q]], alpha, beta, hn[grp][q], d1, d2);
                un[grp][q] = d1 * accu[q];
                if constexpr (MIXED) vn[grp][q] = d1 * accv[q];
                const double cross = MIXED ? accu[q] * accv[q] : accu[q] * accu[q];      // rounded on its own: symmetric in u and v
                sn[grp][q] = fma(d2, cross, d1 * acc2[q]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int grp = 0; grp < 4; ++grp)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = wave + 16 * grp + 4 * q;
                if (j < nout) {
                    curp[j * ML_PS + lane] = hn[grp][q];
                    curu[j * ML_PS + lane] = un[grp][q];
                    if constexpr (MIXED) curv[j * ML_PS + lane] = vn[grp][q];
                    cur2[j * ML_RS + lane] = sn[grp][q];
                }
            }
        for (int j = nout + wave; j < ((nout + 7) & ~7); j += 4) cur2[j * ML_RS + lane] = 0.;      // the left operand's rows up to the next pair of MFMA steps
        __syncthreads();
    }
    // the output layer on the matrix cores: acc = d2_L . W_out[:, columns]
    const int K = N.d[N.L], M = N.M;
    const double* Wo = A.params + N.off[N.L];
    const bool active = col0 < cend;      // (wave-uniform; an idle wave multiplies the last column: no branch round the MFMAs)
    ml_v4d acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = ml_v4d{0., 0., 0., 0.};
    int colj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        colj[j] = col < cend ? col : cend - 1;      // columns past the end of the range repeat its last one (never stored)
    }
    {
        const int npairs = (K + 7) / 8;
        double a0[2][4], b0r[2][4];
        bool keep[2];
        mlp_load(Wo, K, M, cur2, 0, l15, g, colj, a0, b0r, keep);
        mlp_mask(b0r, keep);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            mlp_load(Wo, K, M, cur2, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1, keep);
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
            mlp_mask(b0r, keep);
        }
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        if (col >= cend) continue;
        const double ys = A.yscale[col];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int t = 16 * i + g + 4 * r;
                if (row0 + t >= A.R) continue;
                double res = acc[i][j][r] * ys;
                if (YF != CP_MLP_Y_NONE) {
                    const double y = A.value[(b0 + (i0 + t) / nd) * A.ldv + (col - c0)];
                    const double yu = A.first_u[(row0 + t) * A.ldf + (col - c0)];
                    double yv = yu;
                    if constexpr (MIXED) yv = A.first_v[(row0 + t) * A.ldf + (col - c0)];
                    const double cross = yu * yv;      // rounded on its own: symmetric in u and v
                    if (YF == CP_MLP_Y_EXP10) res = fma(2.302585092994045684 * y, res, y == 0. ? 0. : cross / y);
                    else res = fma(sqrt(fma(y, y, 1.)), res, y * cross / fma(y, y, 1.));
                }
                A.out[(row0 + t) * A.ldo + (col - c0)] = res;
            }
    }
}

// The kernel on the stream, inside the caller's device scope.  LDS: 70 KB at widths <= 32, at most 139 KB (v = u: 52 KB, 104 KB); the launch helper opts in.
template <int YF, bool MIXED>
void mlp_tangent2_launch(cp::Launches& on, const MlpJvp2Args& A, const dim3 grid) {
    on.run<mlp_tangent2_kernel<YF, MIXED>>(grid, 256, (size_t)A.net.nr * (ML_RS + (MIXED ? 3 : 2) * ML_PS) * sizeof(double), A);
}

}  // namespace
