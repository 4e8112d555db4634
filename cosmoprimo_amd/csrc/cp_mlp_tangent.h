// cp_mlp_tangent.h -- the forward-mode derivative kernel of the MLP emulator, written ONCE as a __global__ template for its three variants (included by
// cp_mlp.hip: cp_mlp_jacobian and cp_mlp_jvp; and by cp_mlp_gauss_newton.hip: cp_mlp_gauss_newton), with the device functions, strides and argument
// structs that go with it.  The variant is the type of the kernel's argument, so everything that differs between the variants is chosen at compile time:
//   MlpJacArgs  a row per (point, parameter) pair r = b ndim + i, the input tangent e_i / xscale[i]; stores the rows of the Jacobian
//   MlpJvpArgs  a row per (point, direction) pair r = b K + k, the input tangent tan[b][k][i] / xscale[i]; stores the rows of the product
//   MlpGnArgs   a row tile holds P = floor(64 / ndim) whole points, row t = p ndim + i; the tile of the Jacobian is contracted by the epilogue of
//               cp_gauss_newton.h and never stored
// Every kernel is held to its instructions (tools/compare_device_code.py).  Source is shared by writing one __global__ template whose variants differ under
// `if constexpr` only: a device function holding the shared body changed the instructions of its callers (register allocation), and copies of the body
// were three bodies to keep equal by hand.  DESIGN.md section 4 ('One source for the forward-mode derivative kernels') has the comparison.
//
// The kernel.  Forward mode through the network in the tile scheme of mlp_forward_kernel (64 rows x 256 columns per workgroup; 64 is no multiple of most
// ndim or K, so a point's rows may lie in two workgroups: every lane finds its own point).  A lane carries the primal activation h and the tangent dh of
// its row through the hidden layers on the vector ALUs: z = h W + b, dz = dh W, h = act(z), dh = act'(z) dz, from h_0 = (x - xoffset) / xscale and the
// variant's dh_0 (one FMA each per weight and LDS read).  The last tangent is multiplied by the output kernel on the matrix cores (no bias; operand fetch,
// masking and prefetch of the forward kernel), and the epilogue multiplies by yscale[c] f'(v), f' from the prediction that the forward kernel stored
// before this launch: ln 10 y for 10^v, sqrt(1 + y^2) for sinh.  With K = ndim identity tangents the jvp variant gives the bits of the jacobian variant,
// and the J that the Gauss-Newton variant contracts has them too.
// LDS.  ONE buffer of tangents, k-major with the row stride of 80 doubles (after the last layer it is the MFMA's left operand), and one of primal
// activations, which only the vector ALUs read (64 consecutive doubles per k), with a row stride of 64: a layer is updated IN PLACE -- a wave keeps its at
// most 16 neurons (h, dh) in registers (64, free until the MFMA accumulators are needed) until every wave has read the layer's inputs, one more barrier
// per layer.  nr x (80 + 64) x 8 bytes = 36 KB at widths <= 32 and 72 KB at widths up to 64: two workgroups per CU at every width, the registers' limit.
// (With two buffers each, 144 KB at widths up to 64, a CU held one workgroup and a row cost 1.8 x the forward kernel's: profiles/jacobian.txt.)  The
// Gauss-Newton epilogue reuses the buffers; where it needs more (cp_gauss_newton.h), the launch asks for that.
#pragma once
#include "cp_gauss_newton.h"
#include "cp_math.h"
#include <type_traits>

namespace {

typedef double ml_v4d __attribute__((ext_vector_type(4)));

constexpr int ML_ROWS = 64, ML_COLS = 256, ML_RS = 80, ML_MAX_NDIM = 32, ML_MAX_LAYERS = 8, ML_MAX_WIDTH = 64;
constexpr int ML_PS = 64;      // row stride of the primal buffer of the tangent kernel
enum { ACT_SILU = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_IDENTITY_SILU = 3 };

struct MlpNet : cp::MlpLayout {      // the layout (cp_internal.h: the one list of its fields) and the count of packed parameters
    long long total;
};
static_assert(sizeof(cp::MlpLayout::act) == ML_MAX_LAYERS * sizeof(int) && sizeof(cp::MlpLayout::d) == (ML_MAX_LAYERS + 2) * sizeof(int) &&
                  sizeof(cp::MlpLayout::off) == (ML_MAX_LAYERS + 1) * sizeof(long long),
              "cp::MlpLayout holds ML_MAX_LAYERS hidden layers");

struct MlpJacArgs {
    const double* x;          // (B, ndim) raw parameters
    const double* params;
    const double* xoff;
    const double* xscale;
    const double* yscale;
    const double* value;      // (B, ncols) with row stride ldv: the prediction on [c0, cend), written by the forward kernel before this one
    double* jac;              // (R, ncols) with row stride ldj, R = B ndim: row b ndim + i is point b, parameter i
    long long R, ldv, ldj;
    int c0, cend;
    MlpNet net;
};

struct MlpJvpArgs : MlpJacArgs {      // R = B K rows, jac the (B K, ncols) result
    const double* tan;        // (B, K, ndim), raw-parameter units
    int K;
};

struct MlpGnArgs {
    const double* x;          // (B, ndim) raw parameters
    const double* params;
    const double* xoff;
    const double* xscale;
    const double* yscale;
    cp::MlpLayout net;
    cpgn::Tail tail;
};

// The operands of the eight inner indices 8 p .. 8 p + 7 for one wave: two MFMA steps.  A row of the right operand past K is never read: its place in
// the left operand is 0, and 0 x NaN would not be (row 0 is fetched in its place and masked by mlp_mask).
__device__ __forceinline__ void mlp_load(const double* B, const int K, const int M, const double* buf, const int p, const int l15, const int g, const int (&colj)[4],
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
        for (int i = 0; i < 4; ++i) a[h][i] = buf[k * ML_RS + 16 * i + l15];
    }
}

__device__ __forceinline__ void mlp_mask(double (&b)[2][4], const bool (&keep)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int j = 0; j < 4; ++j) b[h][j] = keep[h] ? b[h][j] : 0.;
}

// act(z) and act'(z) of one pre-activation: the value as activate() forms it, the derivative as activate_derivative() does (cp_mlp.hip), with the
// exponential or tanh that they share taken once (written out: through the two functions the compiler took it twice, and the tangent kernel grew by half)
__device__ __forceinline__ void activate_tangent(int act, double v, double alpha, double beta, double& h, double& d) {
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

// YF: the y function, CP_MLP_Y_* (the same numbers as cpgn::GN_Y_*)
template <int YF, class Args>
__global__ __launch_bounds__(256, 2) void mlp_tangent_kernel(const Args A) {
    constexpr bool JVP = std::is_same<Args, MlpJvpArgs>::value, GN = std::is_same<Args, MlpGnArgs>::value;
    extern __shared__ double ml_lds[];
    const cp::MlpLayout& N = A.net;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    // jacobian, jvp: the tile's first row, its point and the parameter or direction it stands for: row0 + t is point b0 + (i0 + t) / nd.
    // Gauss-Newton: the tile's first point: row t is point b0 + t / ndim, parameter t % ndim
    long long row0 = 0, b0;
    int nd = 0, i0 = 0, c0, cend;
    if constexpr (GN) {
        b0 = (long long)blockIdx.x * A.tail.P;
        c0 = A.tail.c0, cend = A.tail.cend;
    } else {
        if constexpr (JVP) nd = A.K;
        else nd = N.ndim;
        row0 = (long long)blockIdx.x * ML_ROWS;
        b0 = row0 / nd;
        i0 = (int)(row0 - b0 * nd);
        c0 = A.c0, cend = A.cend;
    }
    const int col0 = c0 + (int)blockIdx.y * ML_COLS + wave * 64;
    double* const curt = ml_lds;                    // tangents, nr x ML_RS
    double* const curp = ml_lds + N.nr * ML_RS;     // primal activations, nr x ML_PS
    {      // the inputs of the tile's rows and their tangents, k-major; rows past the end, idle rows and points past the end: finite, never stored
        bool inside;
        long long b;
        int mine = 0;
        const double* tan = nullptr;
        if constexpr (GN) {
            const int p = lane / N.ndim;
            mine = lane - p * N.ndim;
            inside = p < A.tail.P && b0 + p < A.tail.B;
            b = b0 + p;
        } else {
            inside = row0 + lane < A.R;
            b = b0 + (i0 + lane) / nd;
            if constexpr (JVP) tan = A.tan + (row0 + lane) * N.ndim;      // row r = b K + k: tan[b][k] is row r of the (B K, ndim) array
            else mine = (i0 + lane) % nd;
        }
        for (int i = wave; i < N.ndim; i += 4) {
            double v = 0., t = 0.;
            if (inside) {
                const double xs = A.xscale[i];
                v = (A.x[b * N.ndim + i] - A.xoff[i]) / xs;
                if constexpr (JVP) t = tan[i] / xs;
                else t = i == mine ? 1. / xs : 0.;
            }
            curp[i * ML_PS + lane] = v;
            curt[i * ML_RS + lane] = t;
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
                const double hv = curp[k * ML_PS + lane], tv = curt[k * ML_RS + lane];
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
                activate_tangent(act, accz[q] + bias[jq[q]], alpha, beta, hn[grp][q], dval);
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
                    curp[j * ML_PS + lane] = hn[grp][q];
                    curt[j * ML_RS + lane] = tn[grp][q];
                }
            }
        for (int j = nout + wave; j < ((nout + 7) & ~7); j += 4) curt[j * ML_RS + lane] = 0.;      // the left operand's rows up to the next pair of MFMA steps
        __syncthreads();
    }
    // the output layer on the matrix cores: acc = dh_L . W_out[:, columns]
    const int K = N.d[N.L], M = N.M;
    const double* Wo = A.params + N.off[N.L];
    [[maybe_unused]] const bool active = col0 < cend;      // (wave-uniform; an idle wave multiplies the last column: no branch round the MFMAs)
    ml_v4d acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = ml_v4d{0., 0., 0., 0.};
    int colj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        colj[j] = col < cend ? col : cend - 1;      // columns past the end of the range repeat its last one (never stored; their weight is 0 in the Gauss-Newton epilogue)
    }
    {
        const int npairs = (K + 7) / 8;
        double a0[2][4], b0r[2][4];
        bool keep[2];
        mlp_load(Wo, K, M, curt, 0, l15, g, colj, a0, b0r, keep);
        mlp_mask(b0r, keep);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            mlp_load(Wo, K, M, curt, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1, keep);
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
    if constexpr (GN) {
        __syncthreads();      // every wave has read the last tangent: the epilogue takes the LDS over
        cpgn::gn_contract<YF>(A.tail, A.yscale, acc, ml_lds + wave * (cpgn::epilogue_lds_doubles(A.tail.P, N.ndim) / 4), lane, b0, col0);
        cpgn::gn_combine(A.tail, ml_lds, b0, (int)blockIdx.y);
    } else {
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
                    double d = ys;
                    if (YF != CP_MLP_Y_NONE) {
                        const double y = A.value[(b0 + (i0 + t) / nd) * A.ldv + (col - c0)];
                        d *= YF == CP_MLP_Y_EXP10 ? 2.302585092994045684 * y : sqrt(fma(y, y, 1.));
                    }
                    A.jac[(row0 + t) * A.ldj + (col - c0)] = acc[i][j][r] * d;
                }
        }
    }
}

// The kernel on the stream for the variant of A, inside the caller's device scope.  LDS: the hidden layers' buffers (36 KB at widths <= 32, at most 72 KB),
// or the Gauss-Newton epilogue's `epilogue` doubles where those are more.
template <int YF, class Args>
void mlp_tangent_launch(cp::Launches& on, const Args& A, const dim3 grid, const size_t epilogue) {
    const size_t hidden = (size_t)A.net.nr * (ML_RS + ML_PS);
    on.run<mlp_tangent_kernel<YF, Args>>(grid, 256, (hidden > epilogue ? hidden : epilogue) * sizeof(double), A);
}

}  // namespace
