// cp_mlp.hip -- multi-layer perceptron emulator of a calculator (reference emulators/tools/mlp.py) for batches of parameter points (gfx950) + C ABI:
// the batched prediction in one launch, its derivative with respect to the parameters, the loss and its gradient for one training batch, and the Adam
// step (float64 throughout).
// Network.  ndim inputs, L <= 8 hidden layers of widths 1 .. 64, M outputs; a layer is v @ kernel + bias with kernel (n_in, n_out) row-major; a hidden
// layer is followed by silu, relu, tanh or identity-silu (two trained scalars alpha, beta per layer).  Parameters, gradients and Adam moments share ONE
// packed layout: per layer kernel, bias, and for a hidden layer alpha, beta (always there, so that the layout depends on the widths alone).
// Forward kernel (mlp_forward_kernel; predict and the forward pass of the training step).  The tile scheme of taylor_gemm_kernel (cp_taylor.hip): a
// workgroup of four waves owns 64 rows x 256 columns of the result, a wave 64 x 64 (4 x 4 accumulator tiles of 16 x 16, 128 registers).  Fragments of
// v_mfma_f64_16x16x4_f64: lane l supplies A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15] and holds D[row = (l >> 4) + 4 r][col = l & 15]
// in register r.  The hidden layers run on the vector ALUs with a row per lane, a wave taking the neurons j = wave (mod 4), four at a time (one LDS
// read of the activation per four FMAs, the weights wave-uniform); their activations live in two LDS buffers in turn, k-major h[k][row] with a row
// stride of 80 doubles -- the layout the MFMA's left operand is read from without bank conflicts (lanes l and l + 16 of a ds_read_b64 half on
// opposite halves of the bank row) -- and never reach memory in predict.  The last hidden activation is multiplied by the output kernel on the matrix
// cores, the right operand read straight from L1 / L2 (128 contiguous bytes per k), the operands of the next 32 MFMAs requested before this pair of
// steps; rows of the left operand between H_L and the next multiple of 8 are zero and the matching rows of the kernel are masked (0 x NaN).
// Every workgroup of a row tile forms the hidden layers again (sum of n_in n_out FMAs per row against 256 H_L per row on the matrix cores).
// Epilogue, predict: + bias, v * yscale + yoffset per column, then 10^v or sinh(v); training: the residual against Y, scaled by 2 / (b M), to the
// workspace and the sum of its squares per workgroup (fixed order).  Rows and columns past the end are never stored.
// LDS.  2 x NR x 80 x 8 bytes, NR = max(ndim, widths) rounded up to 8: 40 KB at widths <= 32 (launch bounds: two workgroups per CU, the registers'
// limit), 80 KB at widths up to 64 (two workgroups fill the 160 KB of a CU exactly).
// Jacobian (cp_mlp_jacobian: mlp_forward_kernel, then mlp_tangent_kernel).  Forward mode with a row per (point, parameter) pair in the same tile scheme; primal
// and tangent of the hidden layers in LDS, updated in place, NR x (80 + 64) x 8 bytes: 36 KB at widths <= 32, 72 KB at widths up to 64 -- two workgroups
// per CU at every width, the registers' limit (profiles/jacobian.txt).  The kernel and its details: cp_mlp_tangent.h.
// Gradient.  gW_out = h^T . r (mlp_gw_out_kernel) and dh = r . W_out^T (mlp_dh_kernel) on the matrix cores, both operands straight from memory: in the
// first both are contiguous along the 16 lanes of a k (and the column sums of r, the bias gradient, are taken from the fragments already loaded);
// in the second both are contiguous along k, a wave takes one slice of the M inner indices of a row tile and stores a partial result, summed in
// slice order by the kernel that applies the activation's derivative (slices of equal length, a multiple of 8 near M / min(ceil(1024 / row tiles),
// ceil(M / 64)), the last one shorter and its last MFMA step masked: mlp_work).  The hidden layers' products (at most 65 x 64 entries, sums over the batch)
// run on the vector ALUs: a thread per entry and one of 16 phases of the batch, combined in a fixed order.  No floating-point atomics anywhere: two
// calls give the same bits.
// Vector-Jacobian product (cp_mlp_vjp: G = cot . d predict / d x, reverse mode; three launches whatever the depth).  mlp_forward_kernel in its fourth
// group of modes stores the pre-activations as the training pass does and, in its epilogue, the weighted cotangent w = cot yscale f'(v) beside (or
// instead of) the prediction; mlp_dh_kernel multiplies w by the transposed columns of the output kernel; mlp_input_grad_kernel sums its slices and
// walks the hidden layers back in LDS.  No (B, ndim, .) array exists anywhere.  Details above the kernels.
// Jacobian-vector product (cp_mlp_jvp: out (B K, .) = tan . d predict / d x along K directions per point; mlp_forward_kernel, then mlp_tangent_kernel in its
// jvp variant).  The tangent kernel with a row per (point, direction) pair and the input tangent tan[b][k][i] / xscale[i]: the same LDS, registers and
// occupancy, and with K = ndim identity tangents the same bits.  No (B, ndim, .) array exists anywhere.
// Second directional derivative (cp_mlp_jvp2: out (B K, .) = u . d^2 predict / d x d x . v along K pairs of directions per point; mlp_forward_kernel, for a
// y function mlp_tangent_kernel's jvp variant once per tangent set, then mlp_tangent2_kernel of cp_mlp_tangent2.h, which carries h, du, dv and the
// second-order term through the hidden layers and reads the value and the first-order products in its epilogue).
// Contracted second derivative (cp_mlp_vjp2: hess (B, ndim, ndim) = sum_c cot d^2 predict / d x d x; the first two launches of cp_mlp_vjp, with a
// y function mlp_omega_kernel and the Gauss-Newton launches on its signed weights, then mlp_curvature_kernel of cp_mlp_curvature.h, a row per (point,
// pair i <= j): the output layer is contracted with the cotangent once per point, before the second-order pass).  No (B, ., ncols) array beyond vjp's.
// Host side.  cp_mlp_predict(_columns), cp_mlp_jacobian, cp_mlp_vjp, cp_mlp_jvp and cp_mlp_jvp2 are back ends of one front: mlp_front holds their common checks and fills the
// forward kernel's arguments, mlp_yfunction turns the y function into a template argument, mlp_dh_launch picks mlp_dh_kernel<NJ> (vjp and training step);
// an entry point adds its strides, grid cap, null pointers, workspace and ONE device scope, in that order.
// Every kernel is held to its instructions (tools/compare_device_code.py).  Where kernels share source -- the jacobian, jvp and Gauss-Newton variants of
// mlp_tangent_kernel -- they are ONE __global__ template whose variants are chosen at compile time (cp_mlp_tangent.h): a device function for the shared
// body changed its callers' instructions, and copies of the body had to be kept equal by hand.  The small device functions named above are the only others.
#include "cp_mlp_tangent.h"      // the tile's constants, MlpNet, mlp_load and mlp_mask, the tangent kernel and its launch
#include "cp_mlp_tangent2.h"     // the second-order kernel of cp_mlp_jvp2 and its launch
#include "cp_mlp_curvature.h"    // the contracted second-order kernel of cp_mlp_vjp2

namespace {

constexpr int ML_TRAIN = 3;      // mode of the forward kernel: 0 .. 2 predict with the y function CP_MLP_Y_*, 3 the training forward pass,
constexpr int ML_VJP = 4;        // 4 .. 6 the forward pass of the vector-Jacobian product with the y function CP_MLP_Y_* (mode - 4)
constexpr int ML_GS = 64;        // row stride of the LDS buffers of mlp_input_grad_kernel (the vector ALUs read them, a row per lane)

// workspace of cp_mlp_loss_grad, in doubles
struct MlpWork {
    long long z[ML_MAX_LAYERS], h[ML_MAX_LAYERS];   // (b, d[l + 1]) pre-activations and activations of hidden layer l
    long long resid, losspart, part, dz[2], ca, cb, total;
    int nrt, nct, nsl, ks;                          // row tiles, column tiles; slices of the M inner indices of mlp_dh_kernel and their length
};

struct MlpFwdArgs {
    const double* x;          // (R, ndim): raw parameters (predict), scaled ones (training)
    const double* params;
    const double* xoff;
    const double* xscale;
    const double* yoff;
    const double* yscale;
    const double* ytrue;      // training: (R, M)
    const double* cot;        // vjp: the cotangent (R, ncols) with row stride ldc
    double* out;              // predict: (R, ncols) with row stride ldo, the columns [c0, cend) of the (R, M) result; training: the scaled residual (R, M);
                              // vjp: the prediction as in predict, or null
    double* work;             // training, vjp
    long long R, ldo, ldc;
    int c0, cend;             // the column tiles start at c0 (any value: the fragments are fetched with 8-byte loads); nothing of the output layer, yoff or
                              // yscale outside [c0, cend) is read.  Training: [0, M), ldo = M
    double rscale;            // 2 / (R M)
    MlpNet net;
    MlpWork ws;
};

__device__ __forceinline__ double sigmoid(double v) { return 1. / (1. + cpmath::exp_mid(-v)); }

__device__ __forceinline__ double activate(int act, double v, double alpha, double beta) {
    switch (act) {
        case ACT_SILU: return v / (1. + cpmath::exp_mid(-v));
        case ACT_RELU: return v > 0. ? v : (v != v ? v : 0.);      // a NaN stays one
        case ACT_TANH: return tanh(v);
        default: return ((1. - beta) + beta / (1. + cpmath::exp_mid(-alpha * v))) * v;
    }
}

template <int MODE>
__global__ __launch_bounds__(256, 2) void mlp_forward_kernel(const MlpFwdArgs A) {
    constexpr bool VJP = MODE >= ML_VJP;
    constexpr int YF = VJP ? MODE - ML_VJP : MODE;      // the y function (predict, vjp)
    extern __shared__ double ml_lds[];
    const MlpNet& N = A.net;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * ML_ROWS;
    // the range of columns and the row stride of the result; the training pass takes every column, known at compile time (its code is what it was)
    const int c0 = MODE == ML_TRAIN ? 0 : A.c0, cend = MODE == ML_TRAIN ? A.net.M : A.cend;
    const long long ldo = MODE == ML_TRAIN ? (long long)A.net.M : A.ldo;
    const int col0 = c0 + (int)blockIdx.y * ML_COLS + wave * 64;
    double* cur = ml_lds;
    double* nxt = ml_lds + N.nr * ML_RS;
    {      // the inputs of the tile's rows, k-major; rows past the end: finite, never stored
        const long long row = row0 + lane;
        for (int i = wave; i < N.ndim; i += 4) {
            double v = 0.;
            if (row < A.R) {
                v = A.x[row * N.ndim + i];
                if (MODE != ML_TRAIN) v = (v - A.xoff[i]) / A.xscale[i];
            }
            cur[i * ML_RS + lane] = v;
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int l = 0; l < N.L; ++l) {
        const int nin = N.d[l], nout = N.d[l + 1], act = N.act[l];
        const double* W = A.params + N.off[l];
        const double* bias = W + nin * nout;
        const double alpha = bias[nout], beta = bias[nout + 1];
        const bool record = (MODE == ML_TRAIN || VJP) && blockIdx.y == 0 && row0 + lane < A.R;
#pragma unroll 1
        for (int j0 = wave; j0 < nout; j0 += 16) {
            int jq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) jq[q] = j0 + 4 * q < nout ? j0 + 4 * q : j0;
            double acc[4] = {0., 0., 0., 0.};
#pragma unroll 2
            for (int k = 0; k < nin; ++k) {
                const double hv = cur[k * ML_RS + lane];
                const double* wr = W + k * nout;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fma(hv, wr[jq[q]], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = j0 + 4 * q;
                if (j >= nout) break;
                const double z = acc[q] + bias[j];
                const double hval = activate(act, z, alpha, beta);
                nxt[j * ML_RS + lane] = hval;
                if (record) {
                    const long long e = (row0 + lane) * nout + j;
                    A.work[A.ws.z[l] + e] = z;
                    if (!VJP) A.work[A.ws.h[l] + e] = hval;
                }
            }
        }
        for (int j = nout + wave; j < ((nout + 7) & ~7); j += 4) nxt[j * ML_RS + lane] = 0.;      // the left operand's rows up to the next pair of MFMA steps
        __syncthreads();
        double* const t = cur;
        cur = nxt;
        nxt = t;
    }
    // the output layer on the matrix cores
    const int K = N.d[N.L], M = N.M;
    const double* Wo = A.params + N.off[N.L];
    const double* bo = Wo + (long long)K * M;
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
        double a0[2][4], b0[2][4];
        bool keep[2];
        mlp_load(Wo, K, M, cur, 0, l15, g, colj, a0, b0, keep);
        mlp_mask(b0, keep);
#pragma unroll 1
        for (int p = 0; p < npairs; ++p) {
            double a1[2][4], b1[2][4];
            mlp_load(Wo, K, M, cur, p + 1 < npairs ? p + 1 : p, l15, g, colj, a1, b1, keep);
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
            mlp_mask(b0, keep);
        }
    }
    double sq = 0.;      // training: this thread's share of sum (y_pred - y_true)^2
    if (active) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = col0 + 16 * j + l15;
            if (col >= cend) continue;
            const double bj = bo[col];
            double ys = 1., yo = 0.;
            if (MODE != ML_TRAIN) ys = A.yscale[col], yo = A.yoff[col];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long long row = row0 + 16 * i + g + 4 * r;
                    if (row >= A.R) continue;
                    double v = acc[i][j][r] + bj;
                    if (MODE == ML_TRAIN) {
                        v -= A.ytrue[row * M + col];
                        sq = fma(v, v, sq);
                        v *= A.rscale;
                    } else {
                        v = fma(v, ys, yo);
                        if (YF == CP_MLP_Y_EXP10) v = cpmath::exp10_mid(v);
                        if (YF == CP_MLP_Y_SINH) v = sinh(v);
                    }
                    if (VJP) {      // the weighted cotangent, f' from the prediction as mlp_tangent_kernel forms it
                        double d = ys;
                        if (YF != CP_MLP_Y_NONE) d *= YF == CP_MLP_Y_EXP10 ? 2.302585092994045684 * v : sqrt(fma(v, v, 1.));
                        A.work[A.ws.resid + row * (long long)(cend - c0) + (col - c0)] = A.cot[row * A.ldc + (col - c0)] * d;
                        if (!A.out) continue;
                    }
                    A.out[row * ldo + (col - c0)] = v;
                }
        }
    }
    if (MODE == ML_TRAIN) {      // the workgroup's sum in thread order
        __syncthreads();
        ml_lds[threadIdx.x] = sq;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.;
            for (int t = 0; t < 256; ++t) s += ml_lds[t];
            A.work[A.ws.losspart + (long long)blockIdx.y * gridDim.x + blockIdx.x] = s;
        }
    }
}

// act'(z) of one pre-activation, the formulas of mlp_dz_kernel and of activate_tangent (relu: 0 at z <= 0, and a NaN stays one as in activate_tangent;
// the training step's kernel keeps its own copy with the terms its alpha and beta gradients share, and its bits)
__device__ __forceinline__ double activate_derivative(int act, double v, double alpha, double beta) {
    switch (act) {
        case ACT_SILU: {
            const double s = sigmoid(v);
            return s * (1. + v * (1. - s));
        }
        case ACT_RELU: return v > 0. ? 1. : (v != v ? v : 0.);
        case ACT_TANH: {
            const double t = tanh(v);
            return 1. - t * t;
        }
        default: {
            const double s = sigmoid(alpha * v);
            return (1. - beta) + beta * (s + alpha * v * (s * (1. - s)));
        }
    }
}

// dst[0] = scale * sum src[0 .. n): one workgroup of 1024 threads, a thread the entries t, t + 1024, ... in order, then the threads in order
__global__ __launch_bounds__(1024) void mlp_sum_kernel(const double* src, long long n, double scale, double* dst) {
    __shared__ double part[1024];
    double s = 0.;
    for (long long e = threadIdx.x; e < n; e += 1024) s += src[e];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) dst[0] = scale * part[0];
}

// gW_out (H, M) = h^T (H, b) . r (b, M) and gb_out = column sums of r.  A workgroup owns 256 columns, a wave 64 of them and all H <= 16 NI rows; the
// inner index is the sample.  Both operands come straight from memory, contiguous along the 16 lanes of a k.
template <int NI>
__global__ __launch_bounds__(256, 2) void mlp_gw_out_kernel(const double* h, const double* r, const long long b, const int H, const int M, double* gW) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int col0 = (int)blockIdx.x * ML_COLS + wave * 64;
    if (col0 >= M) return;      // (no barrier in this kernel)
    int colj[4], rowi[NI];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = col0 + 16 * j + l15;
        colj[j] = col < M ? col : M - 1;
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) rowi[i] = 16 * i + l15 < H ? 16 * i + l15 : H - 1;
    ml_v4d acc[NI][4];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = ml_v4d{0., 0., 0., 0.};
    double cs[4] = {0., 0., 0., 0.};
    const long long nsteps = (b + 3) / 4;
#pragma unroll 1
    for (long long s = 0; s < nsteps; ++s) {
        const long long k = 4 * s + g;
        const bool inside = k < b;
        const double* hr = h + (inside ? k : 0) * H;
        const double* rr = r + (inside ? k : 0) * M;
        double a[NI], bb[4];
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i] = hr[rowi[i]];
#pragma unroll
        for (int j = 0; j < 4; ++j) bb[j] = rr[colj[j]];
#pragma unroll
        for (int i = 0; i < NI; ++i) a[i] = inside ? a[i] : 0.;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bb[j] = inside ? bb[j] : 0.;
            cs[j] += bb[j];
        }
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // the four lane groups of a column, in a fixed order
        cs[j] += __shfl_xor(cs[j], 16);
        cs[j] += __shfl_xor(cs[j], 32);
        const int col = col0 + 16 * j + l15;
        if (col >= M) continue;
        if (g == 0) gW[(long long)H * M + col] = cs[j];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int row = 16 * i + g + 4 * q;
                if (row < H) gW[(long long)row * M + col] = acc[i][j][q];
            }
    }
}

// partial dh (slice, b, H) = r (b, M) . W_out^T (M, H) over one slice of the M inner indices per wave; both operands contiguous along k, with row
// strides ldr and ldw (the training step: both M; the vjp: M inner indices starting at a column of the output kernel, ldw its full width).
template <int NJ>
__global__ __launch_bounds__(256, 2) void mlp_dh_kernel(const double* r, const long long ldr, const double* W, const long long ldw, const long long b, const int H,
                                                        const int M, const int nsl, const int ks, double* part) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int l15 = lane & 15, g = lane >> 4;
    const int sl = (int)blockIdx.y * 4 + wave;
    if (sl >= nsl) return;      // (no barrier in this kernel)
    const long long row0 = (long long)blockIdx.x * ML_ROWS;
    const int kbeg = sl * ks, kend = kbeg + ks < M ? kbeg + ks : M;
    const double* ar[4];
    const double* br[NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long row = row0 + 16 * i + l15;
        ar[i] = r + (row < b ? row : b - 1) * ldr;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) br[j] = W + (long long)(16 * j + l15 < H ? 16 * j + l15 : H - 1) * ldw;
    ml_v4d acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = ml_v4d{0., 0., 0., 0.};
#pragma unroll 1
    for (int k0 = kbeg; k0 < kend; k0 += 4) {
        const int k = k0 + g;
        const bool inside = k < kend;
        const int kk = inside ? k : kbeg;
        double a[4], bb[NJ];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = ar[i][kk];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bb[j] = br[j][kk];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = inside ? a[i] : 0.;
#pragma unroll
        for (int j = 0; j < NJ; ++j) bb[j] = inside ? bb[j] : 0.;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
    double* out = part + (long long)sl * b * H;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = 16 * j + l15;
        if (col >= H) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long row = row0 + 16 * i + g + 4 * q;
                if (row < b) out[row * H + col] = acc[i][j][q];
            }
    }
}

// dz_l (b, H) = dh_l * act'(z_l) for hidden layer l, a thread per entry.  dh_l: the sum of the nsl partial products of mlp_dh_kernel in slice order (the
// last hidden layer), else dz_{l+1} . W_{l+1}^T.  identity-silu: the entries' contributions to the gradients of alpha and beta to ca, cb.
__global__ __launch_bounds__(256) void mlp_dz_kernel(const double* part, const int nsl, const double* dznext, const double* Wnext, const int Hn, const double* z,
                                                     const long long b, const int H, const int act, const double* ab, double* dz, double* ca, double* cb) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= b * H) return;
    double dh = 0.;
    if (part) {
        for (int s = 0; s < nsl; ++s) dh += part[(long long)s * b * H + e];
    } else {
        const long long row = e / H;
        const int i = (int)(e % H);
        for (int j = 0; j < Hn; ++j) dh = fma(dznext[row * Hn + j], Wnext[i * Hn + j], dh);
    }
    const double v = z[e];
    double d;
    switch (act) {
        case ACT_SILU: {
            const double s = sigmoid(v);
            d = s * (1. + v * (1. - s));
            break;
        }
        case ACT_RELU: d = v > 0. ? 1. : 0.; break;
        case ACT_TANH: {
            const double t = tanh(v);
            d = 1. - t * t;
            break;
        }
        default: {
            const double alpha = ab[0], beta = ab[1];
            const double s = sigmoid(alpha * v), s1 = s * (1. - s);
            d = (1. - beta) + beta * (s + alpha * v * s1);
            ca[e] = dh * (beta * s1 * v * v);
            cb[e] = dh * ((s - 1.) * v);
        }
    }
    dz[e] = dh * d;
}

// Input-gradient kernel (cp_mlp_vjp): the walk back through the hidden layers for 64 points per workgroup, a row per lane, in two LDS buffers in turn,
// k-major g[k][row] with a row stride of 64 doubles (only the vector ALUs read them).  dh of the last hidden layer is the sum of the nsl partial
// products of mlp_dh_kernel in slice order; per layer dz = dh act'(z_l) (z_l from the workspace, a wave the neurons j = wave (mod 4)), then
// dh_{l-1} = dz . W_l^T with a wave taking the inputs i = wave (mod 4), four at a time (one LDS read of dz per four FMAs, the weights wave-uniform and
// contiguous along the sum), summed over j in order; at the end G[b][i] = dh_0[i] / xscale[i].  Nothing but G is stored, no atomics: two calls give the
// same bits.  LDS: 2 x nr x 64 x 8 bytes, at most 64 KB.
struct MlpGradArgs {
    const double* params;
    const double* xscale;
    const double* work;       // z_l and the partial products, at the offsets of ws
    double* grad;             // (B, ndim)
    long long B;
    MlpNet net;
    MlpWork ws;
};

__global__ __launch_bounds__(256, 2) void mlp_input_grad_kernel(const MlpGradArgs A) {
    extern __shared__ double ml_lds[];
    const MlpNet& N = A.net;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const long long row0 = (long long)blockIdx.x * ML_ROWS;
    const long long row = row0 + lane < A.B ? row0 + lane : A.B - 1;      // rows past the end repeat the last one (never stored)
    double* cur = ml_lds;
    double* nxt = ml_lds + N.nr * ML_GS;
    {
        const int H = N.d[N.L];
        const double* part = A.work + A.ws.part;
        for (int j = wave; j < H; j += 4) {
            double dh = 0.;
            for (int s = 0; s < A.ws.nsl; ++s) dh += part[((long long)s * A.B + row) * H + j];
            cur[j * ML_GS + lane] = dh;
        }
    }
#pragma unroll 1
    for (int l = N.L - 1; l >= 0; --l) {
        const int nin = N.d[l], nout = N.d[l + 1], act = N.act[l];
        const double* W = A.params + N.off[l];
        const double alpha = W[(nin + 1) * nout], beta = W[(nin + 1) * nout + 1];
        const double* z = A.work + A.ws.z[l] + row * nout;
        for (int j = wave; j < nout; j += 4) cur[j * ML_GS + lane] *= activate_derivative(act, z[j], alpha, beta);      // (an entry is its own thread's)
        __syncthreads();
#pragma unroll 1
        for (int i0 = wave; i0 < nin; i0 += 16) {
            const double* wr[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) wr[q] = W + (i0 + 4 * q < nin ? i0 + 4 * q : i0) * nout;
            double acc[4] = {0., 0., 0., 0.};
#pragma unroll 2
            for (int j = 0; j < nout; ++j) {
                const double dz = cur[j * ML_GS + lane];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fma(dz, wr[q][j], acc[q]);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (i0 + 4 * q < nin) nxt[(i0 + 4 * q) * ML_GS + lane] = acc[q];
        }
        __syncthreads();
        double* const t = cur;
        cur = nxt;
        nxt = t;
    }
    for (int e = threadIdx.x; e < ML_ROWS * N.ndim; e += 256) {      // the tile's (64, ndim) block of G is contiguous
        const int r = e / N.ndim, i = e - r * N.ndim;
        if (row0 + r < A.B) A.grad[row0 * N.ndim + e] = cur[i * ML_GS + r] / A.xscale[i];
    }
}

// gradient of hidden layer l: gW (nin, nout) = hprev^T . dz, gb (nout) = column sums of dz -- (nin + 1, nout) entries contiguous in the packed
// layout -- a thread per entry and one of 16 phases of the batch (64 entries x 16 phases per workgroup), the phases combined in order.  clear_ab: the
// layer has no alpha, beta to train (not identity-silu); their two gradients, which follow the bias's, are set to 0 here.
__global__ __launch_bounds__(1024) void mlp_gw_hidden_kernel(const double* hprev, const double* dz, const long long b, const int nin, const int nout, double* g,
                                                             const bool clear_ab) {
    __shared__ double part[16][64];
    const int t = threadIdx.x & 63, phase = threadIdx.x >> 6;
    const int e = (int)blockIdx.x * 64 + t;
    double s = 0.;
    if (e < (nin + 1) * nout) {
        const int i = e / nout, j = e % nout;
        if (i < nin) {
            for (long long r = phase; r < b; r += 16) s = fma(hprev[r * nin + i], dz[r * nout + j], s);
        } else {
            for (long long r = phase; r < b; r += 16) s += dz[r * nout + j];
        }
    }
    part[phase][t] = s;
    __syncthreads();
    if (phase == 0 && e < (nin + 1) * nout) {
        double total = 0.;
        for (int p = 0; p < 16; ++p) total += part[p][t];
        g[e] = total;
    }
    if (clear_ab && blockIdx.x == 0 && threadIdx.x < 2) g[(nin + 1) * nout + threadIdx.x] = 0.;
}

__global__ __launch_bounds__(256) void mlp_adam_kernel(double* p, double* m, double* v, const double* g, const long long n, const double lr, const double b1,
                                                       const double b2, const double eps, const double c1, const double c2) {
#pragma clang fp contract(off)      // the formula as written, every operation rounded once
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const double ge = g[e];
    const double me = b1 * m[e] + (1. - b1) * ge;
    const double ve = b2 * v[e] + (1. - b2) * (ge * ge);
    m[e] = me;
    v[e] = ve;
    p[e] -= lr * (me / c1) / (sqrt(ve / c2) + eps);
}

int mlp_net(const char* who, int ndim, int nlayers, const int* widths, const int* activations, int M, MlpNet* net) {
    if (ndim < 1 || nlayers < 1 || M < 1 || !widths) return cp::fail(CP_EINVAL, "%s: need ndim, M >= 1, at least one hidden layer and its widths", who);
    if (ndim > ML_MAX_NDIM) return cp::fail(CP_EUNSUPPORTED, "%s: %d parameters (at most %d)", who, ndim, ML_MAX_NDIM);
    if (nlayers > ML_MAX_LAYERS) return cp::fail(CP_EUNSUPPORTED, "%s: %d hidden layers (at most %d)", who, nlayers, ML_MAX_LAYERS);
    net->ndim = ndim, net->L = nlayers, net->M = M;
    net->d[0] = ndim;
    int widest = ndim;
    for (int l = 0; l < nlayers; ++l) {
        if (widths[l] < 1) return cp::fail(CP_EINVAL, "%s: hidden layer %d has width %d", who, l, widths[l]);
        if (widths[l] > ML_MAX_WIDTH) return cp::fail(CP_EUNSUPPORTED, "%s: hidden layer %d has width %d (at most %d)", who, l, widths[l], ML_MAX_WIDTH);
        if (activations && (activations[l] < ACT_SILU || activations[l] > ACT_IDENTITY_SILU))
            return cp::fail(CP_EINVAL, "%s: activation code %d of hidden layer %d (0 silu, 1 relu, 2 tanh, 3 identity-silu)", who, activations[l], l);
        net->d[l + 1] = widths[l];
        net->act[l] = activations ? activations[l] : 0;
        widest = widths[l] > widest ? widths[l] : widest;
    }
    net->d[nlayers + 1] = M;
    net->nr = (widest + 7) & ~7;
    long long off = 0;
    for (int l = 0; l <= nlayers; ++l) {
        net->off[l] = off;
        off += ((long long)net->d[l] + 1) * net->d[l + 1] + (l < nlayers ? 2 : 0);
    }
    net->total = off;
    return CP_OK;
}

// nsl slices of length ks of the M inner indices of mlp_dh_kernel for nrt row tiles (the rule is above its use in mlp_work)
void mlp_slices(long long nrt, int M, MlpWork* ws) {
    long long nsl = nrt > 0 ? (1024 + nrt - 1) / nrt : 1;
    const long long most = (M + 63) / 64;
    nsl = nsl > most ? most : nsl;
    ws->ks = (int)((((M + nsl - 1) / nsl) + 7) & ~7LL);
    ws->nsl = (M + ws->ks - 1) / ws->ks;
}

void mlp_work(const MlpNet& net, long long b, MlpWork* ws) {
    long long off = 0, hmax = 0;
    for (int l = 0; l < net.L; ++l) {
        ws->z[l] = off, off += b * net.d[l + 1];
        ws->h[l] = off, off += b * net.d[l + 1];
        hmax = net.d[l + 1] > hmax ? net.d[l + 1] : hmax;
    }
    const long long nrt = (b + ML_ROWS - 1) / ML_ROWS;
    ws->nrt = (int)nrt, ws->nct = (net.M + ML_COLS - 1) / ML_COLS;
    // slices of mlp_dh_kernel: min(ceil(1024 / row tiles), ceil(M / 64)) are wanted (about 1024 waves in flight, no more slices than M holds runs of 64); the
    // length ks is M over that count rounded up to a multiple of 8 -- so at most 64 where M sets the count (M = 65: 40, M = 257: 56), longer where the
    // row tiles do (b = 4033, M = 1025: 72), and 8 for M <= 8 -- and nsl = ceil(M / ks) slices are run, the last one the shorter
    mlp_slices(nrt, net.M, ws);
    ws->resid = off, off += b * net.M;
    ws->losspart = off, off += nrt * ws->nct;
    ws->part = off, off += (long long)ws->nsl * b * net.d[net.L];
    ws->dz[0] = off, off += b * hmax;
    ws->dz[1] = off, off += b * hmax;
    ws->ca = off, off += b * hmax;
    ws->cb = off, off += b * hmax;
    ws->total = off;
}

// workspace of cp_mlp_vjp over ncols columns: the pre-activations, the weighted cotangent (B, ncols) in the place of the residual, the partial products
void mlp_vjp_work(const MlpNet& net, long long B, long long ncols, MlpWork* ws) {
    long long off = 0;
    for (int l = 0; l < net.L; ++l) ws->z[l] = off, ws->h[l] = 0, off += B * net.d[l + 1];
    const long long nrt = (B + ML_ROWS - 1) / ML_ROWS;
    ws->nrt = (int)nrt, ws->nct = (int)((ncols + ML_COLS - 1) / ML_COLS);
    mlp_slices(nrt, (int)ncols, ws);
    ws->resid = off, off += B * ncols;
    ws->part = off, off += (long long)ws->nsl * B * net.d[net.L];
    ws->losspart = ws->dz[0] = ws->dz[1] = ws->ca = ws->cb = 0;
    ws->total = off;
}

template <int MODE>
int mlp_forward_launch(cp::Launches& on, const MlpFwdArgs& A) {
    const long long nrt = (A.R + ML_ROWS - 1) / ML_ROWS, nct = (A.cend - A.c0 + ML_COLS - 1) / ML_COLS;
    if (nrt > 0x7fffffffLL || nct > 65535) return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d results (at most 2^37 rows, 2^24 - 256 columns)", on.who(), A.R, A.net.M);
    on.run<mlp_forward_kernel<MODE>>(dim3((unsigned)nrt, (unsigned)nct), 256, (size_t)2 * A.net.nr * ML_RS * sizeof(double), A);      // 40 KB at widths <= 32, at most 80 KB
    return CP_OK;
}

// What cp_mlp_predict, cp_mlp_predict_columns, cp_mlp_jacobian, cp_mlp_vjp and cp_mlp_jvp share: their checks up to the range of columns, in that order, then the
// network, the inputs and the range in F.  What follows is the entry point's own: its strides, its grid cap, the empty batch, its null pointers, its
// workspace, the device, and the outputs in F.
int mlp_front(const char* who, const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
              const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0, long long ncols,
              MlpFwdArgs* F) {
    if (B < 0) return cp::fail(CP_EINVAL, "%s: negative count of points", who);
    if (!activations) return cp::fail(CP_EINVAL, "%s: no activation codes", who);
    const int status = mlp_net(who, ndim, nlayers, widths, activations, M, &F->net);
    if (status != CP_OK) return status;
    if (yfunction < CP_MLP_Y_NONE || yfunction > CP_MLP_Y_SINH) return cp::fail(CP_EINVAL, "%s: y function %d (0 none, 1 10^v, 2 sinh)", who, yfunction);
    if (col0 < 0 || ncols < 1 || ncols > (long long)M - col0) return cp::fail(CP_EINVAL, "%s: columns [%lld, %lld + %lld) of %d", who, col0, col0, ncols, M);
    F->x = d_x, F->params = d_params, F->xoff = d_xoffset, F->xscale = d_xscale, F->yoff = d_yoffset, F->yscale = d_yscale;
    F->R = B, F->c0 = (int)col0, F->cend = (int)(col0 + ncols);
    return CP_OK;
}

// f(std::integral_constant<int, yfunction>): the one place where a checked y function becomes a template argument
template <class F>
int mlp_yfunction(int yfunction, F&& f) {
    if (yfunction == CP_MLP_Y_NONE) return f(std::integral_constant<int, CP_MLP_Y_NONE>{});
    if (yfunction == CP_MLP_Y_EXP10) return f(std::integral_constant<int, CP_MLP_Y_EXP10>{});
    return f(std::integral_constant<int, CP_MLP_Y_SINH>{});
}

// mlp_dh_kernel for a last hidden layer of width H: r (b, M) with row stride ldr times the transposed W (H, M) with row stride ldw, in the slices of ws
void mlp_dh_launch(cp::Launches& on, const double* r, long long ldr, const double* W, long long ldw, long long b, int H, int M, const MlpWork& ws, double* part) {
    const dim3 grid((unsigned)ws.nrt, (unsigned)((ws.nsl + 3) / 4));
    switch ((H + 15) / 16) {
        case 1: on.run<mlp_dh_kernel<1>>(grid, 256, 0, r, ldr, W, ldw, b, H, M, ws.nsl, ws.ks, part); break;
        case 2: on.run<mlp_dh_kernel<2>>(grid, 256, 0, r, ldr, W, ldw, b, H, M, ws.nsl, ws.ks, part); break;
        case 3: on.run<mlp_dh_kernel<3>>(grid, 256, 0, r, ldr, W, ldw, b, H, M, ws.nsl, ws.ks, part); break;
        default: on.run<mlp_dh_kernel<4>>(grid, 256, 0, r, ldr, W, ldw, b, H, M, ws.nsl, ws.ks, part);
    }
}

// workspace of cp_mlp_vjp2: that of cp_mlp_vjp, then with a y function the Gauss-Newton workspace (its slot for the value first), its result and omega
struct MlpVjp2Work {
    cpgn::Plan plan;
    long long gn, fisher, omega, total;
};

int mlp_vjp2_work(const char* who, const MlpNet& net, long long B, long long ncols, int yfunction, MlpWork* ws, MlpVjp2Work* w2) {
    mlp_vjp_work(net, B, ncols, ws);
    w2->gn = w2->fisher = w2->omega = 0, w2->total = ws->total;
    if (yfunction == CP_MLP_Y_NONE) return CP_OK;
    const int status = cpgn::plan(who, B, net.ndim, ncols, &w2->plan);
    if (status != CP_OK) return status;
    if ((B * ncols + 255) / 256 > 0x7fffffffLL)      // the grid of mlp_omega_kernel (the plan has capped B and ncols: no overflow)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld cotangents under a y function (at most 2^39)", who, B, ncols);
    w2->gn = w2->total, w2->total += w2->plan.total;
    w2->fisher = w2->total, w2->total += B * net.ndim * net.ndim;
    w2->omega = w2->total, w2->total += B * ncols;
    return CP_OK;
}

// rows B npairs of mlp_curvature_kernel against its grid, the column tiles of the forward kernel
bool mlp_vjp2_fits(long long B, int ndim, long long ncols) {
    const long long npairs = (long long)ndim * (ndim + 1) / 2;
    return B <= 0x7fffffffLL * ML_ROWS / npairs && (ncols + ML_COLS - 1) / ML_COLS <= 65535;
}

}  // namespace

extern "C" long long cp_mlp_vjp2_workspace_doubles(long long B, int ndim, int nlayers, const int* widths, int M, long long ncols, int yfunction) {
    const char* who = "cp_mlp_vjp2_workspace_doubles";
    MlpNet net;
    if (B < 0) return -(long long)cp::fail(CP_EINVAL, "%s: negative count of points", who);
    const int status = mlp_net(who, ndim, nlayers, widths, nullptr, M, &net);
    if (status != CP_OK) return -(long long)status;
    if (yfunction < CP_MLP_Y_NONE || yfunction > CP_MLP_Y_SINH) return -(long long)cp::fail(CP_EINVAL, "%s: y function %d (0 none, 1 10^v, 2 sinh)", who, yfunction);
    if (ncols < 1 || ncols > M) return -(long long)cp::fail(CP_EINVAL, "%s: %lld columns of %d", who, ncols, M);
    if (!mlp_vjp2_fits(B, ndim, ncols)) return -(long long)cp::fail(CP_EUNSUPPORTED, "%s: %lld points of %d parameters (at most 2^37 rows B ndim (ndim + 1) / 2)", who, B, ndim);
    MlpWork ws;
    MlpVjp2Work w2;
    const int planned = mlp_vjp2_work(who, net, B, ncols, yfunction, &ws, &w2);
    return planned == CP_OK ? w2.total : -(long long)planned;
}

// The launches on the stream: the forward kernel in its vjp mode and mlp_dh_kernel as in cp_mlp_vjp (the value goes to d_value, or with a y function
// to the workspace if there is none); with a y function mlp_omega_kernel, the tangent kernel's Gauss-Newton variant and gn_sum_kernel on omega; then
// mlp_curvature_kernel, which adds that sum and is the one writer of d_hess
extern "C" int cp_mlp_vjp2(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                           const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                           long long ncols, const double* d_cot, long long ldc, double* d_value, long long ldv, double* d_hess, double* d_work,
                           long long work_doubles, int device, void* stream) {
    const char* who = "cp_mlp_vjp2";
    MlpFwdArgs F{};
    int status = mlp_front(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &F);
    if (status != CP_OK) return status;
    if (ldc < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the cotangent is less than its %lld columns", who, ldc, ncols);
    if (d_value && ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    if (!mlp_vjp2_fits(B, ndim, ncols))
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d x %d second derivatives of %lld columns (at most 2^37 rows B ndim (ndim + 1) / 2, 2^24 - 256 columns)", who, B, ndim,
                        ndim, ncols);
    const MlpNet& N = F.net;
    MlpVjp2Work w2;
    status = mlp_vjp2_work(who, N, B, ncols, yfunction, &F.ws, &w2);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale || !d_cot || !d_hess || !d_work) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    const MlpWork& ws = F.ws;
    if (work_doubles < w2.total) return cp::fail(CP_EINVAL, "%s: workspace of %lld doubles, %lld needed (cp_mlp_vjp2_workspace_doubles)", who, work_doubles, w2.total);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    cp::Launches on(who, stream);
    const bool curved = yfunction != CP_MLP_Y_NONE;      // the y function's own curvature: omega J J
    double* const value = d_value || !curved ? d_value : d_work + w2.gn + w2.plan.value;
    const long long ldvalue = d_value ? ldv : ncols;
    F.cot = d_cot, F.out = value, F.work = d_work, F.ldo = ldvalue, F.ldc = ldc;
    const int launched = mlp_yfunction(yfunction, [&](auto y) { return mlp_forward_launch<ML_VJP + decltype(y)::value>(on, F); });
    if (launched != CP_OK) return launched;
    mlp_dh_launch(on, d_work + ws.resid, ncols, d_params + N.off[N.L] + col0, M, B, N.d[N.L], (int)ncols, ws, d_work + ws.part);
    if (curved) {
        double* const omega = d_work + w2.omega;
        const unsigned nblocks = (unsigned)((B * ncols + 255) / 256);      // (checked by mlp_vjp2_work)
        if (yfunction == CP_MLP_Y_EXP10) on.run<mlp_omega_kernel<CP_MLP_Y_EXP10>>(nblocks, 256, 0, d_cot, ldc, value, ldvalue, B, ncols, omega);
        else on.run<mlp_omega_kernel<CP_MLP_Y_SINH>>(nblocks, 256, 0, d_cot, ldc, value, ldvalue, B, ncols, omega);
        const cpgn::Tail tail{omega, nullptr, value, d_work + w2.gn + w2.plan.part, ncols, 0, ldvalue, B, ndim, w2.plan.P, (int)col0, (int)(col0 + ncols)};
        cpgn::mlp_launch(on, d_x, d_params, d_xoffset, d_xscale, d_yscale, N, yfunction, w2.plan, tail, d_work + w2.fisher, nullptr, nullptr);
    }
    const int npairs = ndim * (ndim + 1) / 2;
    const long long R = B * npairs;
    const MlpCurvArgs C{d_x, d_params, d_xoffset, d_xscale, d_work + ws.part, curved ? d_work + w2.fisher : nullptr, d_hess, B, R, npairs, ws.nsl, N};
    on.run<mlp_curvature_kernel>((unsigned)((R + ML_ROWS - 1) / ML_ROWS), 64 * ML_CW, (size_t)4 * N.nr * ML_PS * sizeof(double), C);
    return on.status();
}

// For cp_mlp_gauss_newton (cp_mlp_gauss_newton.hip; declared in cp_internal.h): the checks of mlp_front under its name with the network's layout, and the
// forward kernel on a range of columns among its launches -- what cp_mlp_predict_columns launches, so the value it writes has those bits.
int cp::mlp_front_layout(const char* who, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, int yfunction, long long col0,
                         long long ncols, MlpLayout* layout) {
    MlpFwdArgs F{};
    const int status = mlp_front(who, nullptr, B, ndim, nlayers, widths, activations, M, nullptr, nullptr, nullptr, nullptr, nullptr, yfunction, col0, ncols, &F);
    if (status != CP_OK) return status;
    *layout = F.net;      // (MlpNet is the layout and its total; the entries past the last layer are the zeros of F{})
    return CP_OK;
}

int cp::mlp_predict_launch(Launches& on, const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M,
                           const double* d_params, const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction,
                           long long col0, long long ncols, double* d_out, long long ldo) {
    MlpFwdArgs A{};
    const int status = mlp_front(on.who(), d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &A);
    if (status != CP_OK) return status;
    A.out = d_out, A.ldo = ldo;
    return mlp_yfunction(yfunction, [&](auto y) { return mlp_forward_launch<decltype(y)::value>(on, A); });
}

extern "C" long long cp_mlp_param_count(int ndim, int nlayers, const int* widths, int M) {
    MlpNet net;
    const int status = mlp_net("cp_mlp_param_count", ndim, nlayers, widths, nullptr, M, &net);
    return status == CP_OK ? net.total : -(long long)status;
}

extern "C" long long cp_mlp_workspace_doubles(long long b, int ndim, int nlayers, const int* widths, int M) {
    MlpNet net;
    if (b < 0) return -(long long)cp::fail(CP_EINVAL, "cp_mlp_workspace_doubles: negative batch size");
    const int status = mlp_net("cp_mlp_workspace_doubles", ndim, nlayers, widths, nullptr, M, &net);
    if (status != CP_OK) return -(long long)status;
    MlpWork ws;
    mlp_work(net, b, &ws);
    return ws.total;
}

// cp_mlp_predict is the range [0, M) with row stride M of the same call
static int mlp_predict(const char* who, const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                       const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                       long long ncols, double* d_out, long long ldo, int device, void* stream) {
    MlpFwdArgs A{};
    const int status = mlp_front(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &A);
    if (status != CP_OK) return status;
    if (ldo < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the result is less than its %lld columns", who, ldo, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    A.out = d_out, A.ldo = ldo;
    cp::Launches on(who, stream);
    const int launched = mlp_yfunction(yfunction, [&](auto y) { return mlp_forward_launch<decltype(y)::value>(on, A); });
    return launched != CP_OK ? launched : on.status();
}

extern "C" int cp_mlp_predict(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                              const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, double* d_out,
                              int device, void* stream) {
    return mlp_predict("cp_mlp_predict", d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, 0, M, d_out, M,
                       device, stream);
}

extern "C" int cp_mlp_predict_columns(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M,
                                      const double* d_params, const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale,
                                      int yfunction, long long col0, long long ncols, double* d_out, long long ldo, int device, void* stream) {
    return mlp_predict("cp_mlp_predict_columns", d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0,
                       ncols, d_out, ldo, device, stream);
}

// Two launches on the stream: the forward kernel writes the prediction on the range (what cp_mlp_predict_columns writes), the tangent kernel reads it
extern "C" int cp_mlp_jacobian(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                               const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                               long long ncols, double* d_value, long long ldv, double* d_jac, long long ldj, int device, void* stream) {
    const char* who = "cp_mlp_jacobian";
    MlpFwdArgs F{};
    const int status = mlp_front(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &F);
    if (status != CP_OK) return status;
    if (ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    if (ldj < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the Jacobian is less than its %lld columns", who, ldj, ncols);
    if (B > 0x7fffffffLL * ML_ROWS / ndim || (ncols + ML_COLS - 1) / ML_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %d x %lld results (at most 2^37 rows B ndim, 2^24 - 256 columns)", who, B, ndim, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale || !d_value || !d_jac) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    F.out = d_value, F.ldo = ldv;
    const MlpJacArgs J{d_x, d_params, d_xoffset, d_xscale, d_yscale, d_value, d_jac, B * ndim, ldv, ldj, F.c0, F.cend, F.net};
    const dim3 grid((unsigned)((J.R + ML_ROWS - 1) / ML_ROWS), (unsigned)((ncols + ML_COLS - 1) / ML_COLS));      // (checked above)
    cp::Launches on(who, stream);
    const int launched = mlp_yfunction(yfunction, [&](auto y) {
        const int forward = mlp_forward_launch<decltype(y)::value>(on, F);
        if (forward == CP_OK) mlp_tangent_launch<decltype(y)::value>(on, J, grid, 0);
        return forward;
    });
    return launched != CP_OK ? launched : on.status();
}

// Two launches on the stream as in cp_mlp_jacobian: the forward kernel writes the prediction on the range, the tangent kernel's jvp variant reads it
extern "C" int cp_mlp_jvp(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                          const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                          long long ncols, const double* d_tan, long long K, double* d_value, long long ldv, double* d_out, long long ldo, int device,
                          void* stream) {
    const char* who = "cp_mlp_jvp";
    MlpFwdArgs F{};
    const int status = mlp_front(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &F);
    if (status != CP_OK) return status;
    if (ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    if (ldo < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the result is less than its %lld columns", who, ldo, ncols);
    if (K < 1) return cp::fail(CP_EINVAL, "%s: %lld directions per point (at least 1)", who, K);
    if (K > 0x7fffffffLL || B > 0x7fffffffLL * ML_ROWS / K || (ncols + ML_COLS - 1) / ML_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld x %lld results (at most 2^37 rows B K, 2^31 - 1 directions, 2^24 - 256 columns)", who, B, K, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale || !d_tan || !d_value || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    F.out = d_value, F.ldo = ldv;
    const MlpJvpArgs J{{d_x, d_params, d_xoffset, d_xscale, d_yscale, d_value, d_out, B * K, ldv, ldo, F.c0, F.cend, F.net}, d_tan, (int)K};
    const dim3 grid((unsigned)((J.R + ML_ROWS - 1) / ML_ROWS), (unsigned)((ncols + ML_COLS - 1) / ML_COLS));      // (checked above)
    cp::Launches on(who, stream);
    const int launched = mlp_yfunction(yfunction, [&](auto y) {
        const int forward = mlp_forward_launch<decltype(y)::value>(on, F);
        if (forward == CP_OK) mlp_tangent_launch<decltype(y)::value>(on, J, grid, 0);
        return forward;
    });
    return launched != CP_OK ? launched : on.status();
}

// Up to four launches on the stream: the forward kernel writes the prediction on the range; the tangent kernel's jvp variant writes the first-order
// products along u and along v where they are given (what cp_mlp_jvp writes; the y function's chain rule needs them); mlp_tangent2_kernel reads them
extern "C" int cp_mlp_jvp2(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                           const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                           long long ncols, const double* d_tan_u, const double* d_tan_v, long long K, double* d_value, long long ldv, double* d_first_u,
                           double* d_first_v, long long ldf, double* d_out, long long ldo, int device, void* stream) {
    const char* who = "cp_mlp_jvp2";
    MlpFwdArgs F{};
    const int status = mlp_front(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &F);
    if (status != CP_OK) return status;
    const bool first = yfunction != CP_MLP_Y_NONE || d_first_u || d_first_v;
    if (ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    if (first && ldf < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the first-order products is less than their %lld columns", who, ldf, ncols);
    if (ldo < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the result is less than its %lld columns", who, ldo, ncols);
    if (K < 1) return cp::fail(CP_EINVAL, "%s: %lld directions per point (at least 1)", who, K);
    if (K > 0x7fffffffLL || B > 0x7fffffffLL * ML_ROWS / K || (ncols + ML_COLS - 1) / ML_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld x %lld results (at most 2^37 rows B K, 2^31 - 1 directions, 2^24 - 256 columns)", who, B, K, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale || !d_tan_u || !d_value || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    if (d_first_v && !d_tan_v) return cp::fail(CP_EINVAL, "%s: null pointer (d_first_v without d_tan_v)", who);
    if (yfunction != CP_MLP_Y_NONE && (!d_first_u || (d_tan_v && !d_first_v)))
        return cp::fail(CP_EINVAL, "%s: null pointer (the y function needs the first-order products)", who);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    F.out = d_value, F.ldo = ldv;
    const long long R = B * K;
    const MlpJvp2Args S{d_x, d_params, d_xoffset, d_xscale, d_yscale, d_tan_u, d_tan_v, d_value, d_first_u, d_first_v, d_out, R, ldv, ldf, ldo, F.c0, F.cend, (int)K, F.net};
    const dim3 grid((unsigned)((R + ML_ROWS - 1) / ML_ROWS), (unsigned)((ncols + ML_COLS - 1) / ML_COLS));      // (checked above)
    cp::Launches on(who, stream);
    const int launched = mlp_yfunction(yfunction, [&](auto y) {
        constexpr int YF = decltype(y)::value;
        const int forward = mlp_forward_launch<YF>(on, F);
        if (forward != CP_OK) return forward;
        const double* tans[2] = {d_tan_u, d_tan_v};
        double* firsts[2] = {d_first_u, d_first_v};
        for (int s = 0; s < 2; ++s) {
            if (!firsts[s]) continue;
            const MlpJvpArgs J{{d_x, d_params, d_xoffset, d_xscale, d_yscale, d_value, firsts[s], R, ldv, ldf, F.c0, F.cend, F.net}, tans[s], (int)K};
            mlp_tangent_launch<YF>(on, J, grid, 0);
        }
        if (d_tan_v) mlp_tangent2_launch<YF, true>(on, S, grid);
        else mlp_tangent2_launch<YF, false>(on, S, grid);
        return forward;
    });
    return launched != CP_OK ? launched : on.status();
}

extern "C" long long cp_mlp_vjp_workspace_doubles(long long B, int ndim, int nlayers, const int* widths, int M, long long ncols) {
    const char* who = "cp_mlp_vjp_workspace_doubles";
    MlpNet net;
    if (B < 0) return -(long long)cp::fail(CP_EINVAL, "%s: negative count of points", who);
    const int status = mlp_net(who, ndim, nlayers, widths, nullptr, M, &net);
    if (status != CP_OK) return -(long long)status;
    if (ncols < 1 || ncols > M) return -(long long)cp::fail(CP_EINVAL, "%s: %lld columns of %d", who, ncols, M);
    if (B > 0x7fffffffLL * ML_ROWS) return -(long long)cp::fail(CP_EUNSUPPORTED, "%s: %lld points (at most 2^37)", who, B);
    MlpWork ws;
    mlp_vjp_work(net, B, ncols, &ws);
    return ws.total;
}

// Three launches on the stream: the forward kernel (pre-activations and the weighted cotangent to the workspace, the prediction to d_value if wanted),
// mlp_dh_kernel on the weighted cotangent and the columns [col0, col0 + ncols) of the output kernel, mlp_input_grad_kernel
extern "C" int cp_mlp_vjp(const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, const double* d_params,
                          const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction, long long col0,
                          long long ncols, const double* d_cot, long long ldc, double* d_value, long long ldv, double* d_grad, double* d_work,
                          long long work_doubles, int device, void* stream) {
    const char* who = "cp_mlp_vjp";
    MlpFwdArgs F{};
    const int status = mlp_front(who, d_x, B, ndim, nlayers, widths, activations, M, d_params, d_xoffset, d_xscale, d_yoffset, d_yscale, yfunction, col0, ncols, &F);
    if (status != CP_OK) return status;
    if (ldc < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the cotangent is less than its %lld columns", who, ldc, ncols);
    if (d_value && ldv < ncols) return cp::fail(CP_EINVAL, "%s: row stride %lld of the value is less than its %lld columns", who, ldv, ncols);
    if (B > 0x7fffffffLL * ML_ROWS || (ncols + ML_COLS - 1) / ML_COLS > 65535)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld cotangents (at most 2^37 rows, 2^24 - 256 columns)", who, B, ncols);
    if (B == 0) return CP_OK;
    if (!d_x || !d_params || !d_xoffset || !d_xscale || !d_yoffset || !d_yscale || !d_cot || !d_grad || !d_work) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    const MlpNet& N = F.net;
    mlp_vjp_work(N, B, ncols, &F.ws);
    const MlpWork& ws = F.ws;
    if (work_doubles < ws.total) return cp::fail(CP_EINVAL, "%s: workspace of %lld doubles, %lld needed (cp_mlp_vjp_workspace_doubles)", who, work_doubles, ws.total);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    cp::Launches on(who, stream);
    F.cot = d_cot, F.out = d_value, F.work = d_work, F.ldo = ldv, F.ldc = ldc;
    const int launched = mlp_yfunction(yfunction, [&](auto y) { return mlp_forward_launch<ML_VJP + decltype(y)::value>(on, F); });
    if (launched != CP_OK) return launched;
    // dh of the last hidden layer, in slices of the columns: the weighted cotangent times the columns [col0, col0 + ncols) of the output kernel
    mlp_dh_launch(on, d_work + ws.resid, ncols, d_params + N.off[N.L] + col0, M, B, N.d[N.L], (int)ncols, ws, d_work + ws.part);
    const MlpGradArgs G{d_params, d_xscale, d_work, d_grad, B, N, ws};
    on.run<mlp_input_grad_kernel>((unsigned)ws.nrt, 256, (size_t)2 * N.nr * ML_GS * sizeof(double), G);
    return on.status();
}

extern "C" int cp_mlp_loss_grad(const double* d_X, const double* d_Y, long long b, int ndim, int nlayers, const int* widths, const int* activations, int M,
                                const double* d_params, double* d_work, long long work_doubles, double* d_loss, double* d_grad, int device, void* stream) {
    const char* who = "cp_mlp_loss_grad";
    MlpFwdArgs A{};
    if (b < 0) return cp::fail(CP_EINVAL, "cp_mlp_loss_grad: negative batch size");
    if (!activations) return cp::fail(CP_EINVAL, "cp_mlp_loss_grad: no activation codes");
    const int status = mlp_net(who, ndim, nlayers, widths, activations, M, &A.net);
    if (status != CP_OK) return status;
    if (b == 0) return CP_OK;
    if (!d_X || !d_Y || !d_params || !d_work || !d_loss) return cp::fail(CP_EINVAL, "cp_mlp_loss_grad: null pointer");
    const MlpNet& N = A.net;
    mlp_work(N, b, &A.ws);
    const MlpWork& ws = A.ws;
    if (work_doubles < ws.total) return cp::fail(CP_EINVAL, "cp_mlp_loss_grad: workspace of %lld doubles, %lld needed (cp_mlp_workspace_doubles)", work_doubles, ws.total);
    if ((long long)ws.nrt * 64 > 0x7fffffffLL || (b * ML_MAX_WIDTH + 255) / 256 > 0x7fffffffLL) return cp::fail(CP_EUNSUPPORTED, "cp_mlp_loss_grad: batch of %lld rows", b);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_mlp_loss_grad: cannot select device %d", device);
    cp::Launches on(who, stream);
    A.x = d_X, A.params = d_params, A.ytrue = d_Y, A.out = d_work + ws.resid, A.work = d_work, A.R = b;
    A.ldo = M, A.c0 = 0, A.cend = M;
    A.rscale = 2. / ((double)b * (double)M);
    const int launched = mlp_forward_launch<ML_TRAIN>(on, A);
    if (launched != CP_OK) return launched;
    on.run<mlp_sum_kernel>(1, 1024, 0, d_work + ws.losspart, (long long)ws.nrt * ws.nct, 1. / ((double)b * (double)M), d_loss);
    if (!d_grad) return on.status();
    const int L = N.L, H = N.d[L];
    const double* resid = d_work + ws.resid;
    {      // the output layer's gradient
        const double* hL = d_work + ws.h[L - 1];
        double* gW = d_grad + N.off[L];
        const dim3 grid((unsigned)ws.nct);
        switch ((H + 15) / 16) {
            case 1: on.run<mlp_gw_out_kernel<1>>(grid, 256, 0, hL, resid, b, H, M, gW); break;
            case 2: on.run<mlp_gw_out_kernel<2>>(grid, 256, 0, hL, resid, b, H, M, gW); break;
            case 3: on.run<mlp_gw_out_kernel<3>>(grid, 256, 0, hL, resid, b, H, M, gW); break;
            default: on.run<mlp_gw_out_kernel<4>>(grid, 256, 0, hL, resid, b, H, M, gW);
        }
    }
    mlp_dh_launch(on, resid, M, d_params + N.off[L], M, b, H, M, ws, d_work + ws.part);      // dh of the last hidden layer, in slices of the outputs
    for (int l = L - 1; l >= 0; --l) {      // hidden layer l: d[l] -> d[l + 1]
        const int nin = N.d[l], nout = N.d[l + 1];
        double* dz = d_work + ws.dz[l & 1];
        const double* ab = d_params + N.off[l] + (long long)(nin + 1) * nout;
        double* gl = d_grad + N.off[l];
        const unsigned nblocks = (unsigned)((b * nout + 255) / 256);
        if (l == L - 1)
            on.run<mlp_dz_kernel>(nblocks, 256, 0, d_work + ws.part, ws.nsl, nullptr, nullptr, 0, d_work + ws.z[l], b, nout, N.act[l], ab, dz, d_work + ws.ca,
                                  d_work + ws.cb);
        else
            on.run<mlp_dz_kernel>(nblocks, 256, 0, nullptr, 0, d_work + ws.dz[(l + 1) & 1], d_params + N.off[l + 1], N.d[l + 2], d_work + ws.z[l], b, nout, N.act[l],
                                  ab, dz, d_work + ws.ca, d_work + ws.cb);
        const double* hprev = l == 0 ? d_X : d_work + ws.h[l - 1];
        on.run<mlp_gw_hidden_kernel>((unsigned)(((nin + 1) * nout + 63) / 64), 1024, 0, hprev, dz, b, nin, nout, gl, N.act[l] != ACT_IDENTITY_SILU);
        double* gab = gl + (long long)(nin + 1) * nout;
        if (N.act[l] == ACT_IDENTITY_SILU) {
            on.run<mlp_sum_kernel>(1, 1024, 0, d_work + ws.ca, b * nout, 1., gab);
            on.run<mlp_sum_kernel>(1, 1024, 0, d_work + ws.cb, b * nout, 1., gab + 1);
        }
    }
    return on.status();
}

extern "C" int cp_mlp_adam(double* d_params, double* d_m, double* d_v, const double* d_grad, long long n, double lr, double b1, double b2, double eps, double c1,
                           double c2, int device, void* stream) {
    if (n < 0) return cp::fail(CP_EINVAL, "cp_mlp_adam: negative count of parameters");
    if (!(c1 > 0.) || !(c2 > 0.)) return cp::fail(CP_EINVAL, "cp_mlp_adam: bias corrections c1 = %g, c2 = %g must be positive", c1, c2);
    if (n == 0) return CP_OK;
    if (!d_params || !d_m || !d_v || !d_grad) return cp::fail(CP_EINVAL, "cp_mlp_adam: null pointer");
    if ((n + 255) / 256 > 0x7fffffffLL) return cp::fail(CP_EUNSUPPORTED, "cp_mlp_adam: %lld parameters", n);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_mlp_adam: cannot select device %d", device);
    cp::Launches on("cp_mlp_adam", stream);
    on.run<mlp_adam_kernel>((unsigned)((n + 255) / 256), 256, 0, d_params, d_m, d_v, d_grad, n, lr, b1, b2, eps, c1, c2);
    return on.status();
}
