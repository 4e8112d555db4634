// cp_xi_filter.hip -- the kirkby2013 correlation-function BAO filter (reference bao_filter.py:835-909) over many rows of xi(s), one rs_drag ratio per
// cosmology, in one launch.  Per row, with rho the ratio of its cosmology:
//   precision_i = interp(s_i / rho, knots, weights)              on the fit samples [fit_begin, fit_end)  (np.interp, 0 outside)
//   center_i    = interp(s_i / rho, knots[2:6], 1 - weights[2:6]) on every sample
//   p           = the weighted least-squares fit of the five powers (s / 128)^(1 - j), j = 0 .. 4, on the fit samples
//   xinow_i     = (1 - center_i) xi_i + center_i fit(s_i)
// The powers are scaled by 128 (exact): the normal matrix of the raw powers s^1 .. s^-3 has a condition number of 3e19, that of the scaled ones 1e7.
// Its entries depend on j + k only (a Hankel matrix: 9 moments); with the 5 right-hand sides, 14 sums per row, reduced across the wave in one
// transposed pass (17 lane exchanges instead of 84), then an LDL^T solve in registers.
// HBM-bound: 16 ns bytes per row (xi read once, xinow written once).  A wave per row; rows with ns even and <= 1024 (16-byte aligned) are read with
// 16-byte loads, all issued before the first use, and staged in LDS; any other row is read one sample per lane, the fit samples, then the row.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/cosmoprimo_amd.h"
#include "cp_error.h"
#include "cp_internal.h"

namespace {

constexpr double PIVOT = 128., INV_PIVOT = 1. / 128.;
constexpr int NV = 8, ROW_LDS = 128 * NV;     // double2 per lane of the staged kernel: rows of up to 1024 samples
constexpr int BLOCK = 256, WAVES_PER_BLOCK = BLOCK / 64;

struct Window {
    double knot[8], weight[8], slope[7];    // precision: np.interp(x, knot, weight, left=0, right=0)
    double cvalue[4], cslope[3];            // blend: np.interp(x, knot[2:6], cvalue = 1 - weight[2:6], left=0, right=0)
};

struct Args {
    const double* xi;
    double* out;
    const double* s;
    const double* rescale;
    long long nrows, per_cosmology;
    int ns, fit_begin, fit_end;
    Window w;
};

// np.interp(x, xp, fp, left=0, right=0) on N knots: slope[j] (x - xp[j]) + fp[j] on [xp[j], xp[j+1]), fp[N-1] at xp[N-1], NaN for NaN.  The knots
// come from the kernel's arguments (scalar registers); the segment's knot, value and slope are read from the window's copy in LDS (T: the table)
template <int N>
__device__ __forceinline__ double interp(double x, const double* xp, const double* xp_lds, const double* fp_lds, const double* slope_lds) {
    int j = -1;
#pragma unroll
    for (int k = 0; k < N; ++k) j += x >= xp[k];
    double v = 0.;
    if (j == N - 1) v = x == xp[N - 1] ? fp_lds[N - 1] : 0.;
    else if (j >= 0) v = fma(slope_lds[j], x - xp_lds[j], fp_lds[j]);
    return x == x ? v : x;
}

// one fit sample into the partial sums: acc[m] = sum w t^(2 - m), m = 0 .. 8 (the moments), acc[9 + j] = sum w xi t^(1 - j), j = 0 .. 4
__device__ __forceinline__ void accumulate(double s, double xi, double rho, const Window& W, const Window& T, double (&acc)[16]) {
    const double w = interp<8>(s / rho, W.knot, T.knot, T.weight, T.slope);
    const double t = s * INV_PIVOT, u = PIVOT / s, u2 = u * u, u3 = u2 * u;
    const double wx = w * xi, wt = w * t, wu = w * u;
    acc[0] = fma(wt, t, acc[0]);
    acc[1] += wt;
    acc[2] += w;
    acc[3] += wu;
    acc[4] = fma(wu, u, acc[4]);
    acc[5] = fma(wu, u2, acc[5]);
    acc[6] = fma(wu, u3, acc[6]);
    acc[7] = fma(wu * u2, u2, acc[7]);
    acc[8] = fma(w * u3, u3, acc[8]);
    acc[9] = fma(wx, t, acc[9]);
    acc[10] += wx;
    acc[11] = fma(wx, u, acc[11]);
    acc[12] = fma(wx, u2, acc[12]);
    acc[13] = fma(wx, u3, acc[13]);
}

// sums of the 16 partials over the wave, transposed: at each exchange a lane keeps half of its values and receives the partner's half; afterwards
// lane 4 m holds the total of acc[m] (m = 8 b5 + 4 b4 + 2 b3 + b2 of the lane's bits)
__device__ __forceinline__ double wave_sums(double (&acc)[16], int lane) {
#pragma unroll
    for (int h = 8, mask = 32; h >= 1; h >>= 1, mask >>= 1) {
        const bool upper = lane & mask;
#pragma unroll
        for (int i = 0; i < h; ++i) {
            const double keep = upper ? acc[i + h] : acc[i], send = upper ? acc[i] : acc[i + h];
            acc[i] = keep + __shfl_xor(send, mask);
        }
    }
    double v = acc[0];
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    return v;
}

// a wave's LDS accesses run in order: this only keeps the compiler from moving them across the phases of a row
__device__ __forceinline__ void wave_lds_phase() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double lane_value(double v, int src) {
    const long long bits = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the fit's parameters from the reduced sums: G p = R with G[j][k] = M[j + k], by LDL^T (G is symmetric positive definite)
__device__ __forceinline__ void solve(double total, double (&p)[5]) {
    double M[9], R[5];
#pragma unroll
    for (int m = 0; m < 9; ++m) M[m] = lane_value(total, 4 * m);
#pragma unroll
    for (int j = 0; j < 5; ++j) R[j] = lane_value(total, 4 * (9 + j));
    double L[5][5], D[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        double d = M[2 * j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 5; ++i) {
            double a = M[i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k] * D[k];
            L[i][j] = a / d;
        }
    }
    double y[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        double v = R[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 4; i >= 0; --i) {
        double v = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 5; ++k) v -= L[k][i] * p[k];
        p[i] = v;
    }
}

__device__ __forceinline__ bool all_finite(const double (&p)[5]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) ok = ok && isfinite(p[j]);
    return ok;
}

// may the blend factor of separation s be non-zero (x = s / rho inside [knot[2], knot[5]])?  A superset of the samples where it is, tested with
// 1 / rho; the value itself is then computed with s / rho, as the reference does
__device__ __forceinline__ bool maybe_center(double s, double inv_rho, const Window& W) {
    const double x = s * inv_rho;
    return x >= W.knot[2] * (1. - 1e-12) && x <= W.knot[5] * (1. + 1e-12);
}

// xinow of one sample: (1 - c) xi + c fit(s); where c = 0 the reference's fit * 0 makes a non-finite fit NaN
__device__ __forceinline__ double blended(double s, double xi, double rho, const double (&p)[5], const Window& W, const Window& T) {
    const double c = interp<4>(s / rho, W.knot + 2, T.knot + 2, T.cvalue, T.cslope);
    const double t = s * INV_PIVOT, u = PIVOT / s;
    const double fit = fma(p[0], t, p[1]) + u * fma(u, fma(u, p[4], p[3]), p[2]);
    return fma(c, fit, (1. - c) * xi);
}

// the window in LDS, for the reads at a per-lane segment of interp (all 30 values in scalar registers are more than a wave has beside the rest)
__device__ __forceinline__ void stage_window(const Args& A, Window& T) {
    if (threadIdx.x == 0) T = A.w;
    __syncthreads();
}

__device__ __forceinline__ double rescale_of(const Args& A, long long row) {
    return A.rescale[A.per_cosmology == 1 ? row : row / A.per_cosmology];
}

// rows of at most 2 x NV x 64 samples, ns even, every pointer 16-byte aligned: the row is requested in NV 16-byte loads per lane, all issued before
// the first use, and staged in the wave's slice of LDS (ROW_LDS doubles), from which the fit and the blend read what they need without unrolling
__global__ __launch_bounds__(BLOCK) void kirkby_rows_kernel(Args A) {
    __shared__ double2 lds_s[ROW_LDS / 2];
    __shared__ double2 lds_x[WAVES_PER_BLOCK][ROW_LDS / 2];
    __shared__ Window T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long nwaves = (long long)gridDim.x * WAVES_PER_BLOCK;
    const int n2 = A.ns >> 1;
    for (int j = threadIdx.x; j < n2; j += BLOCK) lds_s[j] = reinterpret_cast<const double2*>(A.s)[j];
    stage_window(A, T);
    const double* ss = reinterpret_cast<const double*>(lds_s);
    const double* xs = reinterpret_cast<const double*>(lds_x[wave]);
    for (long long row = (long long)blockIdx.x * WAVES_PER_BLOCK + wave; row < A.nrows; row += nwaves) {
        const double2* x2 = reinterpret_cast<const double2*>(A.xi + row * A.ns);
        double2 x[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int j = lane + 64 * k;
            x[k] = j < n2 ? x2[j] : make_double2(0., 0.);
        }
        const double rho = rescale_of(A, row), inv_rho = 1. / rho;
        wave_lds_phase();      // (the previous row's reads of the slice are done)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int j = lane + 64 * k;
            if (j < n2) lds_x[wave][j] = x[k];
        }
        wave_lds_phase();
        double acc[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) acc[m] = 0.;
        for (int i = A.fit_begin + lane; i < A.fit_end; i += 64) accumulate(ss[i], xs[i], rho, A.w, T, acc);
        double p[5];
        solve(wave_sums(acc, lane), p);
        const bool finite = all_finite(p);
        double2* o2 = reinterpret_cast<double2*>(A.out + row * A.ns);
        for (int j = lane; j < n2; j += 64) {
            const double2 sv = lds_s[j];
            double2 o = lds_x[wave][j];
            const bool in0 = maybe_center(sv.x, inv_rho, A.w), in1 = maybe_center(sv.y, inv_rho, A.w);
            o.x = in0 ? blended(sv.x, o.x, rho, p, A.w, T) : (finite ? o.x : NAN);
            o.y = in1 ? blended(sv.y, o.y, rho, p, A.w, T) : (finite ? o.y : NAN);
            o2[j] = o;
        }
    }
}

// any row: the fit samples, then the whole row, one sample per lane and pass
__global__ __launch_bounds__(BLOCK) void kirkby_rows_any_kernel(Args A) {
    __shared__ Window T;
    stage_window(A, T);
    const int lane = threadIdx.x & 63;
    const long long nwaves = (long long)gridDim.x * WAVES_PER_BLOCK;
    for (long long row = (long long)blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6); row < A.nrows; row += nwaves) {
        const double* x = A.xi + row * A.ns;
        const double rho = rescale_of(A, row), inv_rho = 1. / rho;
        double acc[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) acc[m] = 0.;
        for (int i = A.fit_begin + lane; i < A.fit_end; i += 64) accumulate(A.s[i], x[i], rho, A.w, T, acc);
        double p[5];
        solve(wave_sums(acc, lane), p);
        const bool finite = all_finite(p);
        double* o = A.out + row * A.ns;
        for (int i = lane; i < A.ns; i += 64) {
            const double si = A.s[i], xi = x[i];
            o[i] = maybe_center(si, inv_rho, A.w) ? blended(si, xi, rho, p, A.w, T) : (finite ? xi : NAN);
        }
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int cp_kirkby2013_rows(const double* d_xi, double* d_xinow, long long nrows, int ns, const double* d_s, int fit_begin, int fit_end,
                                  const double* d_rescale, long long rows_per_cosmology, const double* knots8, const double* weights8, int device,
                                  void* stream) {
    if (nrows < 0 || ns < 1 || rows_per_cosmology < 1) return cp::fail(CP_EINVAL, "cp_kirkby2013_rows: bad sizes");
    if (fit_begin < 0 || fit_end > ns || fit_end - fit_begin < 5)
        return cp::fail(CP_EINVAL, "cp_kirkby2013_rows: the fit range [%d, %d) must hold at least 5 of the %d samples", fit_begin, fit_end, ns);
    if (!knots8 || !weights8) return cp::fail(CP_EINVAL, "cp_kirkby2013_rows: null window");
    Args A;
    Window& W = A.w;
    for (int j = 0; j < 8; ++j) {
        if (!std::isfinite(knots8[j]) || !std::isfinite(weights8[j]) || knots8[j] <= 0. || (j && knots8[j] <= knots8[j - 1]))
            return cp::fail(CP_EINVAL, "cp_kirkby2013_rows: the window knots must be positive, finite and ascending");
        W.knot[j] = knots8[j];
        W.weight[j] = weights8[j];
    }
    for (int j = 0; j < 7; ++j) W.slope[j] = (weights8[j + 1] - weights8[j]) / (knots8[j + 1] - knots8[j]);
    for (int j = 0; j < 4; ++j) W.cvalue[j] = 1. - weights8[2 + j];
    for (int j = 0; j < 3; ++j) W.cslope[j] = (W.cvalue[j + 1] - W.cvalue[j]) / (knots8[3 + j] - knots8[2 + j]);
    if (nrows == 0) return CP_OK;
    if (!d_xi || !d_xinow || !d_s || !d_rescale) return cp::fail(CP_EINVAL, "cp_kirkby2013_rows: null pointer");
    A.xi = d_xi;
    A.out = d_xinow;
    A.s = d_s;
    A.rescale = d_rescale;
    A.nrows = nrows;
    A.per_cosmology = rows_per_cosmology;
    A.ns = ns;
    A.fit_begin = fit_begin;
    A.fit_end = fit_end;
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_kirkby2013_rows: cannot select device %d", device);
    const long long blocks = (nrows + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const unsigned grid = (unsigned)(blocks < 2048 ? blocks : 2048);      // a wave per row, 8 workgroups per CU at most; the waves walk the rest
    const bool in_registers = ns % 2 == 0 && ns <= 128 * NV && aligned16(d_xi) && aligned16(d_xinow) && aligned16(d_s);
    cp::Launches on("cp_kirkby2013_rows", stream);
    if (in_registers)
        on.run<kirkby_rows_kernel>(grid, BLOCK, 0, A);
    else
        on.run<kirkby_rows_any_kernel>(grid, BLOCK, 0, A);
    return on.status();
}
