// cp_spline_tables.hip -- many splines at once, each on ITS OWN knots with values all of them share: the inverse of a monotonic table for a batch
// of cosmologies (gfx950) + C ABI.
//
// DistanceToRedshift (reference utils.py:275-316) splines the redshift grid over a cosmology's distances, Interpolator1D(rgrid, zgrid)
// (jax.py:139-177: CubicSpline(bc_type='natural') for k = 3, interp1d(kind='linear') for k = 1).  For a batch of cosmologies the knots (the
// distances) differ from row to row and the values (the redshifts) are shared -- neither cp_spline_points (one set of knots, many queries) nor
// cp_spline_columns (per-row knots, a few shared queries) fits.  Two steps:
//   build : one wave per row.  The row's knots and the values go to LDS; the system for the knot first derivatives (scipy's, natural ends) is
//           diagonally dominant, so every lane eliminates its own run of intervals plus TAB_HALO knots on either side (the scheme of
//           column_spline_kernel, cp_spline.hip) and the row is solved in (n / 64 + 2 TAB_HALO) dependent steps instead of 2 n.  What is written
//           are the four polynomial coefficients of every interval, so that a query is a search and a Horner form: no division.  The LAST interval
//           is written in a form that holds the values of both its knots (table_last below): a power form returns the value of the interval's
//           left knot exactly and its right knot within rounding only, and the last knot of a row is the right knot of an interval alone.
//   apply : a search plus one cubic per (row, query).  Many queries per row (a catalogue under a few hundred trial cosmologies): the workgroup
//           stages its row in LDS and every lane bisects there (spline_points_lds_kernel's scheme, cp_interp.hip).  Very many rows with a few
//           queries each (chain samples): one lane per (row, query) bisects in the row's knots in memory -- filling LDS would cost more than
//           the queries.  Both evaluate the same coefficients with the same instructions: bit-identical results.
// A row whose knots are not finite or not strictly ascending gets ok = 0 at build and comes out NaN throughout; the other rows never see it.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/cosmoprimo_amd.h"
#include "cp_error.h"
#include "cp_internal.h"

namespace {

// Knots a lane eliminates beyond either end of its run.  What the elimination still knows of its (wrong) start after k knots is the product of its k
// factors c_i = dx_{i-1} / (2 (dx_{i-1} + dx_i) - dx_i c_{i-1}), each < 1/2: 2 - sqrt(3) = 0.268 per knot on uniform knots, dx_{i-1} / (2 dx_{i-1} + 1.5 dx_i)
// at least where the spacing changes, so -> 1/2 only along knots whose spacing shrinks by a large factor at EVERY step in the direction of the
// elimination.  40 knots hold the tolerance of the tests (1e-11 relative) on every family of tests/spline_tables_cases.py, spacings that double over 39
// consecutive knots among them (32 did not: 3 tolerances); spacings that grow geometrically over more knots than that are outside the guarantee
// (tools/gen_spline_tables_edges_golden.py states the condition on a table, DESIGN.md section 6 the families).
constexpr int TAB_HALO = 40;
constexpr int TAB_MAX_KNOTS = 4096;      // build: knots, values and the run's eliminated rows in LDS, 32 n bytes = 128 KB
constexpr int TAB_LDS_KNOTS = 2048;      // apply: knots + 4 coefficients per interval in LDS, 80 KB (SPLINE_LDS_KNOTS of cp_interp.hip)
constexpr long long TAB_LDS_QUERIES = 4096;      // per row, from which on staging the row (5 n loads per workgroup) is cheaper than bisecting in memory

// intervals per lane of the build: odd, so that the lanes' LDS addresses (run apart) fall on different banks
__host__ __device__ inline int table_run(int n) { return ((n - 1 + 63) / 64) | 1; }

// ---- build ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void spline_tables_build_kernel(const double* __restrict__ xk, const double* __restrict__ y, long long nrows, int n,
                                                                 int order, double* __restrict__ coef, int* __restrict__ ok_out) {
    extern __shared__ double rowlds[];      // knots (n), values (n), then the eliminated rows (c, d) of the lanes' own runs (n each)
    double* xs = rowlds;
    double* ys = rowlds + n;
    double* cs = ys + n;
    double* ds = cs + n;
    const int lane = threadIdx.x;
    const int run = table_run(n);
    for (long long row = blockIdx.x; row < nrows; row += gridDim.x) {
        const double* xr = xk + row * n;
        bool bad = false;
        for (int i = lane; i < n; i += 64) {
            const double v = xr[i];
            xs[i] = v;
            ys[i] = y[i];
            bad |= !(v - v == 0.) || (i > 0 && !(v > xr[i - 1]));      // NaN, Inf, or not above its left neighbour
        }
        cp::wave_lds_phase();
        const bool ok = !__any(bad);
        if (lane == 0) ok_out[row] = ok ? 1 : 0;
        const int a = lane * run, b = a + run < n - 1 ? a + run : n - 1;      // the lane's intervals [a, b)
        if (ok && a < b) {
            double4* out = reinterpret_cast<double4*>(coef + (row * (n - 1) + a) * 4);
            if (order == 1) {
                for (int k = a; k < b; ++k)
                    out[k - a] = k == n - 2 ? double4{ys[k], 0., 0., ys[k + 1]} : double4{ys[k], (ys[k + 1] - ys[k]) / (xs[k + 1] - xs[k]), 0., 0.};
            } else {
                // scipy CubicSpline, bc_type='natural': 2 s_0 + s_1 = 3 slope_0; dxp s_{i-1} + 2 (dxm + dxp) s_i + dxm s_{i+1} = 3 (dxp slm + dxm slp);
                // s_{n-2} + 2 s_{n-1} = 3 slope_{n-2}.  From the left, knot f0 as if the spline began there: s_i + c_i s_{i+1} = d_i up to knot b - 1
                const int f0 = a - TAB_HALO > 0 ? a - TAB_HALO : 0, f1 = b + TAB_HALO < n - 1 ? b + TAB_HALO : n - 1;
                double dxm = xs[f0 + 1] - xs[f0], slm = (ys[f0 + 1] - ys[f0]) / dxm;
                double c = 0.5, d = 1.5 * slm;
                if (f0 >= a) { cs[f0] = c; ds[f0] = d; }
                for (int i = f0 + 1; i < b; ++i) {
                    const double dxp = xs[i + 1] - xs[i], slp = (ys[i + 1] - ys[i]) / dxp;
                    const double inv = 1. / (2. * (dxm + dxp) - dxp * c);
                    c = dxm * inv;
                    d = (3. * (dxp * slm + dxm * slp) - dxp * d) * inv;
                    if (i >= a) { cs[i] = c; ds[i] = d; }
                    dxm = dxp; slm = slp;
                }
                // from the right, knot f1 as if the spline ended there: s_i + e_i s_{i-1} = g_i down to knot b
                double dxp = xs[f1] - xs[f1 - 1], slp = (ys[f1] - ys[f1 - 1]) / dxp;
                double e = 0.5, g = 1.5 * slp;
                for (int i = f1 - 1; i >= b; --i) {
                    const double dxl = xs[i] - xs[i - 1], sll = (ys[i] - ys[i - 1]) / dxl;
                    const double inv = 1. / (2. * (dxl + dxp) - dxl * e);
                    e = dxp * inv;
                    g = (3. * (dxp * sll + dxl * slp) - dxl * g) * inv;
                    dxp = dxl; slp = sll;
                }
                // the two relations that meet between knots b - 1 and b give s_b; then back through the lane's own rows
                double s_hi = (g - e * ds[b - 1]) / (1. - e * cs[b - 1]);
                for (int k = b - 1; k >= a; --k) {
                    const double s_lo = ds[k] - cs[k] * s_hi;
                    // PPoly coefficients of the interval as scipy's CubicSpline forms them (spline_points_kernel, cp_interp.hip)
                    const double h = xs[k + 1] - xs[k], slope = (ys[k + 1] - ys[k]) / h;
                    const double t = (s_lo + s_hi - 2. * slope) / h;
                    if (k == n - 2) {      // table_last: with t = u / h, (1 - t) y_k + t y_{k+1} + t (1 - t) (A + t (B - A)), A = h s_k - dy, B = dy - h s_{k+1}
                        const double dy = ys[k + 1] - ys[k], A = h * s_lo - dy;
                        out[k - a] = double4{ys[k], A, (dy - h * s_hi) - A, ys[k + 1]};
                    } else {
                        out[k - a] = double4{ys[k], s_lo, (slope - s_lo) / h - t, t / h};
                    }
                    s_hi = s_lo;
                }
            }
        }
        cp::wave_lds_phase();      // the next row overwrites the staging
    }
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------------------
// the cubic of one interval at u = x - x_k; explicit fused multiply-adds: the two kernels below must round alike
__device__ __forceinline__ double table_cubic(double c0, double c1, double c2, double c3, double u) { return fma(u, fma(u, fma(u, c3, c2), c1), c0); }

// the last interval, c = (y_{n-2}, A, B - A, y_{n-1}), at t = u / h: t is exactly 0 at its left knot and exactly 1 (h / h) at the last knot of the row, where every
// term but the knot's own value is an exact zero -- both knots return their values bit for bit.  One division, for the queries of this one interval only.
__device__ __forceinline__ double table_last(const double4 c, double u, double h) {
    const double t = u / h;
    return fma(t * (1. - t), fma(t, c.z, c.y), fma(t, c.w, fma(-t, c.x, c.x)));
}

// (a branch, not a select: the division is not to be paid by the queries of the other intervals)
__device__ __forceinline__ double table_eval(const double4 c, double u, double h, bool last) {
    if (__builtin_expect(last, 0)) return table_last(c, u, h);
    return table_cubic(c.x, c.y, c.z, c.w, u);
}

struct ApplyArgs {
    const double* xk;      // (nrows, n)
    const double* coef;    // (nrows, n - 1, 4)
    const int* ok;         // (nrows)
    long long nrows, nq;
    int n, per_row;
    int* flag;             // raised by a query outside its row's knots (or NaN) in a row that is ok; NULL: nobody asked
};

// many queries per row: workgroup (row, w of nsplit) stages the row and takes the queries w * 256 + tid, + 256 nsplit, ...
template <typename real>
__global__ __launch_bounds__(256) void spline_tables_lds_kernel(const ApplyArgs A, const real* __restrict__ xq, real* __restrict__ out, int nsplit) {
    extern __shared__ __attribute__((aligned(32))) double lds[];      // (c0, c1, c2, c3) of the n - 1 intervals (read 32 bytes at a time), then the knots (n)
    const int n = A.n;
    double* cf = lds;
    double* xs = lds + 4 * (n - 1);
    const long long row = blockIdx.x / nsplit;
    const int w = (int)(blockIdx.x - row * nsplit);
    const real* q = xq + (A.per_row ? row * A.nq : 0);
    real* o = out + row * A.nq;
    if (!A.ok[row]) {      // (workgroup-uniform)
        for (long long i = (long long)w * 256 + threadIdx.x; i < A.nq; i += 256LL * nsplit) o[i] = (real)__builtin_nan("");
        return;
    }
    const double* xr = A.xk + row * n;
    const double* cr = A.coef + row * (n - 1) * 4;
    for (int i = threadIdx.x; i < n; i += 256) xs[i] = xr[i];
    for (int i = threadIdx.x; i < 4 * (n - 1); i += 256) cf[i] = cr[i];
    __syncthreads();
    const double x0 = xs[0], xn = xs[n - 1];
    bool outside = false;
    for (long long i = (long long)w * 256 + threadIdx.x; i < A.nq; i += 256LL * nsplit) {
        const double v = (double)q[i];
        double r = __builtin_nan("");
        if (v >= x0 && v <= xn) {
            int lo = 0, hi = n - 1;      // xs[lo] <= v < xs[hi], or v == xn in the last interval
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (xs[mid] <= v) lo = mid; else hi = mid;
            }
            const double4 c = *reinterpret_cast<const double4*>(cf + 4 * lo);
            r = table_eval(c, v - xs[lo], xn - xs[n - 2], lo == n - 2);
        } else {
            outside = true;
        }
        o[i] = (real)r;
    }
    if (outside && A.flag) atomicOr(A.flag, 1);
}

// a few queries per row (or rows too long for LDS): one lane per (row, query), the bisection in the row's knots in memory
template <typename real>
__global__ __launch_bounds__(256) void spline_tables_rows_kernel(const ApplyArgs A, const real* __restrict__ xq, real* __restrict__ out) {
    const int n = A.n;
    const long long total = A.nrows * A.nq;
    bool outside = false;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / A.nq;
        const double v = (double)xq[A.per_row ? i : i - row * A.nq];
        double r = __builtin_nan("");
        if (A.ok[row]) {
            const double* xr = A.xk + row * n;
            const double x0 = xr[0], xn = xr[n - 1];
            if (v >= x0 && v <= xn) {
                int lo = 0, hi = n - 1;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (xr[mid] <= v) lo = mid; else hi = mid;
                }
                const double4 c = *reinterpret_cast<const double4*>(A.coef + (row * (n - 1) + lo) * 4);
                r = table_eval(c, v - xr[lo], xn - xr[lo], lo == n - 2);
            } else {
                outside = true;
            }
        }
        out[i] = (real)r;
    }
    if (outside && A.flag) atomicOr(A.flag, 1);
}

template <typename real>
int spline_tables_apply(const double* d_xk, const double* d_coef, const int* d_ok, long long nrows, int n, const real* d_xq, int per_row, long long nq,
                        real* d_out, int* d_flag, int* outside, int device, void* stream, const char* who) {
    if (nrows < 0 || nq < 0 || n < 2) return cp::fail(CP_EINVAL, "%s: need n >= 2 knots and non-negative counts of rows and queries", who);
    if (outside) *outside = 0;
    if (nrows == 0 || nq == 0) return CP_OK;
    if (!d_xk || !d_coef || !d_ok || !d_xq || !d_out) return cp::fail(CP_EINVAL, "%s: null pointer", who);
    if (outside && !d_flag) return cp::fail(CP_EINVAL, "%s: the range flag needs a device word (d_flag)", who);
    if (nq > (1LL << 40) / nrows) return cp::fail(CP_EUNSUPPORTED, "%s: %lld x %lld results (at most 2^40)", who, nrows, nq);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    hipStream_t hs = static_cast<hipStream_t>(stream);
    cp::Launches on(who, stream);
    int* flag = outside ? d_flag : nullptr;
    if (flag && hipMemsetAsync(flag, 0, sizeof(int), hs) != hipSuccess) return cp::fail(CP_EDEVICE, "%s: clearing the range flag failed", who);
    const ApplyArgs A{d_xk, d_coef, d_ok, nrows, nq, n, per_row ? 1 : 0, flag};
    if (n <= TAB_LDS_KNOTS && nq >= TAB_LDS_QUERIES && nrows <= (1 << 20)) {
        // workgroups per row: at least 8192 queries each (twice what pays for the staging), about 2048 workgroups in all
        long long nsplit = nq / 8192, cap = 2048 / nrows;
        nsplit = nsplit < cap ? nsplit : cap;
        nsplit = nsplit < 1 ? 1 : nsplit;
        const size_t lds = (size_t)(n + 4 * (n - 1)) * sizeof(double);
        on.run<spline_tables_lds_kernel<real>>((unsigned)(nrows * nsplit), 256, lds, A, d_xq, d_out, (int)nsplit);
    } else {
        const long long blocks = (nrows * nq + 255) / 256;
        const unsigned grid = (unsigned)(blocks < 256 * 16 ? blocks : 256 * 16);
        on.run<spline_tables_rows_kernel<real>>(grid, 256, 0, A, d_xq, d_out);
    }
    int st = on.status();
    if (st == CP_OK && outside) {      // the flag comes back with the stream drained (cp_interp_table_apply)
        int host = 0;
        if (hipMemcpyAsync(&host, d_flag, sizeof(int), hipMemcpyDeviceToHost, hs) != hipSuccess || hipStreamSynchronize(hs) != hipSuccess)
            st = cp::fail(CP_EDEVICE, "%s: reading the range flag failed", who);
        if (st == CP_OK && host) *outside = 1;
    }
    return st;
}

}  // namespace

extern "C" int cp_spline_tables_build(const double* d_xk, const double* d_y, long long nrows, int n, int order, double* d_coef, int* d_ok, int device,
                                      void* stream) {
    if (nrows < 0 || n < 2) return cp::fail(CP_EINVAL, "cp_spline_tables_build: need n >= 2 knots and a non-negative count of rows");
    if (order != 1 && order != 3) return cp::fail(CP_EINVAL, "cp_spline_tables_build: order %d (1: linear, 3: natural cubic spline)", order);
    if (nrows == 0) return CP_OK;
    if (!d_xk || !d_y || !d_coef || !d_ok) return cp::fail(CP_EINVAL, "cp_spline_tables_build: null pointer");
    if (n > TAB_MAX_KNOTS) return cp::fail(CP_EUNSUPPORTED, "cp_spline_tables_build: %d knots per row (at most %d: a row is solved in LDS)", n, TAB_MAX_KNOTS);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_spline_tables_build: cannot select device %d", device);
    const size_t lds = (size_t)4 * n * sizeof(double);
    const unsigned grid = (unsigned)(nrows < 256 * 32 ? nrows : 256 * 32);
    cp::Launches on("cp_spline_tables_build", stream);
    on.run<spline_tables_build_kernel>(grid, 64, lds, d_xk, d_y, nrows, n, order, d_coef, d_ok);
    return on.status();
}

extern "C" int cp_spline_tables_apply(const double* d_xk, const double* d_coef, const int* d_ok, long long nrows, int n, const double* d_xq, int per_row,
                                      long long nq, double* d_out, int* d_flag, int* outside, int device, void* stream) {
    return spline_tables_apply<double>(d_xk, d_coef, d_ok, nrows, n, d_xq, per_row, nq, d_out, d_flag, outside, device, stream, "cp_spline_tables_apply");
}

extern "C" int cp_spline_tables_apply_f32(const double* d_xk, const double* d_coef, const int* d_ok, long long nrows, int n, const float* d_xq, int per_row,
                                          long long nq, float* d_out, int* d_flag, int* outside, int device, void* stream) {
    return spline_tables_apply<float>(d_xk, d_coef, d_ok, nrows, n, d_xq, per_row, nq, d_out, d_flag, outside, device, stream, "cp_spline_tables_apply_f32");
}
