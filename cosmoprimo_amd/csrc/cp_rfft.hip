// cp_rfft.hip -- batched real FFTs of rows (gfx950) + C ABI: the two methods of the reference's FFT engine protocol,
//   forward(fun)  = rfft(fun, axis=-1)                      (cosmoprimo/fftlog.py:536-539)
//   backward(fun) = irfft(conj(fun), n=size, axis=-1)       (cosmoprimo/fftlog.py:541-544)
// as standalone transforms on device rows, for callers that hold an engine object (NumpyFFTEngine / FFTWEngine by name) and call its methods
// themselves.  FFTlog.__call__ does not come through here: it is the fused kernel (cp_fftlog_kernel.h).
//
// A real row of N samples is ONE complex FFT of M = N / 2 points (z_m = x_2m + i x_2m+1) and a pass over its spectrum:
//   E_k = (Z_k + conj Z_{M-k}) / 2,  O_k = (Z_k - conj Z_{M-k}) / 2i,  X_k = E_k + e^{-2 pi i k / N} O_k,  k = 0 .. M  (Z_M = Z_0),
// and back  Z_k = E_k + i O_k  with  E_k = (X_k + conj X_{M-k}) / 2,  O_k = (X_k - conj X_{M-k}) / 2 e^{+2 pi i k / N},  z = IFFT_M(Z) =
// conj(FFT_M(conj Z)) / M.  A workgroup takes a row at a time: rows never share a transform, so a NaN or a huge row cannot reach another
// (numpy transforms row by row); a row that holds a NaN or an infinity is stored as NaN, every number of it, as the paired transforms of the
// library store such a row (cp_dst.hip, cp_fftlog_body.h).  The complex FFT is the workgroup transform of cp_fft_workgroup.h, which cp_dst.hip runs too: the
// passes of the FFTLog kernel (cp_fft_core.h), the twiddles of the passes behind the first resident in LDS.  The imaginary parts of the DC and Nyquist
// bins are ignored on the way back, as numpy's c2r does.  HBM: 8 N + 16 (M + 1) bytes per row either way.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/cosmoprimo_amd.h"
#include "cp_error.h"
#include "cp_fft_workgroup.h"
#include "cp_fftlog_tables.h"
#include "cp_internal.h"

namespace {

using namespace cpfft;

struct RArgs {
    const double* in;
    double* out;
    long long nrows;
    const cplx* tw;      // Plan<M, P> twiddles
    const cplx* rot;     // (M) e^{-2 pi i k / N}
    int conj_input;      // backward: transform conj(in) (the reference's engine convention)
};

template <int M, int P, bool BACKWARD>
__global__ __launch_bounds__(M / P) void rfft_kernel(const RArgs A) {
    using WG = WorkgroupFft<M, P>;
    constexpr int T = WG::T, N = 2 * M;
    extern __shared__ __attribute__((aligned(4096))) char rsmem[];
    cplx* lds = reinterpret_cast<cplx*>(rsmem);
    cplx* ltw = WG::twiddles(lds);
    const int t = threadIdx.x;
    for (int i = t; i < WG::TW_SLOTS; i += T) ltw[i] = A.tw[M + i];
    // A row with a sample that is not finite: left to the arithmetic, a NaN reaches every bin, but an infinity ends as +-Inf in a few (DC or
    // Nyquist of the forward transform, the samples that only additions reach on the way back).  The thread that meets such a sample raises the
    // row's flag before its first LDS store, the barriers of the transform publish it, and the row is stored as NaN.  Two flags taken in turn:
    // a row's flag is cleared ahead of the row's first barrier, when its last reader (two rows back) is behind the first barrier of the row between.
    // (ONE flag would not do: its readers sit behind the last barrier of the transform, with no barrier between them and the next row's clearing.)
    __shared__ int bad_row[2];
    const double nan = __builtin_nan("");
    int turn = 0;
    for (long long row = blockIdx.x; row < A.nrows; row += gridDim.x, turn ^= 1) {
        cplx x[P];
        if (t == 0) bad_row[turn] = 0;
        __syncthreads();      // LDS reuse across rows (and the table fill on the first one)
        bool bad = false;
        int tt = t;
        asm volatile("" : "+v"(tt));
        if constexpr (!BACKWARD) {
            const cplx* src = reinterpret_cast<const cplx*>(A.in + row * N);      // (x_2m, x_2m+1) is z_m
            cplx* dst = reinterpret_cast<cplx*>(A.out) + row * (M + 1);
#pragma unroll
            for (int r = 0; r < P; ++r) {
                x[r] = src[tt + T * r];
                bad |= not_finite(x[r].re) || not_finite(x[r].im);
            }
            if (bad) bad_row[turn] = 1;
            WG::forward(tt, A.tw, x, lds, ltw);
            asm volatile("" : "+v"(tt));
            const bool skip = bad_row[turn] != 0;
#pragma unroll 4
            for (int s = 0; s < P; ++s) {
                const int k = tt + T * s;
                const cplx v = lds[swz<M, P>(WG::pos_of_freq(k))];
                const cplx u = lds[swz<M, P>(WG::pos_of_freq((M - k) % M))];
                const cplx w = A.rot[k];
                const cplx e = cplx{0.5 * (v.re + u.re), 0.5 * (v.im - u.im)};
                const cplx o = cplx{0.5 * (v.im + u.im), 0.5 * (u.re - v.re)};
                cplx X = cplx{e.re + (w.re * o.re - w.im * o.im), e.im + (w.re * o.im + w.im * o.re)};
                if (k == 0) {      // real bins: DC here, Nyquist = E_0 - O_0 behind the last bin
                    X.im = 0.;
                    dst[M] = skip ? cplx{nan, nan} : cplx{e.re - o.re, 0.};
                }
                dst[k] = skip ? cplx{nan, nan} : X;
            }
        } else {
            const cplx* src = reinterpret_cast<const cplx*>(A.in) + row * (M + 1);
            cplx* dst = reinterpret_cast<cplx*>(A.out + row * N);
            const double sign = A.conj_input ? -1. : 1.;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                const int k = tt + T * r;
                cplx a = src[k], b = src[M - k];
                a.im *= sign;
                b.im *= sign;
                if (k == 0) a.im = b.im = 0.;      // DC and Nyquist count as real (numpy's c2r)
                bad |= not_finite(a.re) || not_finite(a.im) || (k == 0 && not_finite(b.re));
                const cplx w = A.rot[k];           // e^{-2 pi i k / N}: its conjugate is the factor of O_k
                const cplx e = cplx{0.5 * (a.re + b.re), 0.5 * (a.im - b.im)};
                const cplx d = cplx{0.5 * (a.re - b.re), 0.5 * (a.im + b.im)};
                const cplx o = cplx{d.re * w.re + d.im * w.im, d.im * w.re - d.re * w.im};
                // conj(Z_k) = conj(E_k + i O_k)
                x[r].re = e.re - o.im;
                x[r].im = -(e.im + o.re);
            }
            if (bad) bad_row[turn] = 1;
            WG::forward(tt, A.tw, x, lds, ltw);
            asm volatile("" : "+v"(tt));
            const bool skip = bad_row[turn] != 0;
            const double scale = 1. / M;
#pragma unroll 4
            for (int s = 0; s < P; ++s) {
                const int m = tt + T * s;
                const cplx g = lds[swz<M, P>(WG::pos_of_freq(m))];
                dst[m] = skip ? cplx{nan, nan} : cplx{g.re * scale, -g.im * scale};
            }
        }
    }
}

template <int M, int P>
void rlaunch(cp::Launches& on, bool backward, const RArgs& A, int grid) {
    constexpr int T = M / P, lds = WorkgroupFft<M, P>::lds_bytes();
    if (backward) on.run<rfft_kernel<M, P, true>>(grid, T, lds, A);
    else on.run<rfft_kernel<M, P, false>>(grid, T, lds, A);
}

// X(M, P): half sizes and points per thread
#define CP_RFFT_SIZES(X) X(4, 4) X(8, 8) X(16, 16) X(32, 16) X(64, 16) X(128, 16) X(256, 16) X(512, 16) X(1024, 16) X(2048, 16) X(4096, 16) X(8192, 16)

}  // namespace

struct cp_rfft_plan {
    int size, device;
    cp::DeviceArray<cplx> d_tw, d_rot;
};

extern "C" int cp_rfft_plan_destroy(cp_rfft_plan* p) { return cp::destroy_plan(p); }

extern "C" int cp_rfft_plan_create(cp_rfft_plan** out, int size, int device) {
    if (!out) return cp::fail(CP_EINVAL, "cp_rfft_plan_create: null plan pointer");
    *out = nullptr;
    if (size < 8 || size > 16384 || (size & (size - 1)))
        return cp::fail(CP_EUNSUPPORTED, "cp_rfft_plan_create: size %d (powers of two from 8 to 16384: the padded sizes FFTlog makes)", size);
    const int m = size / 2;
    std::vector<cplx> tw, rot(m);
#define X(M_, P_) \
    if (m == M_) build_twiddles<M_, P_>(tw);
    CP_RFFT_SIZES(X)
#undef X
    for (int k = 0; k < m; ++k) rot[k] = unit_root(k, size);
    cp::PlanPtr<cp_rfft_plan> p(new (std::nothrow) cp_rfft_plan());
    if (!p) return cp::fail(CP_ENOMEM, "cp_rfft_plan_create: host allocation failed");
    p->size = size; p->device = device;
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_rfft_plan_create: cannot select device %d", device);
    hipError_t e = p->d_tw.upload(tw.data(), tw.size());
    if (e == hipSuccess) e = p->d_rot.upload(rot.data(), m);
    if (e != hipSuccess) return cp::place_status("cp_rfft_plan_create", device, e);
    *out = p.release();
    return CP_OK;
}

static int rfft_run(const cp_rfft_plan* p, const double* d_in, double* d_out, long long nrows, bool backward, int conj_input, void* stream, const char* what) {
    if (!p) return cp::fail(CP_EINVAL, "%s: null plan", what);
    if (nrows < 0) return cp::fail(CP_EINVAL, "%s: negative row count", what);
    if (nrows == 0) return CP_OK;
    if (!d_in || !d_out) return cp::fail(CP_EINVAL, "%s: null device pointer", what);
    if (d_in == d_out) return cp::fail(CP_EINVAL, "%s: the transform is not in place", what);
    cp::DeviceScope scope(p->device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", what, p->device);
    RArgs A;
    A.in = d_in; A.out = d_out; A.nrows = nrows; A.tw = p->d_tw; A.rot = p->d_rot; A.conj_input = conj_input;
    const int m = p->size / 2;
    const int grid = (int)(nrows < 2048 ? nrows : 2048);
    cp::Launches on(what, stream);
#define X(M_, P_) \
    if (m == M_) rlaunch<M_, P_>(on, backward, A, grid);
    CP_RFFT_SIZES(X)
#undef X
    return on.status();
}

extern "C" int cp_rfft_forward(const cp_rfft_plan* p, const double* d_in, double* d_out, long long nrows, void* stream) {
    return rfft_run(p, d_in, d_out, nrows, false, 0, stream, "cp_rfft_forward");
}

extern "C" int cp_rfft_backward(const cp_rfft_plan* p, const double* d_in, double* d_out, long long nrows, int conj_input, void* stream) {
    return rfft_run(p, d_in, d_out, nrows, true, conj_input != 0, stream, "cp_rfft_backward");
}
