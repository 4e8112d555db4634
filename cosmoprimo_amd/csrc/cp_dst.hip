// cp_dst.hip -- batched orthonormal DST-II / DST-III of rows (gfx950) + C ABI.
//
// Replaces scipy.fftpack.dst / idst (type=2, norm='ortho') of the wallish2018 BAO filter
// (reference cosmoprimo/bao_filter.py:371-372, 412):
//   Y_k = f_k sum_n x_n sin(pi (k+1) (2n+1) / (2N)),  f_k = sqrt(2/N) (k < N-1), sqrt(1/N) (k = N-1);  inverse = transpose.
// With x'_n = (-1)^n x_n the DST-II is the DCT-II of x' read backwards (Y_k = f_k C'_{N-1-k}), and the DCT-II comes from ONE
// N-point complex FFT of the reordered sequence v_m = x'_{2m}, v_{N-1-m} = x'_{2m+1} (Makhoul 1980):
// C'_k = Re(e^{-i pi k / 2N} V_k).  Two real rows are packed as v_a + i v_b and separated after the FFT through
// V_a[k] = (V[k] + conj V[N-k]) / 2, V_b[k] = (V[k] - conj V[N-k]) / 2i.  The inverse runs the same network backwards:
// Hermitian-symmetrised spectra H = H_a + i H_b, v = conj(FFT(conj H)).
// The FFT is the workgroup transform of cp_fft_workgroup.h (the passes of the FFTLog kernel, cp_fft_core.h; cp_rfft.hip runs it too).  What the
// kernels of this file and of cp_wallish_tail.h do to a PAIR around it -- the split layout's index, the separation of the forward spectrum, the Hermitian
// packing of the inverse, a generated pair into the transform -- is written once, ahead of the kernels.  Optional fused elementwise maps for the filter:
// forward input log(k_n x_n), inverse output exp(y_n) / k_n.  HBM traffic: 16 N bytes per row (read + write), HBM-bound.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/cosmoprimo_amd.h"
#include "cp_error.h"
#include "cp_internal.h"
#include "cp_fft_workgroup.h"
#include "cp_fftlog_tables.h"
#include "cp_math.h"
#include "cp_power_eval.h"
#include "cp_wallish_dd.h"
#include "cp_splice_uniform.h"

namespace {

using namespace cpfft;

struct Args {
    const double* in;   // (nrows, N)
    double* out;        // (nrows, N)
    long long nrows;
    const cplx* tw;     // Plan twiddles
    const cplx* rot;    // (N) e^{-i pi k / (2N)} = (cos, -sin)
    const double* kx;   // (N) optional abscissa for the fused maps, or nullptr
    const double* ikx;  // (N) its reciprocals (the plan's table), or nullptr
    int fused;          // forward: x_n := log(kx_n * in_n); inverse: out_n := exp(y_n) / kx_n
    int split;          // coefficients stored de-interleaved: Y_0, Y_2, ... in the first half of the row, Y_1, Y_3, ... in the second
};

// Powers of two that bring a row whose largest sample has the high dword `top` (hi_abs) to the order of 1, and back: exact factors, so that the two
// rows of a pair meet in the complex FFT at the same magnitude whatever theirs are (2^-1022 .. 2^1022: subnormal and the very largest rows end within 2)
__device__ __forceinline__ void row_scale(unsigned top, double& to_unit, double& back) {
    int field = 2046 - (int)(top >> 20);      // bits 30..20: the biased exponent
    field = field < 1 ? 1 : (field > 2045 ? 2045 : field);
    to_unit = __builtin_bit_cast(double, (unsigned long long)field << 52);
    back = __builtin_bit_cast(double, (unsigned long long)(2046 - field) << 52);
}

// ... and then to a 2-norm in [1, 2): `sq` is the sum of the squares of the row's samples after row_scale, in units of 2^-40 (an integer sum: the same
// in whatever order the threads add to it, so that two launches on the same rows scale them alike).  The spectra of the two rows, which is where they
// meet, have the rows' 2-norms (the transform is orthonormal), not their largest samples: an impulse next to a constant row of the same height
// would otherwise meet a spectrum sqrt(N) times its own.  `to_unit` and `back` of row_scale are updated; `up` is applied before `back` on the way out.
__device__ __forceinline__ double square_2m40(double v) { return v * v * 0x1p40; }
__device__ __forceinline__ void norm_scale(unsigned long long sq, double& to_unit, double& up) {
    int k = sq ? ((63 - __builtin_clzll(sq)) - 40) >> 1 : 0;      // floor(log2(sum of squares) / 2)
    k = k < -64 ? -64 : (k > 64 ? 64 : k);
    to_unit *= __builtin_bit_cast(double, (unsigned long long)(1023 - k) << 52);      // exact: a power of two (subnormal ones included)
    up = __builtin_bit_cast(double, (unsigned long long)(1023 + k) << 52);
}

// ---- two real rows through one complex transform: the pieces the kernels below (and cp_wallish_tail.h) share ----
// position of coefficient j in its row: the wallish2018 filter treats even- and odd-indexed coefficients as two sequences (bao_filter.py:373), so they can
// be written / read as two half rows (split) instead of being gathered by separate copy kernels
template <int N>
__device__ __forceinline__ int split_at(int split, int j) {
    return split ? ((j & 1) * (N / 2) + (j >> 1)) : j;
}

// forward: frequencies k (v) and N - k (u) of the packed transform and rot = e^{-i pi k / 2N} = (cos, -sin) give coefficient N - 1 - k of either row, but for its
// norm f:  V_a = ((p + r)/2, (q - s)/2), V_b = ((q + s)/2, (r - p)/2);  C' = cos * re + sin * im
__device__ __forceinline__ double separated_a(cplx v, cplx u, cplx rot) { return 0.5 * (rot.re * (v.re + u.re) - rot.im * (v.im - u.im)); }
__device__ __forceinline__ double separated_b(cplx v, cplx u, cplx rot) { return 0.5 * (rot.re * (v.im + u.im) - rot.im * (u.re - v.re)); }

// inverse: the scaled coefficients N - 1 - k (A) and k - 1 (B) of a row and rot give frequency k >= 1 of its Hermitian-symmetrised spectrum (k = 0: A alone,
// real); the pair goes into the transform as conj(H_a + i H_b) (the transform runs forward)
__device__ __forceinline__ cplx hermitian_bin(double A, double B, cplx rot) {
    const double cs = rot.re, sn = -rot.im;
    return cplx{0.5 * (A * cs + B * sn), 0.5 * (A * sn - B * cs)};
}
__device__ __forceinline__ cplx conj_packed(cplx Ha, cplx Hb) { return cplx{Ha.re - Hb.im, -(Ha.im + Hb.re)}; }

// A pair that generate_row (below) has left in the thread's own slots (row a at 2 m, row b at 2 m + 1, m = t + T r in Makhoul order) into the
// transform's registers, the (-1)^n sign folded in.  A row with a sample that is not finite raises its flag; the barrier publishes the flags and lets every
// thread read its slots before the first pass overwrites the region.  The caller zeroes a flagged row in x (written there: behind a return of this function
// the join of that branch changed the order of the butterflies' operands).
template <int N, int P>
__device__ __forceinline__ void pack_generated_pair(int t, bool has_b, const double* slots, int* bad_row, cplx* x) {
    constexpr int T = N / P;
    bool bad_a = false, bad_b = false;
#pragma unroll
    for (int r = 0; r < P; ++r) {      // the thread's own slots: no barrier
        const int m = t + T * r;
        const bool lower = m < N / 2;
        const double a = slots[2 * m], b = has_b ? slots[2 * m + 1] : 0.;
        bad_a |= not_finite(a);
        bad_b |= not_finite(b);
        x[r].re = lower ? a : -a;
        x[r].im = lower ? b : -b;
    }
    if (bad_a) bad_row[0] = 1;
    if (bad_b) bad_row[1] = 1;
    __syncthreads();
}

#ifndef CP_DST_INVERSE_VIA_LDS      // inverse transform: 1 the rows are read once, in memory order, and handed to the threads through LDS; 0 every coefficient is read by
#define CP_DST_INVERSE_VIA_LDS 1    // two threads (one an iteration ahead, one in place)
#endif
#ifndef CP_DST_ABLATE      // diagnostic builds of the inverse transform (wrong results): 1 no fused map, 2 no in-place loads of the second half, 4 no stores, 8 no transform
#define CP_DST_ABLATE 0
#endif

template <int N, int P, bool INVERSE>
__global__ __launch_bounds__(N / P, 2) void dst_kernel(const Args A) {
    using WG = WorkgroupFft<N, P>;
    constexpr int T = WG::T;
    extern __shared__ __attribute__((aligned(4096))) char smem[];  // 4096: see LdsView (cp_fft_core.h)
    cplx* lds = reinterpret_cast<cplx*>(smem);
    cplx* ltw = WG::twiddles(lds);  // data slots of one packed pair, then the tables
    const int t = threadIdx.x;
    for (int i = t; i < WG::TW_SLOTS; i += T) ltw[i] = A.tw[N + i];
    const long long npairs = (A.nrows + 1) / 2;
    const double fn = sqrt(2. / N), fl = sqrt(1. / N);
    // Rows stay independent although two of them share one complex FFT (scipy transforms row by row): a row holding a sample that is
    // not finite -- or, for the fused log map, not positive -- goes into the transform as a harmless constant and is stored as NaN; its
    // partner is untouched.  The flags of the pair are raised by whichever thread meets such a sample and read behind one barrier.
    // The two rows share the FFT's multiplications, whose rounding is relative to the larger of the two spectra: each row goes in scaled by a power of
    // two and comes out scaled back, so that a row keeps its own accuracy whatever its partner (scipy transforms row by row).  Two stages, one LDS
    // reduction and one barrier each: first the row's largest sample to the order of 1 (row_top: the largest hi_abs, gathered with the flags; row_scale),
    // which makes the squares safe to sum, then its 2-norm -- the size of its spectrum -- to [1, 2) (row_sq, norm_scale).
    __shared__ int bad_row[2];
    __shared__ unsigned row_top[2];
    __shared__ unsigned long long row_sq[2];      // norm_scale
    __shared__ int pair_flag;   // inverse transform: some sample of the pair is not finite
    __shared__ cpmath::MathTables mt;      // the table-driven exponential of the fused inverse map (the barrier at the top of the first pair covers the fill)
    if (INVERSE) cpmath::fill_math_tables(&mt);
    const double nan = __builtin_nan("");
    // forward transform: the rows of the NEXT pair are fetched (in Makhoul order) while this pair is transformed -- the loads of a pair used to sit
    // at the top of its iteration, in front of everything that needs them, with two waves per SIMD to cover their latency
    double na[P], nb[P];
    auto fetch = [&](long long p) {
        const double* ra = A.in + 2 * p * N;
        const double* rb = 2 * p + 1 < A.nrows ? ra + N : ra;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int m = t + T * r;
            const int n = m < N / 2 ? 2 * m : 2 * (N - 1 - m) + 1;
            na[r] = ra[n];
            nb[r] = rb[n];
        }
    };
    // inverse transform: half of a pair's samples (the coefficients N - 1 - k of both rows) the same way; the other half (k - 1) are read in place
    auto at = [&](int j) { return split_at<N>(A.split, j); };      // position of coefficient j in its row
    auto fetch_inverse = [&](long long p) {
        const double* ra = A.in + 2 * p * N;
        const double* rb = 2 * p + 1 < A.nrows ? ra + N : ra;
#pragma unroll
        for (int r = 0; r < P; ++r) {
            // CP_DST_INVERSE_VIA_LDS: the rows as they lie in memory (every coefficient read ONCE; the threads pick what they need out of LDS)
            const int ia = CP_DST_INVERSE_VIA_LDS ? t + T * r : at(N - 1 - (t + T * r));
            na[r] = ra[ia];
            nb[r] = rb[ia];
        }
    };
    if ((long long)blockIdx.x < npairs) {
        if (INVERSE) fetch_inverse(blockIdx.x);
        else fetch(blockIdx.x);
    }
    for (long long p = blockIdx.x; p < npairs; p += gridDim.x) {
        const bool has_b = 2 * p + 1 < A.nrows;
        const double* ra = A.in + 2 * p * N;
        const double* rb = has_b ? ra + N : ra;
        double* oa = A.out + 2 * p * N;
        double* ob = has_b ? oa + N : oa;
        cplx x[P];
        if (t == 0) bad_row[0] = bad_row[1] = pair_flag = 0, row_top[0] = row_top[1] = 0u, row_sq[0] = row_sq[1] = 0ull;
        __syncthreads();  // LDS reuse across pairs (and the table fill on the first one)
        int tt = t;
        asm volatile("" : "+v"(tt));
        unsigned top_a = 0u, top_b = 0u;
        if constexpr (!INVERSE) {
            // Makhoul reordering with the (-1)^n sign folded in
            bool bad_a = false, bad_b = false;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                const int m = tt + T * r;
                const bool lower = m < N / 2;
                const int n = lower ? 2 * m : 2 * (N - 1 - m) + 1;
                double a = na[r], b = nb[r];
                bad_a |= not_finite(a) || (A.fused && !(a > 0.));
                bad_b |= not_finite(b) || (A.fused && !(b > 0.));
                if (A.fused) {
                    const double kk = A.kx[n];
                    a = cpmath::log_pos(kk * a);      // rows with a sample that is not positive are flagged above and left out
                    b = cpmath::log_pos(kk * b);
                }
                x[r].re = lower ? a : -a;
                x[r].im = has_b ? (lower ? b : -b) : 0.;
                top_a = max(top_a, hi_abs(a));
                top_b = max(top_b, hi_abs(b));
            }
            if (p + gridDim.x < npairs) fetch(p + gridDim.x);
            if (bad_a) bad_row[0] = 1;
            if (bad_b) bad_row[1] = 1;
            atomicMax(&row_top[0], top_a);
            atomicMax(&row_top[1], top_b);
            __syncthreads();
            const bool skip_a = bad_row[0] != 0, skip_b = bad_row[1] != 0;
            double sa, sb, back_a, back_b, up_a, up_b;
            row_scale(row_top[0], sa, back_a);
            row_scale(row_top[1], sb, back_b);
            unsigned long long sq_a = 0ull, sq_b = 0ull;
#pragma unroll
            for (int r = 0; r < P; ++r) {
                x[r].re = skip_a ? 0. : x[r].re * sa;
                x[r].im = skip_b ? 0. : x[r].im * sb;
                sq_a += (unsigned long long)square_2m40(x[r].re);
                sq_b += (unsigned long long)square_2m40(x[r].im);
            }
            atomicAdd(&row_sq[0], sq_a);
            atomicAdd(&row_sq[1], sq_b);
            __syncthreads();
            sa = sb = 1.;
            norm_scale(row_sq[0], sa, up_a);
            norm_scale(row_sq[1], sb, up_b);
#pragma unroll
            for (int r = 0; r < P; ++r) {
                x[r].re *= sa;
                x[r].im *= sb;
            }
            WG::forward(tt, A.tw, x, lds, ltw);
            asm volatile("" : "+v"(tt));
            // separate the two rows, rotate, scale; frequency k -> output index N - 1 - k
#pragma unroll 4
            for (int s = 0; s < P; ++s) {
                const int k = tt + T * s;
                const cplx v = WG::at(lds, WG::pos_of_freq(k));
                const cplx u = WG::at(lds, WG::pos_of_freq((N - k) % N));
                const cplx rot = A.rot[k];  // (cos, -sin)
                const double f = k == 0 ? fl : fn;
                const double ya = separated_a(v, u, rot), yb = separated_b(v, u, rot);
                oa[at(N - 1 - k)] = skip_a ? nan : f * ya * up_a * back_a;
                if (has_b) ob[at(N - 1 - k)] = skip_b ? nan : f * yb * up_b * back_b;
            }
        } else {
            // Hermitian-symmetrised, conjugated spectrum of the pair; a row that is skipped does not take part
            const double2* staged = reinterpret_cast<const double2*>(lds);      // (a, b) of the pair at their positions in memory (CP_DST_INVERSE_VIA_LDS)
            if (CP_DST_INVERSE_VIA_LDS) {
                double2* w = reinterpret_cast<double2*>(lds);
#pragma unroll
                for (int r = 0; r < P; ++r) w[tt + T * r] = double2{na[r], nb[r]};
            }
#pragma unroll
            for (int r = 0; r < P; ++r) {      // (every coefficient of the pair is in na / nb of exactly one thread, in either order of fetch_inverse)
                top_a = max(top_a, hi_abs(na[r]));
                top_b = max(top_b, hi_abs(nb[r]));
            }
            atomicMax(&row_top[0], top_a);
            atomicMax(&row_top[1], top_b);
            __syncthreads();
            double sa, sb, back_a, back_b, up_a, up_b;
            row_scale(row_top[0], sa, back_a);
            row_scale(row_top[1], sb, back_b);
            unsigned long long sq_a = 0ull, sq_b = 0ull;
#pragma unroll
            for (int r = 0; r < P; ++r) {      // (a row that is not finite adds anything at all: it is left out below, whatever its scale)
                const double va = na[r] * sa, vb = nb[r] * sb;
                sq_a += fabs(va) < 4. ? (unsigned long long)square_2m40(va) : 0ull;
                sq_b += fabs(vb) < 4. ? (unsigned long long)square_2m40(vb) : 0ull;
            }
            atomicAdd(&row_sq[0], sq_a);
            atomicAdd(&row_sq[1], sq_b);
            __syncthreads();
            norm_scale(row_sq[0], sa, up_a);
            norm_scale(row_sq[1], sb, up_b);
            auto spectrum = [&](bool keep_a, bool keep_b, bool prefetched) {
#pragma unroll
                for (int r = 0; r < P; ++r) {
                    const int k = tt + T * r;
                    const double fa = k == 0 ? fl : fn;                 // f_{N-1-k}
                    const double fb = (k == 0 || k == 1) ? (k == 0 ? fl : fn) : fn;   // f_{k-1} (k = 0 handled below)
                    const int ia = N - 1 - k, ib = k == 0 ? N - 1 : k - 1;
                    double Aa, Ab, Ba, Bb;
                    if (CP_DST_INVERSE_VIA_LDS && prefetched) {
                        const double2 va = staged[at(ia)], vb = staged[at(ib)];
                        Aa = fa * (va.x * sa); Ab = fa * (va.y * sb);
                        Ba = (k == 0 ? fa : fb) * (vb.x * sa); Bb = (k == 0 ? fa : fb) * (vb.y * sb);
                    } else {
                        Aa = fa * ((prefetched ? na[r] : ra[at(ia)]) * sa); Ab = fa * ((prefetched ? nb[r] : rb[at(ia)]) * sb);
                        Ba = (k == 0 ? fa : fb) * (((CP_DST_ABLATE & 2) ? na[r] : ra[at(ib)]) * sa); Bb = (k == 0 ? fa : fb) * (((CP_DST_ABLATE & 2) ? nb[r] : rb[at(ib)]) * sb);
                    }
                    const cplx rot = A.rot[k];
                    cplx Ha, Hb;
                    if (k == 0) {
                        Ha = cplx{Aa, 0.};
                        Hb = cplx{Ab, 0.};
                    } else {
                        Ha = hermitian_bin(Aa, Ba, rot);
                        Hb = hermitian_bin(Ab, Bb, rot);
                    }
                    if (!keep_a) Ha = cplx{0., 0.};
                    if (!keep_b) Hb = cplx{0., 0.};
                    x[r] = conj_packed(Ha, Hb);
                }
            };
            spectrum(true, has_b, true);
            if (p + gridDim.x < npairs) fetch_inverse(p + gridDim.x);
            // a sample that is not finite shows in the packed spectrum, though not which row it came from: the pair is flagged from the registers
            // (no second pass over the rows), and only a flagged pair -- rare -- reads its rows again to tell the two apart and leave the bad one out
            bool suspect = false;
#pragma unroll
            for (int r = 0; r < P; ++r) suspect |= not_finite(x[r].re) || not_finite(x[r].im);
            if (suspect) pair_flag = 1;
            __syncthreads();
            bool skip_a = false, skip_b = false;
            if (pair_flag) {     // uniform over the workgroup
                bool bad_a = false, bad_b = false;
                asm volatile("" : "+v"(tt));
#pragma unroll 1
                for (int r = 0; r < P; ++r) {
                    const int k = tt + T * r;
                    const int ia = N - 1 - k, ib = k == 0 ? N - 1 : k - 1;
                    bad_a |= not_finite(ra[at(ia)]) || not_finite(ra[at(ib)]);
                    bad_b |= not_finite(rb[at(ia)]) || not_finite(rb[at(ib)]);
                }
                if (bad_a) bad_row[0] = 1;
                if (bad_b) bad_row[1] = 1;
                __syncthreads();
                skip_a = bad_row[0] != 0;
                skip_b = bad_row[1] != 0;
                // finite rows whose sum overflowed in the packing stay as they are (skip_a = skip_b = false): nothing to separate
                if (skip_a | skip_b) spectrum(!skip_a, has_b && !skip_b, false);
            }
            if (!(CP_DST_ABLATE & 8)) WG::forward(tt, A.tw, x, lds, ltw);
            else {
                Pass<N, P, 0>::store_lds(tt, lds, x);
                __syncthreads();
            }
            asm volatile("" : "+v"(tt));
            // LDS holds (v_a[m], -v_b[m]) at pos(m); undo the reordering and the (-1)^n sign
#pragma unroll 4
            for (int s = 0; s < P; ++s) {
                const int n = tt + T * s;
                const bool even = (n & 1) == 0;
                const int m = even ? n / 2 : N - 1 - (n - 1) / 2;
                const cplx g = WG::at(lds, WG::pos_of_freq(m));
                double ya = (even ? g.re : -g.re) * up_a * back_a;
                double yb = (even ? -g.im : g.im) * up_b * back_b;
                if (A.fused && !(CP_DST_ABLATE & 1)) {
                    const double ik = A.ikx ? A.ikx[n] : cpmath::recip(A.kx[n]);
                    ya = cpmath::exp_tab(ya, &mt) * ik;
                    yb = cpmath::exp_tab(yb, &mt) * ik;
                }
                if ((CP_DST_ABLATE & 4) && ya != 12345.678) continue;
                oa[n] = skip_a ? nan : ya;
                if (has_b) ob[n] = skip_b ? nan : yb;
            }
        }
    }
}

// ---- forward transform of log(k P_c(k)) with the spectra of an analytic engine EVALUATED in the kernel (wallish2018 on a batch of cosmologies,
// bao_filter.py:371 behind eisenstein_hu.py:315-324): the evaluation (~400 fp64 instructions per sample, vector-ALU bound) and the transform
// (16 N bytes of LDS / HBM traffic per row, memory bound) were two launches with 4096 doubles per vector written and read between them; here a
// workgroup evaluates the 2 x 4096 samples of a pair of cosmologies straight into the transform's input (Makhoul order, (-1)^n folded in) and the
// chip sees both kinds of work at once, as in the fused sigma(r, z) kernel (cp_sigma.hip).  The arithmetic of a sample is power_kernel's
// CP_PK_LOG_K_MATTER (cp_power.hip), term by term, with k^1.08 and k^1.4 from tables next to log k (transfer_eh_powers) where power_kernel takes
// exponentials of the tabulated logarithm: the two agree to rounding (3e-16), not bit for bit.
struct GenArgs {
    Args dst;                        // out, tw, rot, split; in / kx / fused unused
    long long ncosmo;
    cpcosmo::Param bg[CP_BG_NPARAMS];
    cpcosmo::Param pw[CP_PK_NPARAMS];
    int second_is_omega_m;
    const double* ncdm_tab;          // massive neutrinos (cp_ncdm.tab; nsp == 0: none): today's densities only -- Omega0_m of pk_callable, Omega_m of BBKS
    int nsp;
    const double* k;                 // (N) wavenumbers, h/Mpc
    const double* ln_k;              // (N) their logarithms (log_pos, as power_kernel takes them)
    const cppower::CosmoConsts* consts;  // (ncosmo) the cosmologies' constants (cp_power_coefficients)
    // the next step of wallish2018 in the epilogue (bao_filter.py:373-405): second derivatives of the clamped splines through the even- and the
    // odd-indexed coefficients, the box between their maxima, the box rewritten -- box != null (split layout only)
    int* box;                        // (2 ncosmo, 2) or null
    int margin_first, margin_second, off0, off1;
};

#ifndef CP_DST_GEN_ILP
#define CP_DST_GEN_ILP 2
#endif
#ifndef CP_DST_GEN_PREFETCH
#define CP_DST_GEN_PREFETCH 1
#endif

// ln_k: (4, n) log k, k^1.08, k^1.4 (cp_power_eval.h), 1 / k; then (n, 4): (k, log k, k^1.08, k^1.4) of the sample the generating transform puts at
// position m of its reordered sequence (Makhoul's order: m < n / 2: sample 2 m, else 2 (n - 1 - m) + 1) -- a thread of generate_row walks m = t + T r:
// its four numbers are 32 contiguous bytes, a wave's 2 KB, where four tables indexed by the sample number took four scattered 8-byte loads and their addresses
__global__ void dst_log_kernel(const double* k, double* ln_k, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        cppower::powers_of_wavenumber(k[i], ln_k, i, n);
        ln_k[3 * n + i] = 1. / k[i];
        const int m = (i & 1) ? n - 1 - (i - 1) / 2 : i / 2;
        double* g = ln_k + 4 * (size_t)n + 4 * (size_t)m;
        g[0] = k[i];
        g[1] = ln_k[i];
        g[2] = ln_k[n + i];
        g[3] = ln_k[2 * n + i];
    }
}

// log(k P(k)) of cosmology ic at the thread's P samples m = t + T r of the reordered sequence, into the thread's own slots of the data region
// (double index 2 (t + T r) + row).  NOT unrolled: sixteen copies of a 400-instruction evaluation would not fit the instruction cache.
// GP: a pointer to the arguments -- const GenArgs* (a by-value kernel parameter: dst_generate_kernel), or GenArgsK: the kernel-argument segment itself, read
// through the constant address space where a value is used (wallish_full_kernel: its arguments held in scalar registers over the whole loop over pairs were
// ~800 v_readlane / v_writelane among the 9 300 vector instructions of a pair).  Everything is taken into locals that live as long as this function.
typedef const GenArgs __attribute__((address_space(4))) * GenArgsK;

template <int N, int P, int ENGINE, typename GP>
__device__ __forceinline__ void generate_row(GP G, long long ic, int t, double* slots, const cpmath::MathTables* mt) {
    using namespace cppower;
    constexpr int T = N / P;
    const CosmoConsts K = load_uniform(G->consts + ic);      // (scalar loads: the cosmology's constants in scalar registers)
    const PkPerCosmology& pc = K.pk;
    const double2* gen = reinterpret_cast<const double2*>(G->ln_k + 4 * (size_t)N);      // (k, log k), (k^1.08, k^1.4) of position m of the reordered sequence (dst_log_kernel)
    const double ln_pk_unit = K.ln_pk_unit;
    // CP_DST_GEN_ILP samples per iteration: independent chains of logarithms / exponentials / reciprocals for the two waves of a SIMD to interleave
    // ... whose table entries are requested an iteration ahead (CP_DST_GEN_PREFETCH: the loads of iteration r0 + ILP are in flight under the ~500
    // instructions of iteration r0; at the top of the iteration that uses them they sat in front of everything, with one other wave on the SIMD to cover them)
    double2 kl[CP_DST_GEN_ILP], pw[CP_DST_GEN_ILP];
#pragma unroll
    for (int u = 0; u < CP_DST_GEN_ILP; ++u) {
        kl[u] = gen[2 * (t + T * u)];
        pw[u] = gen[2 * (t + T * u) + 1];
    }
#pragma unroll 1
    for (int r0 = 0; r0 < P; r0 += CP_DST_GEN_ILP) {
        double2 kl_now[CP_DST_GEN_ILP], pw_now[CP_DST_GEN_ILP];
#pragma unroll
        for (int u = 0; u < CP_DST_GEN_ILP; ++u) {
            kl_now[u] = kl[u];
            pw_now[u] = pw[u];
            if (CP_DST_GEN_PREFETCH) {
                const int mn = t + T * ((r0 + CP_DST_GEN_ILP + u) & (P - 1));      // (the last iteration asks for the first entries again: never used)
                kl[u] = gen[2 * mn];
                pw[u] = gen[2 * mn + 1];
            } else if (r0 + CP_DST_GEN_ILP < P) {
                const int mn = t + T * (r0 + CP_DST_GEN_ILP + u);
                kl[u] = gen[2 * mn];
                pw[u] = gen[2 * mn + 1];
            }
        }
        if (!CP_DST_GEN_PREFETCH) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (measurements: the entries waited for where they are requested)
#pragma unroll
        for (int u = 0; u < CP_DST_GEN_ILP; ++u) {
            const int m = t + T * (r0 + u);
            const double kh = kl_now[u].x, ln_kh = kl_now[u].y;
            const double Tk = transfer_any<ENGINE>(K, kh, ln_kh, pw_now[u].x, pw_now[u].y, mt);
            slots[2 * m] = 2. * (ln_kh + (CP_MATH_TABLES_OFF ? log_pos(fabs(Tk)) : log_tab_any(fabs(Tk), mt))) + ln_pk_unit + primordial_tilt_exponent(pc, ln_kh);
        }
    }
}

template <int N, int P, int ENGINE>
__global__ __launch_bounds__(N / P, 2) void dst_generate_kernel(const GenArgs G) {
    using WG = WorkgroupFft<N, P>;
    constexpr int T = WG::T;
    const Args& A = G.dst;
    extern __shared__ __attribute__((aligned(4096))) char smem[];
    cplx* lds = reinterpret_cast<cplx*>(smem);
    cplx* ltw = WG::twiddles(lds);
    const int t = threadIdx.x;
    for (int i = t; i < WG::TW_SLOTS; i += T) ltw[i] = A.tw[N + i];
    double* dd_tabs = reinterpret_cast<double*>(ltw + WG::TW_SLOTS);      // 2 x DD_NTAB elimination factors of the box step (G.box only)
    if (G.box) cpdd::fill_tables(dd_tabs);
    const long long npairs = (G.ncosmo + 1) / 2;
    const double fn = sqrt(2. / N), fl = sqrt(1. / N);
    __shared__ int bad_row[2];
    __shared__ cpmath::MathTables mt;      // (the barrier at the top of the first pair covers it)
    cpmath::fill_math_tables(&mt);
    const double nan = __builtin_nan("");
    static_assert(!padded_lds(N, P), "the generated samples go through natural-order slots of the data region");
    for (long long p = blockIdx.x; p < npairs; p += gridDim.x) {
        const bool has_b = 2 * p + 1 < G.ncosmo;
        double* oa = A.out + 2 * p * N;
        double* ob = has_b ? oa + N : oa;
        if (t == 0) bad_row[0] = bad_row[1] = 0;
        __syncthreads();  // LDS reuse across pairs (and the table fill on the first one)
        double* slots = reinterpret_cast<double*>(lds);
        int tt = t;
        asm volatile("" : "+v"(tt));      // (nothing derived from the thread's number is kept in registers from one pair to the next: what the compiler hoists
                                           // out of this loop lives through the transform, in registers the kernel does not have -- spilled and reloaded)
        generate_row<N, P, ENGINE>(&G, 2 * p, tt, slots, cpmath::tables_present(&mt));
        if (has_b) generate_row<N, P, ENGINE>(&G, 2 * p + 1, tt, slots + 1, cpmath::tables_present(&mt));
        cplx x[P];
        pack_generated_pair<N, P>(tt, has_b, slots, bad_row, x);
        const bool skip_a = bad_row[0] != 0, skip_b = bad_row[1] != 0;
        if (skip_a | skip_b) {
#pragma unroll
            for (int r = 0; r < P; ++r) {
                if (skip_a) x[r].re = 0.;
                if (skip_b) x[r].im = 0.;
            }
        }
        asm volatile("" : "+v"(tt));
        WG::forward(tt, A.tw, x, lds, ltw);
        asm volatile("" : "+v"(tt));
        if (!G.box) {
#pragma unroll 4
            for (int s = 0; s < P; ++s) {
                const int k = tt + T * s;
                const cplx v = WG::at(lds, WG::pos_of_freq(k));
                const cplx u = WG::at(lds, WG::pos_of_freq((N - k) % N));
                const cplx rot = A.rot[k];
                const double f = k == 0 ? fl : fn;
                const double ya = separated_a(v, u, rot), yb = separated_b(v, u, rot);
                oa[split_at<N>(A.split, N - 1 - k)] = skip_a ? nan : f * ya;
                if (has_b) ob[split_at<N>(A.split, N - 1 - k)] = skip_b ? nan : f * yb;
            }
            continue;
        }
        // ---- the coefficients stay on the CU for the next step of the filter: the four sequences of the pair (even / odd coefficients of rows a, b),
        // one per wave, in the data region of the transform (4 x 2048 doubles, XOR layout) ----
        if constexpr (N == 4096) {
            using namespace cpdd;
            constexpr int S = 32, NS = N / 2;
            double va[P], vb[P];
#pragma unroll
            for (int s = 0; s < P; ++s) {
                const int k = tt + T * s;
                const cplx v = WG::at(lds, WG::pos_of_freq(k));
                const cplx u = WG::at(lds, WG::pos_of_freq((N - k) % N));
                const cplx rot = A.rot[k];
                const double f = k == 0 ? fl : fn;
                va[s] = skip_a ? nan : f * separated_a(v, u, rot);
                vb[s] = skip_b ? nan : f * separated_b(v, u, rot);
            }
            __syncthreads();      // every thread has its coefficients: the data region is free
            double* seqs = reinterpret_cast<double*>(lds);
#pragma unroll
            for (int s = 0; s < P; ++s) {
                const int j = N - 1 - (tt + T * s);      // coefficient j of its row: sequence (j & 1), knot j >> 1
                const int slot = Xor32Layout::at(j >> 1);
                seqs[(j & 1) * NS + slot] = va[s];
                seqs[(2 + (j & 1)) * NS + slot] = vb[s];
            }
            __syncthreads();
            int lane = tt;
            asm volatile("" : "+v"(lane));      // (nothing of the tail is hoisted out of the loop over pairs: 32 squared abscissae and 32 slots would live through the transform)
            const int wave = __builtin_amdgcn_readfirstlane(lane >> 6);
            lane &= 63;
            if (wave < 2 || has_b) {
                double* buf = seqs + wave * NS;
                const long long row = 2 * p + (wave >> 1);
                double* seq = A.out + row * N + (wave & 1) * NS;      // split layout: [even-indexed | odd-indexed] coefficients of the row
                double own[S];      // the wave's sequence, knot lane + 64 k in register k: the solve overwrites the buffer
#pragma unroll
                for (int k = 0; k < S; ++k) own[k] = buf[Xor32Layout::at(lane + 64 * k)];
                int first, second;
                second_derivatives_and_box<S, Xor32Layout>(buf, dd_tabs, lane, G.margin_first, G.margin_second, first, second);
                const long long srow = 2 * row + (wave & 1);
                if (lane == 0) {
                    G.box[2 * srow] = first + G.off0;
                    G.box[2 * srow + 1] = second + G.off1;
                }
                wave_lds_phase();      // the last reads of M are done: the buffer is free
                const int a = first + G.off0, b = second + G.off1;
                const bool removed = remove_box<S>(buf, dd_tabs + DD_NTAB, lane, a, b,
                                                   [&](int lo, int L, int R, int hi, double* zl, double* zr) {
#pragma unroll
                                                       for (int k = 0; k < S; ++k) {
                                                           const int i = lane + 64 * k;
                                                           const double x = (double)(i + 1);
                                                           if (i >= lo && i <= L) zl[i - lo] = own[k] * (x * x);
                                                           if (i >= R && i <= hi) zr[i - R] = own[k] * (x * x);
                                                       }
                                                   },
                                                   seq);
                // the knots that stay: every address of the sequence is written exactly once (the box by remove_box, the rest here)
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const int i = lane + 64 * k;
                    if (!(removed && i >= a && i <= b)) seq[i] = own[k];
                }
            }
        }
    }
}


#ifndef CP_TAIL_HEADER      // (measurements: another version of the kernel, tools/variants/, built beside the shipped library by tools/variant_lib.sh)
#define CP_TAIL_HEADER "cp_wallish_tail.h"
#endif
#include CP_TAIL_HEADER      // wallish_tail_kernel: everything of the filter behind its forward transform (cp_wallish_tail below)

template <int N>
void launch(cp::Launches& on, bool inverse, const Args& A, int grid) {
    constexpr int P = 16, T = N / P, lds = WorkgroupFft<N, P>::lds_bytes();
    if (inverse) on.run<dst_kernel<N, P, true>>(grid, T, lds, A);
    else on.run<dst_kernel<N, P, false>>(grid, T, lds, A);
}

}  // namespace

struct cp_dst_plan {
    int n, device;
    cp::DeviceArray<cplx> d_tw, d_rot;
    cp::DeviceArray<double> d_kx;
    cp::DeviceArray<double> d_ln_kx;      // log of the abscissa, filled at the first cp_dst_forward_analytic (device kernel: the bits of power_kernel's own logarithm)
};

extern "C" int cp_dst_plan_destroy(cp_dst_plan* p) { return cp::destroy_plan(p); }

extern "C" int cp_dst_plan_create(cp_dst_plan** out, int n, const double* kx, int device) {
    if (!out) return cp::fail(CP_EINVAL, "cp_dst_plan_create: null plan pointer");
    *out = nullptr;
    if (n != 256 && n != 1024 && n != 4096) return cp::fail(CP_EUNSUPPORTED, "cp_dst_plan_create: length %d not instantiated (256, 1024, 4096)", n);
    std::vector<cplx> tw, rot(n);
    if (n == 256) build_twiddles<256, 16>(tw);
    else if (n == 1024) build_twiddles<1024, 16>(tw);
    else build_twiddles<4096, 16>(tw);
    for (int k = 0; k < n; ++k) rot[k] = unit_root(k, 4LL * n);  // e^{-2 pi i k / 4N} = e^{-i pi k / 2N}
    cp::PlanPtr<cp_dst_plan> p(new (std::nothrow) cp_dst_plan());
    if (!p) return cp::fail(CP_ENOMEM, "cp_dst_plan_create: host allocation failed");
    p->n = n; p->device = device;
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_dst_plan_create: cannot select device %d", device);
    hipError_t e = p->d_tw.upload(tw.data(), tw.size());
    if (e == hipSuccess) e = p->d_rot.upload(rot.data(), n);
    if (e == hipSuccess && kx) e = p->d_kx.upload(kx, n);
    if (e == hipSuccess && kx) e = p->d_ln_kx.alloc(8 * (size_t)n);
    if (e != hipSuccess) return cp::place_status("cp_dst_plan_create", device, e);
    if (kx) {      // log of the abscissa with the kernels' own logarithm (default stream, then waited for: plan creation is synchronous)
        cp::Launches on("cp_dst_plan_create", nullptr);
        on.run<dst_log_kernel>((n + 255) / 256, 256, 0, p->d_kx.get(), p->d_ln_kx.get(), n);
        if (on.status() != CP_OK || hipDeviceSynchronize() != hipSuccess) return cp::fail(CP_EDEVICE, "cp_dst_plan_create: cannot tabulate log k");
    }
    *out = p.release();
    return CP_OK;
}

extern "C" int cp_dst_execute(const cp_dst_plan* p, const double* d_in, double* d_out, long long nrows, int inverse, int flags, void* stream) {
    if (flags & ~(CP_DST_FUSED | CP_DST_SPLIT)) return cp::fail(CP_EINVAL, "cp_dst_execute: unknown flags %d", flags);
    const int fused = flags & CP_DST_FUSED;
    if (!p) return cp::fail(CP_EINVAL, "cp_dst_execute: null plan");
    if (nrows < 0) return cp::fail(CP_EINVAL, "cp_dst_execute: negative row count");
    if (nrows == 0) return CP_OK;
    if (!d_in || !d_out) return cp::fail(CP_EINVAL, "cp_dst_execute: null device pointer");
    if (fused && !p->d_kx) return cp::fail(CP_EINVAL, "cp_dst_execute: the fused log / exp maps need the abscissa given at plan creation");
    cp::DeviceScope scope(p->device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_dst_execute: cannot select device %d", p->device);
    Args A;
    A.in = d_in; A.out = d_out; A.nrows = nrows; A.tw = p->d_tw; A.rot = p->d_rot; A.kx = p->d_kx; A.ikx = p->d_ln_kx ? p->d_ln_kx + 3 * (size_t)p->n : nullptr; A.fused = fused; A.split = (flags & CP_DST_SPLIT) != 0;
    const long long npairs = (nrows + 1) / 2;
    const int grid = (int)(npairs < 512 ? npairs : 512);
    cp::Launches on("cp_dst_execute", stream);
    if (p->n == 256) launch<256>(on, inverse != 0, A, grid);
    else if (p->n == 1024) launch<1024>(on, inverse != 0, A, grid);
    else launch<4096>(on, inverse != 0, A, grid);
    return on.status();
}

namespace {

// dst_generate_kernel, wallish_tail_kernel, wallish_full_kernel: the transform's LDS and the 2 x DD_NTAB elimination factors of the box step behind it
constexpr int WALLISH_LDS = WorkgroupFft<4096, 16>::lds_bytes(2 * cpdd::DD_NTAB * (int)sizeof(double));

}  // namespace

extern "C" long long cp_dst_forward_analytic_workspace_bytes(long long ncosmo) { return ncosmo < 0 ? -1 : cp::coef_workspace_bytes(ncosmo, 0); }

namespace {

bool bad_margins(int margin_first, int margin_second) { return margin_first < 0 || 2 * margin_first >= 2048 || margin_second < 0 || margin_second >= 2048; }

// two workgroups per CU are resident (LDS): every workgroup the same number of pairs
int wallish_grid(long long nrows, int device) { return cp::balanced_grid((nrows + 1) / 2, 2LL * cp::cu_count(device)); }

// The forward side of wallish2018 for a batch of analytic cosmologies (dst_generate_kernel, wallish_full_kernel): the transform's tables, the cosmology
// block, the plan's wavenumbers.  d_out null: the coefficients stay on the CU.
void fill_generate(GenArgs& G, const cp_dst_plan* p, long long ncosmo, const cp_param* bg_params, int second_is_omega_m, const cp_ncdm* ncdm, int nsp,
                   const cp_param* pk_params, double* d_out, bool split, const void* consts) {
    G.dst.in = nullptr; G.dst.out = d_out; G.dst.nrows = ncosmo; G.dst.tw = p->d_tw; G.dst.rot = p->d_rot; G.dst.kx = nullptr; G.dst.ikx = nullptr; G.dst.fused = 0;
    G.dst.split = split;
    cpcosmo::fill_cosmology(G, ncosmo, bg_params, pk_params, second_is_omega_m, ncdm, nsp, nullptr, consts);
    G.k = p->d_kx;
    G.ln_k = p->d_ln_kx;
}

// What cp_wallish_tail and cp_wallish_full ask of their plans (the splice plan's tables into *U); npk: the columns of P
int wallish_plans(const char* who, const cp_dst_plan* p, const cp_splice_plan* splice, int npk, cpsu::Tables* U) {
    if (p->n != 4096 || !p->d_kx || !p->d_ln_kx)
        return cp::fail(CP_EUNSUPPORTED, "%s: needs a transform plan of length 4096 made with its abscissa (wallish2018's linear grid)", who);
    int device = -1;
    if (!cp_splice_plan_uniform_view(splice, U, &device) || device != p->device)
        return cp::fail(CP_EUNSUPPORTED, "%s: the splice plan does not run the uniform-stretch scheme on the transform's device", who);
    // the stretch comes from the transformed rows, everything else from the rows of P; the stretch, the slot in front of it and the 64 S knots the
    // lanes own lie inside a row of the transform; one query per column of P
    if (U->src_u != 1 || (U->wl > 0 && U->src_l != 0) || (U->wr > 0 && U->src_r != 0) || U->col_u < 1 || U->col_u + 64 * U->S + 1 > 4096 || U->nq != npk ||
        U->ngb > cpsu::NGB || U->S != 49 || U->col_l + U->wl > npk || U->col_r + U->wr > npk)
        return cp::fail(CP_EUNSUPPORTED, "%s: the splice plan is not the filter's (stretch of %d knots at column %d of array %d, %d queries)", who, U->nm, U->col_u,
                        U->src_u, U->nq);
    return CP_OK;
}

// everything of wallish2018 behind its forward transform (wallish_tail_kernel, the tail of wallish_full_kernel)
void fill_tail(TailArgs& G, const cp_dst_plan* p, const cpsu::Tables& U, long long nrows, double* d_coef, const double* d_pk, int margin_first, int margin_second,
               int offset_first, int offset_second, const double* d_tophat, int* d_box, double* d_out) {
    G.nrows = nrows; G.coef = d_coef; G.tw = p->d_tw; G.rot = p->d_rot; G.ikx = p->d_ln_kx + 3 * (size_t)p->n;
    G.U = U;
    G.pk = d_pk; G.tophat = d_tophat; G.out = d_out; G.box = d_box;
    G.margin_first = margin_first; G.margin_second = margin_second; G.off0 = offset_first; G.off1 = offset_second;
}

int dst_forward_analytic(const cp_dst_plan* p, int engine, long long ncosmo, const cp_param* bg_params, int second_is_omega_m, const cp_ncdm* ncdm,
                         const cp_param* pk_params, double* d_out, void* d_work, int flags, int* d_box, int margin_first, int margin_second, int offset_first,
                         int offset_second, void* stream) {
    const char* who = "cp_dst_forward_analytic";
    if (!p) return cp::fail(CP_EINVAL, "cp_dst_forward_analytic: null plan");
    if (flags & ~CP_DST_SPLIT) return cp::fail(CP_EINVAL, "cp_dst_forward_analytic: unknown flags %d", flags);
    if (p->n != 4096 || !p->d_kx) return cp::fail(CP_EUNSUPPORTED, "cp_dst_forward_analytic: needs a plan of length 4096 made with its abscissa (wallish2018's linear grid)");
    if (!cpcosmo::engine_known(engine)) return cpcosmo::unknown_engine(who, engine);
    if (ncosmo < 0) return cp::fail(CP_EINVAL, "cp_dst_forward_analytic: negative batch");
    if (ncosmo == 0) return CP_OK;
    if (!bg_params || !pk_params || !d_out || !d_work) return cp::fail(CP_EINVAL, "cp_dst_forward_analytic: null pointer");
    int nsp;
    int st = cpcosmo::ncdm_species(ncdm, who, &nsp);
    if (st != CP_OK) return st;
    cp::DeviceScope scope(p->device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_dst_forward_analytic: cannot select device %d", p->device);
    const double* knots;
    st = cpcosmo::ncdm_knots(nsp, p->device, who, &knots);
    if (st != CP_OK) return st;
    char* coef = cp::coef_workspace(d_work, ncosmo).coef;
    cp::Launches on(who, stream);
    cp_power_coefficients(engine, ncosmo, bg_params, second_is_omega_m, ncdm, nsp, knots, pk_params, coef, on);
    GenArgs G{};
    fill_generate(G, p, ncosmo, bg_params, second_is_omega_m, ncdm, nsp, pk_params, d_out, (flags & CP_DST_SPLIT) != 0, coef);
    G.box = d_box; G.margin_first = margin_first; G.margin_second = margin_second; G.off0 = offset_first; G.off1 = offset_second;
    const int grid = wallish_grid(ncosmo, p->device);
    cpcosmo::dispatch_engine(engine, [&](auto e) { on.run<dst_generate_kernel<4096, 16, decltype(e)::value>>(grid, 4096 / 16, WALLISH_LDS, G); });
    return on.status();
}

}  // namespace

extern "C" int cp_dst_forward_analytic(const cp_dst_plan* p, int engine, long long ncosmo, const cp_param* bg_params, int second_is_omega_m,
                                       const cp_ncdm* ncdm, const cp_param* pk_params, double* d_out, void* d_work, int flags, void* stream) {
    return dst_forward_analytic(p, engine, ncosmo, bg_params, second_is_omega_m, ncdm, pk_params, d_out, d_work, flags, nullptr, 0, 0, 0, 0, stream);
}

extern "C" int cp_dst_forward_analytic_box(const cp_dst_plan* p, int engine, long long ncosmo, const cp_param* bg_params, int second_is_omega_m,
                                           const cp_ncdm* ncdm, const cp_param* pk_params, double* d_out, void* d_work, int* d_box, int margin_first, int margin_second,
                                           int offset_first, int offset_second, void* stream) {
    if (!d_box) return cp::fail(CP_EINVAL, "cp_dst_forward_analytic_box: null box pointer");
    if (bad_margins(margin_first, margin_second)) return cp::fail(CP_EINVAL, "cp_dst_forward_analytic_box: bad margins");
    return dst_forward_analytic(p, engine, ncosmo, bg_params, second_is_omega_m, ncdm, pk_params, d_out, d_work, CP_DST_SPLIT, d_box, margin_first, margin_second,
                                offset_first, offset_second, stream);
}

// ---- cp_wallish_tail: everything of wallish2018 behind its forward transform, one kernel (wallish_tail_kernel above) ----
extern "C" int cp_wallish_tail(const cp_dst_plan* p, const cp_splice_plan* splice, double* d_coef, const double* d_pk, int npk, long long nrows, int margin_first,
                               int margin_second, int offset_first, int offset_second, const double* d_tophat, int* d_box, double* d_out, void* stream) {
    if (!p || !splice) return cp::fail(CP_EINVAL, "cp_wallish_tail: null plan");
    if (nrows < 0) return cp::fail(CP_EINVAL, "cp_wallish_tail: negative batch");
    if (bad_margins(margin_first, margin_second)) return cp::fail(CP_EINVAL, "cp_wallish_tail: bad margins");
    cpsu::Tables U;
    const int st = wallish_plans("cp_wallish_tail", p, splice, npk, &U);
    if (st != CP_OK) return st;
    if (nrows == 0) return CP_OK;
    if (!d_coef || !d_pk || !d_box || !d_out) return cp::fail(CP_EINVAL, "cp_wallish_tail: null device pointer");
    cp::DeviceScope scope(p->device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_wallish_tail: cannot select device %d", p->device);
    TailArgs G{};
    fill_tail(G, p, U, nrows, d_coef, d_pk, margin_first, margin_second, offset_first, offset_second, d_tophat, d_box, d_out);
    cp::Launches on("cp_wallish_tail", stream);
    on.run<wallish_tail_kernel<49>>(wallish_grid(nrows, p->device), 256, WALLISH_LDS, G);
    return on.status();
}

// ---- cp_wallish_full: wallish2018 of a batch of analytic cosmologies, one kernel (wallish_full_kernel, cp_wallish_tail.h) ----
extern "C" int cp_wallish_full(const cp_dst_plan* p, const cp_splice_plan* splice, int engine, long long ncosmo, const cp_param* bg_params, int second_is_omega_m,
                               const cp_ncdm* ncdm, const cp_param* pk_params, const double* d_pk, int npk, int margin_first, int margin_second, int offset_first,
                               int offset_second, const double* d_tophat, int* d_box, double* d_coef, double* d_out, void* d_work, void* stream) {
    const char* who = "cp_wallish_full";
    if (!p || !splice) return cp::fail(CP_EINVAL, "cp_wallish_full: null plan");
    if (ncosmo < 0) return cp::fail(CP_EINVAL, "cp_wallish_full: negative batch");
    if (!cpcosmo::engine_known(engine)) return cpcosmo::unknown_engine(who, engine);
    if (bad_margins(margin_first, margin_second)) return cp::fail(CP_EINVAL, "cp_wallish_full: bad margins");
    cpsu::Tables U;
    int st = wallish_plans(who, p, splice, npk, &U);
    if (st != CP_OK) return st;
    if (ncosmo == 0) return CP_OK;
    if (!bg_params || !pk_params || !d_pk || !d_box || !d_out || !d_work) return cp::fail(CP_EINVAL, "cp_wallish_full: null pointer");
    int nsp;
    st = cpcosmo::ncdm_species(ncdm, who, &nsp);
    if (st != CP_OK) return st;
    cp::DeviceScope scope(p->device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_wallish_full: cannot select device %d", p->device);
    const double* knots;
    st = cpcosmo::ncdm_knots(nsp, p->device, who, &knots);
    if (st != CP_OK) return st;
    char* coef = cp::coef_workspace(d_work, ncosmo).coef;
    cp::Launches on(who, stream);
    cp_power_coefficients(engine, ncosmo, bg_params, second_is_omega_m, ncdm, nsp, knots, pk_params, coef, on);
    FullArgs F{};
    fill_tail(F.tail, p, U, ncosmo, d_coef, d_pk, margin_first, margin_second, offset_first, offset_second, d_tophat, d_box, d_out);
    fill_generate(F.gen, p, ncosmo, bg_params, second_is_omega_m, ncdm, nsp, pk_params, nullptr, true, coef);
    const int grid = wallish_grid(ncosmo, p->device);
    cpcosmo::dispatch_engine(engine, [&](auto e) { on.run<wallish_full_kernel<49, decltype(e)::value>>(grid, 256, WALLISH_LDS, F); });
    return on.status();
}
