// cp_fftlog_body.h -- the per-thread phases of the fused FFTLog kernel (device code for gfx950;
// also host-compilable for tests/host_emu, see cp_fft_core.h).
//
// One workgroup of T = NP/P threads transforms one *pair* of rows (z = a + i b) per iteration:
//   phase 0            : HBM -> registers (pad + extrapolate + x prefactor), DIF pass 0, -> LDS
//   phases 1..NPASS-2  : LDS -> DIF pass I -> LDS (in place)
//   phase NPASS-1      : LDS -> last DIF pass, x U (digit-reversed table), first DIT pass -> LDS
//   phases ..2NPASS-3  : LDS -> DIT pass I -> LDS
//   phase 2NPASS-2     : LDS -> DIT pass 0, x postfactor, crop, registers -> HBM
// Reference semantics: cosmoprimo/fftlog.py:198-241 (FFTlog.__call__) and :436-505 (pad).
#pragma once
#include <math.h>

#include "cp_fft_core.h"
#if defined(__HIPCC__)      // (the CPU emulation of the kernel's phases, tests/host_emu, compiles this header with g++: it takes the library's pow)
#include "cp_math.h"
#endif

namespace cpfft {

enum { CP_EXTRAP_CONST = 0, CP_EXTRAP_EDGE = 1, CP_EXTRAP_LOG = 2 };

// diagnostic switches (tools/mb_variants.sh); the library is built with the defaults
#ifndef CP_INTERPAIR_BARRIER
#define CP_INTERPAIR_BARRIER 0
#endif
// The four waves of a headline workgroup (NP = 4096, P = 16, zero padding) leave the barrier behind phase 0 together, do identical work and reach the CU's
// one LDS pipe together in the three barrier-free phases that follow.  CP_WAVE_SKEW > 0: behind that barrier wave w sleeps order[w] x CP_WAVE_SKEW x 64 cycles
// (s_sleep 1) before it issues its phase-1 reads; CP_WAVE_ORDER holds order[w] in hex digit w (0x3210: plain; 0x3120: waves 0, 2, 1, 3, i.e. SIMD order when
// the waves sit on SIMDs 0, 2, 1, 3).  Decides when a wave runs, never what it computes.  0: off, no code is emitted.  1 (64 / 128 / 192 cycles, plain order)
// measured best of 0 ... 12: -1.4 % on the headline, three times over (profiles/headline_wave_skew_ab.txt); 2-3 and 12 gain nothing, 7-9 about 1 %.
#ifndef CP_WAVE_SKEW
#define CP_WAVE_SKEW 1
#endif
#ifndef CP_WAVE_ORDER
#define CP_WAVE_ORDER 0x3210
#endif
#ifndef CP_WIDE_IO  // 1: 16-byte row loads / stores shared by lane pairs through DPP lane transposes; 0: one 8-byte access per sample
#define CP_WIDE_IO 0
#endif
// Row independence.  Two rows share one complex transform (z = a + i b), so without care a NaN / Inf in one row reaches its pair
// partner and rounding is relative to the larger row of the pair -- numpy's row-by-row FFTs (reference fftlog.py:538-544) do
// neither.  The kernel therefore finds, per row, the largest |sample| (its exponent field: 0 .. 2047, 2047 = Inf / NaN) and
//   * transforms a non-finite row as zeros and stores NaN for it (all of numpy's output for such a row is NaN as well);
//   * when the exponents of the two rows differ by more than CP_ROW_SCALE_SPREAD, scales each row by the power of two that
//     brings its largest sample to [1, 2) (exact), and scales the results back (exact): rounding becomes relative to the row's
//     own magnitude.  Within the spread nothing is done: the error is at most 2^spread times the row-relative one.
// Magnitudes are those of the TILTED samples a_j * pre_j (what the FFT sees; with 'log' extrapolation the raw padded samples of
// similar rows differ by orders of magnitude where the prefactor is tiny).  The zero-padded HALF variant takes them from the
// prefetch registers a pair ahead and reduces over the workgroup through the barrier that precedes the last phase (no extra
// barrier); the other variants reduce inside phase 0 (one extra barrier per pair).
#ifndef CP_ROW_SCREEN
#define CP_ROW_SCREEN 1
#endif
#ifndef CP_ROW_SCALE_SPREAD
#define CP_ROW_SCALE_SPREAD 4
#endif
#ifndef CP_SCREEN_SUM  // 1: a thread's magnitude is the exponent of the sum of its |samples| instead of their maximum
#define CP_SCREEN_SUM 0
#endif
// The first CP_PIN_TW0 pass-0 twiddles of a thread stay in registers for the whole launch (HALF variants at NP = 4096 only): they are the same
// for every pair, the kernel uses 225-238 of the 256 registers two waves per SIMD leave it, and every table load taken out pays (measured on
// 100 000 x 2048, nt rows: 0 -> 0.972 ms, 3 -> 0.965, 6 -> 0.958, 7 -> 0.951, 8 -> 0.953 with all 256 registers taken).
#ifndef CP_PIN_TW0
#define CP_PIN_TW0 7
#endif
#ifndef CP_EARLY_TW1
#define CP_EARLY_TW1 1
#endif

// Input front ends (how phase 0 pads the row):
//   IN_GENERIC   any n / NP, constant or edge padding: clamped (always valid) loads + selects, branch-free
//   IN_LOG       IN_GENERIC plus 'log' extrapolation (a pow() per padded element)
//   IN_HALF      n == NP/2 and P in {8, 16}: the row occupies exactly r in [P/4, 3P/4) of every thread's P
//                points (in_left = NP/4 = (P/4) T, fftlog.py:149-153 with minfolds=2 and n a power of two);
//                constant or edge padding
//   IN_HALF_ZERO IN_HALF with zero padding (the reference default extrap=0): padded points are never formed
//   IN_HALF_ZERO_GEN  IN_HALF_ZERO for a kernel that PRODUCES its rows itself (cp_sigma.hip evaluates P(k) into the row registers in front of
//                phase 0): nothing is prefetched from memory, the rows are screened inside phase 0
// Output back ends:
//   OUT_GENERIC  bounds-checked crop (any out_off / n_out, incl. keep_padding)
//   OUT_HALF     n == NP/2, cropped output: exactly s in [P/4, 3P/4) (out_left = NP/4)
//   OUT_HALF_WINDOW  OUT_HALF that stores the output columns [out_first, out_last) only (a consumer that reads a part of every row: the
//                step from the FFTLog grid to 256 radii of sigma(r, z) reads a third of it -- the rest never has to reach HBM)
enum { IN_GENERIC = 0, IN_LOG = 1, IN_HALF = 2, IN_HALF_ZERO = 3, IN_HALF_ZERO_GEN = 4 };
enum { OUT_GENERIC = 0, OUT_HALF = 1, OUT_HALF_WINDOW = 2 };

struct FftlogArgs {
    const double* in;   // (nbatch, nker, n) row-major
    double* out;        // (nbatch, nker, n_out)
    long long nbatch;   // batch items; each holds nker rows
    int nker;           // transforms "in parallel" (reference FFTlog.nparallel)
    int n;              // input row length
    int in_left;        // left padding of the input (fftlog.py:152)
    int out_off;        // first padded output index kept (fftlog.py:235), 0 when keep_padding
    int n_out;          // output row length (n or NP)
    int ext_l, ext_r;   // CP_EXTRAP_*
    double val_l, val_r;
    int stream_rows;    // bit 0: the rows are read, bit 1: written with the non-temporal cache policy (3: launches larger than the Infinity Cache)
    const double* pre;  // (nker, NP) padded prefactor
    const double* post; // (nker, NP) padded postfactor
    const cplx* u;      // (nker, NP) Hermitian-extended u / NP in thread layout [(i R + s) T + t]
    const cplx* tw;     // concatenated per-pass twiddles, Plan::tw_offset
    int out_first, out_last;  // OUT_HALF_WINDOW only: the columns of an output row that are stored
    unsigned* cu_ticket;  // one arrival counter per CU (CP_CU_SLOTS entries, never reset: cp_fftlog_kernel.h, balances_cu)
#if defined(CP_STAMPS)
    double* val_stamp;  // diagnostic builds: per-wave cycle sums
    unsigned long long* bar_log;  // per workgroup: CU identity, start clock, two barrier clocks per pair (null: not recorded)
    int bar_log_pairs;            // pairs per workgroup the log has room for
#endif
};

template <int NP, int P, int IN_MODE = IN_LOG, int OUT_MODE = OUT_GENERIC>
struct Fftlog {
    using PL = Plan<NP, P>;
    static constexpr int T = PL::T;
    static constexpr int NPASS = PL::NPASS;
    static constexpr int NPH = 2 * NPASS - 1;  // phases separated by workgroup barriers
    static constexpr int LAST = NPASS - 1;
    // phase 1 is a middle DIF phase with LDS twiddles (NPASS >= 3) whose table reads can be issued in phase 0
    static constexpr bool EARLY_TW1 = CP_EARLY_TW1 && NPASS >= 3 && CP_ABLATE == 0;
    static constexpr bool HALF_IN = IN_MODE == IN_HALF || IN_MODE == IN_HALF_ZERO || IN_MODE == IN_HALF_ZERO_GEN;
    static constexpr bool ZERO_PADDED_IN = IN_MODE == IN_HALF_ZERO || IN_MODE == IN_HALF_ZERO_GEN;
    static constexpr bool ROWS_FROM_MEMORY = IN_MODE != IN_HALF_ZERO_GEN;
    // pass-0 twiddles s = 1 .. KPIN of the thread are loaded once per launch (State::wpin) instead of once per pair
    static constexpr int KPIN = (HALF_IN && NP == 4096 && P == 16 && CP_ABLATE == 0) ? CP_PIN_TW0 : 0;
    // LDS: the data slots of one packed pair (NP, or more for a padded layout), then the twiddle tables of passes >= 1
    // (Plan::tw_offset order)
    static constexpr int LDS_DATA = lds_data_slots(NP, P);
    static constexpr int LDS_TW_ENTRIES = NPASS > 1 ? PL::TW_TOTAL - NP : 0;
    // ... then the scratch of the row screening: one (max a, max b) pair of unsigned per wave
    // (full waves: one slot per wave, filled after a DPP reduction; workgroups smaller than a wave: one slot per thread -- lane
    // operations must not read the inactive lanes of a partial wave)
    static constexpr int SCR_SLOTS = T >= 64 ? T / 64 : T;
    static constexpr int LDS_SCR_BYTES = ((SCR_SLOTS * 8 + 15) / 16) * 16;
    static constexpr int LDS_BYTES = NPASS > 1 ? (LDS_DATA + LDS_TW_ENTRIES) * (int)sizeof(cplx) + LDS_SCR_BYTES : 0;
    static CP_HD unsigned* lds_scr(cplx* lds) { return reinterpret_cast<unsigned*>(lds + LDS_DATA + LDS_TW_ENTRIES); }
    static constexpr bool SCREEN = CP_ROW_SCREEN && CP_ABLATE == 0;
    // the zero-padded HALF variant (the reference's default extrap=0) screens a pair ahead, from the prefetch registers
    static constexpr bool SCREEN_AHEAD = SCREEN && IN_MODE == 3 /* IN_HALF_ZERO */ && !CP_WIDE_IO;
#if defined(__HIP_DEVICE_COMPILE__)
    static constexpr bool SCREEN_AHEAD_DEVICE = SCREEN_AHEAD;
#else
    static constexpr bool SCREEN_AHEAD_DEVICE = false;  // the host emulation screens in phase 0
#endif
    // Which pass-0 butterfly (j = the low 8 bits of its elements' indices) thread t takes.  Identity except under the padded LDS
    // layout, where the lanes of each half wave are permuted so that the 16 lanes ds_read_b128 serves together (lane groups
    // {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}: MI355X_MICROARCH.md) all hold the same middle digit: slot = lo + 17 mid + 272 hi
    // is then conflict-free for the pass-0 shape as well (tools/lds_conflict_model.py).  A wave still covers the same 64
    // consecutive samples of a row, so the HBM access pattern is unchanged.
    static CP_HD int pass0_thread(int t) {
        if constexpr (padded_lds(NP, P) && !CP_WIDE_IO) {
            constexpr unsigned char perm32[32] = {0,  1,  2,  3,  19, 20, 21, 22, 23, 24, 25, 26, 4,  5,  6,  7,
                                                  27, 28, 29, 30, 8,  9,  10, 11, 12, 13, 14, 15, 31, 16, 17, 18};
            return (t & ~31) + perm32[t & 31];
        }
        return t;
    }
    // pass whose butterflies phase PH ends with (the shape of its LDS writes) / starts with (the shape of its LDS reads)
    static constexpr int write_pass(int ph) { return ph <= LAST ? ph : NPH - 1 - ph; }
    static constexpr int read_pass(int ph) { return ph < LAST ? ph : NPH - 1 - ph; }
    // no workgroup barrier is needed between phases PH and PH + 1 when that exchange stays inside single waves
    template <int PH>
    static constexpr bool barrier_free_after() {
        if constexpr (NPASS > 1 && PH + 1 < NPH) {
            // the barrier in front of the last phase also publishes the screening scratch of the next pair (HALF variants)
            if (SCREEN_AHEAD && PH == NPH - 2 && T > 64) return false;
            return exchange_is_wave_local<NP, P>(write_pass(PH), read_pass(PH + 1));
        }
        return false;
    }
    template <int I>
    static CP_HD const cplx* lds_tw(const cplx* lds) {
        return lds + LDS_DATA + (PL::tw_offset(I) - NP);
    }
    static constexpr bool HALF_OUT = OUT_MODE == OUT_HALF || OUT_MODE == OUT_HALF_WINDOW;
    static_assert((!HALF_IN && !HALF_OUT) || ((P == 16 || P == 8) && NPASS > 1), "HALF modes need P in {8, 16} and NP > P");
    // HALF modes: the row occupies points r in [Q, Q + H) of every thread's P (Q = P/4 padded points on either side)
    static constexpr int H = P / 2, Q = P / 4;

    // padded input element j of one row (reference pad(): fftlog.py:483-505); branch-free for constant / edge
    // ratio^e of the log-log continuation of a row beyond its ends (fftlog.py:486-501): the ratio of two neighbouring samples, a whole exponent of at most the
    // padding.  For a positive, normal ratio and |e log ratio| < 700 it is exp(e log(ratio)) with the package's own logarithm and exponential (cp_math.h: both
    // below 1 ulp; the product carries |e log ratio| ulp, 1e-15 for the 8 of a thousand steps of a 0.8 % ratio) -- 45 instructions where the library's pow
    // takes ~150 and the padded half of a log-extrapolated row was two thirds of its transform's time; anything else (zero, negative, Inf, NaN, overflow) is
    // the library's.
    static CP_HD __attribute__((noinline)) double ratio_pow(double ratio, int e) {      // (a call, like pow: 32 copies per thread cost registers the kernel does not have)
#if defined(__HIP_DEVICE_COMPILE__)
        if (ratio > 2.2250738585072014e-308 && ratio < 1.7976931348623157e308) {
            const double x = (double)e * cpmath::log_pos(ratio);
            if (fabs(x) < 700.) return cpmath::exp_mid(x);
        }
#endif
        return pow(ratio, (double)e);
    }

    // The same per ROW instead of per point: log(a_1 / a_0) and log(a_{n-2} / a_{n-1}) once per thread and row (load_input), a padded point is then its end value
    // times one exponential.  ok_* false: an end ratio that is not positive and normal (or no log extrapolation on that side) -- those points take fetch().
    struct LogEnds {
        double ln_l, ln_r;
        bool ok_l, ok_r;
    };
    static CP_HD LogEnds log_ends(const double* __restrict__ a, const FftlogArgs& A) {
        LogEnds E{0., 0., false, false};
#if defined(__HIP_DEVICE_COMPILE__)
        if (IN_MODE == IN_LOG && A.n >= 2) {
            const double rl = a[1] / a[0], rr = a[A.n - 2] / a[A.n - 1];
            E.ok_l = A.ext_l == CP_EXTRAP_LOG && rl > 2.2250738585072014e-308 && rl < 1.7976931348623157e308;
            E.ok_r = A.ext_r == CP_EXTRAP_LOG && rr > 2.2250738585072014e-308 && rr < 1.7976931348623157e308;
            E.ln_l = E.ok_l ? log_call(rl) : 0.;
            E.ln_r = E.ok_r ? log_call(rr) : 0.;
        }
#endif
        return E;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __attribute__((noinline)) double log_call(double x) { return cpmath::log_pos(x); }
    static __device__ __attribute__((noinline)) double exp_call(double x) { return cpmath::exp_mid(x); }
#endif
    static CP_HD double fetch_log(const double* __restrict__ a, int j, const FftlogArgs& A, const LogEnds& E) {
#if defined(__HIP_DEVICE_COMPILE__)
        const int idx = j - A.in_left;
        if (idx < 0 && E.ok_l) {
            const double x = (double)idx * E.ln_l;
            if (fabs(x) < 700.) return a[0] * exp_call(x);
        } else if (idx >= A.n && E.ok_r) {
            const double x = -(double)(idx - A.n + 1) * E.ln_r;
            if (fabs(x) < 700.) return a[A.n - 1] * exp_call(x);
        }
#endif
        return fetch(a, j, A);
    }

    static CP_HD double fetch(const double* __restrict__ a, int j, const FftlogArgs& A) {
        const int idx = j - A.in_left;
        const int cl = idx < 0 ? 0 : (idx >= A.n ? A.n - 1 : idx);
        double v = a[cl];  // in range: the sample; out of range: the edge value
        if (idx < 0) {
            if (A.ext_l == CP_EXTRAP_CONST) v = A.val_l;
            if (IN_MODE == IN_LOG && A.ext_l == CP_EXTRAP_LOG) v = v * ratio_pow(a[1] / v, idx);
        } else if (idx >= A.n) {
            if (A.ext_r == CP_EXTRAP_CONST) v = A.val_r;
            if (IN_MODE == IN_LOG && A.ext_r == CP_EXTRAP_LOG) v = v / ratio_pow(a[A.n - 2] / v, idx - A.n + 1);
        }
        return v;
    }

    // ---- row screening (see CP_ROW_SCREEN above) -------------------------------------------------------------------------
    // info = magnitude field of row a | magnitude field of row b << 16.  The field is the exponent field of the row's largest |tilted sample|, with two
    // amendments: 0 is kept for a row that IS zero, and a row whose largest sample is subnormal counts as exponent field 1 (tiny_to_one, make_info).
    struct RowFix {
        int any, nan_a, nan_b, sh_a, sh_b;  // sh: power of two applied to the row on the way in (0: none), undone on the way out
    };
    // A row of zeros beside a live partner: its half of the packed transform holds the rounding of the partner's, where numpy's row-by-row
    // transform gives exactly 0.  It takes the "shift" CP_ZERO_ROW_SHIFT, beyond the whole range of the format: ldexp leaves its zeros as
    // they are on the way in and takes whatever finite values came out to (signed) zero on the way out -- no further case in the fix-ups.
    static constexpr int CP_ZERO_ROW_SHIFT = 4096;
    static CP_HD RowFix decode_info(unsigned info) {
        const int ea = (int)(info & 0xffffu), eb = (int)(info >> 16);
        RowFix f;
        f.nan_a = ea == 2047;
        f.nan_b = eb == 2047;
        const int d = ea - eb;
        // (a subnormal row has field 1: beside a distant partner it comes up by 2^1022, exactly, and goes back down with one rounding)
        const int scale = !f.nan_a && !f.nan_b && ea != 0 && eb != 0 && (d > CP_ROW_SCALE_SPREAD || d < -CP_ROW_SCALE_SPREAD);
        f.sh_a = scale ? 1023 - ea : 0;
        f.sh_b = scale ? 1023 - eb : 0;
        const int zero_a = ea == 0 && eb != 0, zero_b = eb == 0 && ea != 0;
        if (zero_a) f.sh_a = CP_ZERO_ROW_SHIFT;
        if (zero_b) f.sh_b = CP_ZERO_ROW_SHIFT;
        f.any = f.nan_a | f.nan_b | scale | zero_a | zero_b;
        return f;
    }
    // hi_abs of a sample (or of a sum of |samples|) that is not zero but has an empty high dword (below 2^-1042) counts as 1
    static CP_HD unsigned tiny_to_one(unsigned h, double v) { return (h == 0u && v != 0.) ? 1u : h; }
    static CP_HD unsigned field(unsigned m) { return (m >> 20) | (unsigned)(m != 0u && m < (1u << 20)); }
    static CP_HD unsigned make_info(unsigned ma, unsigned mb) { return field(ma) | (field(mb) << 16); }
    // The verdict is decoded once per pair: `gate` maps every info word that asks for nothing to 0, and the fix-ups test that word only.
    static CP_HD unsigned gate(unsigned info) { return decode_info(info).any ? info : 0u; }
    template <int N>
    static CP_HD void fix_input(unsigned gated, cplx* x) {
        if (gated == 0u) return;  // wave-uniform on the device
        const RowFix f = decode_info(gated);
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (f.nan_a) x[r].re = 0.;
            else if (f.sh_a) x[r].re = ldexp(x[r].re, f.sh_a);
            if (f.nan_b) x[r].im = 0.;
            else if (f.sh_b) x[r].im = ldexp(x[r].im, f.sh_b);
        }
    }
    template <int N>
    static CP_HD void fix_output(unsigned gated, double* ya, double* yb) {
        if (gated == 0u) return;
        const RowFix f = decode_info(gated);
#pragma unroll
        for (int s = 0; s < N; ++s) {
            if (f.nan_a) ya[s] = __builtin_nan("");
            else if (f.sh_a) ya[s] = ldexp(ya[s], -f.sh_a);
            if (f.nan_b) yb[s] = __builtin_nan("");
            else if (f.sh_b) yb[s] = ldexp(yb[s], -f.sh_b);
        }
    }
    template <int N>
    static CP_HD void thread_max(const double* a, const double* b, unsigned& ma, unsigned& mb) {
#if CP_SCREEN_SUM
        // magnitude of the thread's samples as the exponent of sum |a_r| (between the largest sample and N times it; NaN / Inf
        // propagate): N fp64 additions with the absolute value as an operand modifier, instead of 2 N integer operations
        double sa = 0., sb = 0.;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            sa += __builtin_fabs(a[r]);
            sb += __builtin_fabs(b[r]);
        }
        const unsigned ha = tiny_to_one(hi_abs(sa), sa), hb = tiny_to_one(hi_abs(sb), sb);
        ma = ma > ha ? ma : ha;
        mb = mb > hb ? mb : hb;
        return;
#endif
#pragma unroll
        for (int r = 0; r < N; ++r) {
            const unsigned ha = hi_abs(a[r]), hb = hi_abs(b[r]);
            ma = ma > ha ? ma : ha;
            mb = mb > hb ? mb : hb;
        }
        if (ma == 0u || mb == 0u) {  // rare: every high dword of a row empty -- zero throughout, or samples below 2^-1042?
#pragma unroll
            for (int r = 0; r < N; ++r) {
                ma = tiny_to_one(ma, a[r]);
                mb = tiny_to_one(mb, b[r]);
            }
        }
    }
    template <int N>
    static CP_HD void thread_max(const cplx* x, unsigned& ma, unsigned& mb) {
#pragma unroll
        for (int r = 0; r < N; ++r) {
            const unsigned ha = hi_abs(x[r].re), hb = hi_abs(x[r].im);
            ma = ma > ha ? ma : ha;
            mb = mb > hb ? mb : hb;
        }
        if (ma == 0u || mb == 0u) {  // rare, as above
#pragma unroll
            for (int r = 0; r < N; ++r) {
                ma = tiny_to_one(ma, x[r].re);
                mb = tiny_to_one(mb, x[r].im);
            }
        }
    }
    // phase 0 of the variants that do not screen ahead: the thread's tilted points x[0..N) -> reduction over the workgroup (one
    // barrier) -> the pair's exponent fields in `info`, fix-up applied.  Host emulation: magnitudes straight from the rows.
    template <int N>
    static CP_HD void screen_in_phase0(int t, const FftlogArgs& A, const double* ra, const double* rb, const double* pre, cplx* lds, unsigned& info,
                                       cplx* x) {
#if defined(__HIP_DEVICE_COMPILE__)
        unsigned ma = 0, mb = 0;
        thread_max<N>(x, ma, mb);
        if constexpr (T > 1) {
            screen_publish(t, lds, ma, mb);
            __syncthreads();
            info = screen_collect(lds);
        } else {
            info = make_info(ma, mb);
        }
#else
        info = host_row_info(ra, rb, pre, A);
#endif
        info = gate(info);
        fix_input<N>(info, x);
    }
#if defined(__HIP_DEVICE_COMPILE__)
    // workgroup reduction of the per-thread maxima: wave maximum by DPP, one 8-byte LDS slot per wave, published by the next
    // workgroup barrier (or by the in-order LDS of a single-wave workgroup), collected by every thread
    static __device__ __forceinline__ void screen_publish(int t, cplx* lds, unsigned ma, unsigned mb) {
        if constexpr (T >= 64) {
            wave_max2_u32(ma, mb);
            if ((t & 63) == 63) {      // the lane that holds the wave maxima
                unsigned* scr = lds_scr(lds) + 2 * (t >> 6);
                scr[0] = ma;
                scr[1] = mb;
            }
        } else {
            unsigned* scr = lds_scr(lds) + 2 * t;
            scr[0] = ma;
            scr[1] = mb;
        }
    }
    static __device__ __forceinline__ unsigned screen_collect(cplx* lds) {
        const unsigned* scr = lds_scr(lds);
        unsigned ma = 0, mb = 0;
#pragma unroll
        for (int w = 0; w < SCR_SLOTS; ++w) {
            ma = ma > scr[2 * w] ? ma : scr[2 * w];
            mb = mb > scr[2 * w + 1] ? mb : scr[2 * w + 1];
        }
        return (unsigned)__builtin_amdgcn_readfirstlane((int)make_info(ma, mb));
    }
#else
    // host pass of the kernel source / host emulation: never called (the emulation takes the magnitudes from the rows)
    static void screen_publish(int, cplx*, unsigned, unsigned) {}
    static unsigned screen_collect(cplx*) { return 0u; }
#endif
    // host emulation: the magnitudes straight from the rows (the emulated threads run one after the other)
    static CP_HD unsigned host_row_info(const double* __restrict__ ra, const double* __restrict__ rb, const double* __restrict__ pre,
                                        const FftlogArgs& A) {
        unsigned ma = 0, mb = 0;
        for (int j = 0; j < NP; ++j) {
            const double va = fetch(ra, j, A) * pre[j], vb = fetch(rb, j, A) * pre[j];
            const unsigned ha = tiny_to_one(hi_abs(va), va), hb = tiny_to_one(hi_abs(vb), vb);
            ma = ma > ha ? ma : ha;
            mb = mb > hb ? mb : hb;
        }
        return make_info(ma, mb);
    }

    // HALF front end, split in two so the HBM loads of the NEXT pair are issued a whole pair ahead
    // (prefetch registers va / vb live across the phases): issue ...
    static CP_HD void prefetch_rows(int t, const double* __restrict__ ra, const double* __restrict__ rb, double* va, double* vb, int stream_rows) {
#if defined(__HIP_DEVICE_COMPILE__) && CP_WIDE_IO
        // 16-byte accesses: the even lane of each pair loads (a[n], a[n+1]) from row a, the odd lane (b[n], b[n+1]) from row b
        // (n = the even lane's sample), then they trade one double through a DPP lane swap so that every lane holds its own
        // (a[n], b[n]).  Halves the vector-memory instructions; 8-byte-per-lane accesses issue at about half the rate.
        if (T >= 2 && !(CP_ABLATE & 8)) {
            // The trade itself is done when the rows are consumed (unpack_rows, phase 0 of the next pair): any ALU work on
            // the loaded registers here would make this phase wait for the HBM round trip.
            const bool odd = t & 1;
            const long long drow = reinterpret_cast<const char*>(rb) - reinterpret_cast<const char*>(ra);
            const unsigned voff = (unsigned)(t & ~1) * 8u + (odd ? (unsigned)drow : 0u);
#pragma unroll
            for (int r = 0; r < H; ++r) {
                const cplx v = ld_cplx(ra, voff, (unsigned)(T * r) * 8u);  // (lo, hi) = samples n, n + 1 of this lane's row
                va[r] = v.re;
                vb[r] = v.im;
            }
            return;
        }
#endif
        if ((stream_rows & 1) && !(CP_ABLATE & 8)) {  // wave-uniform (a kernel argument)
#pragma unroll
            for (int r = 0; r < H; ++r) {
                va[r] = ld_row_f64_nt(ra, (unsigned)t * 8u, (unsigned)(T * r) * 8u);
                vb[r] = ld_row_f64_nt(rb, (unsigned)t * 8u, (unsigned)(T * r) * 8u);
            }
            return;
        }
#pragma unroll
        for (int r = 0; r < H; ++r) {
            if (CP_ABLATE & 8) {
                va[r] = 1e-3 * t + r;
                vb[r] = 2e-3 * t - r;
            } else {
                va[r] = ld_f64(ra, (unsigned)t * 8u, (unsigned)(T * r) * 8u);
                vb[r] = ld_f64(rb, (unsigned)t * 8u, (unsigned)(T * r) * 8u);
            }
        }
    }

    // ... and consume: x[r + Q] = (va[r], vb[r]) * pre[t + T (r + 4)]; padded points from the constant / edge value.
    // SCREEN_AHEAD: the products were formed when the rows were screened (screen_prefetched) and st.info_cur holds the verdict;
    // otherwise the screening happens in here (`info` returns the pair's exponent fields).
    template <class ST>
    static CP_HD void load_input_half(int t, int t_real, const FftlogArgs& A, const double* __restrict__ ra, const double* __restrict__ rb,
                                      bool has_b, const double* __restrict__ pre, cplx* lds, ST& st, cplx* x) {
        double ia[H], ib[H];
#pragma unroll
        for (int r = 0; r < H; ++r) ia[r] = st.va[r], ib[r] = st.vb[r];
#if defined(__HIP_DEVICE_COMPILE__) && CP_WIDE_IO
        // (va, vb) hold (row[n], row[n+1]) of this lane's row: trade with the neighbour lane
        if (T >= 2 && !(CP_ABLATE & 8)) lane_transpose2_all<H>(ia, ib);
#endif
#if defined(__HIP_DEVICE_COMPILE__)
        constexpr bool tilted = SCREEN_AHEAD;
#else
        constexpr bool tilted = false;
#endif
#pragma unroll
        for (int r = 0; r < H; ++r) {
            x[r + Q].re = tilted ? ia[r] : ia[r] * st.fpre[r];
            x[r + Q].im = tilted ? ib[r] : ib[r] * st.fpre[r];  // an incomplete pair has row b aliased to row a (never stored)
        }
        if constexpr (IN_MODE == IN_HALF) {
            const double la = A.ext_l == CP_EXTRAP_CONST ? A.val_l : ra[0];
            const double lb = A.ext_l == CP_EXTRAP_CONST ? A.val_l : rb[0];
            const double ha = A.ext_r == CP_EXTRAP_CONST ? A.val_r : ra[A.n - 1];
            const double hb = A.ext_r == CP_EXTRAP_CONST ? A.val_r : rb[A.n - 1];
#pragma unroll
            for (int r = 0; r < Q; ++r) {
                const double fl = pre[t + T * r], fh = pre[t + T * (r + 3 * Q)];
                x[r].re = la * fl;
                x[r].im = lb * fl;
                x[r + 3 * Q].re = ha * fh;
                x[r + 3 * Q].im = hb * fh;
            }
        } else {
#pragma unroll
            for (int r = 0; r < Q; ++r) x[r] = x[r + 3 * Q] = cplx{0., 0.};
        }
        if constexpr (SCREEN) {
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (SCREEN_AHEAD) {
                fix_input<H>(st.info_cur, x + Q);
                return;
            }
#endif
            if constexpr (IN_MODE == IN_HALF) {
                screen_in_phase0<P>(t_real, A, ra, rb, pre, lds, st.info_cur, x);
            } else {  // zero padding: only the H in-range points count
                screen_in_phase0<H>(t_real, A, ra, rb, pre, lds, st.info_cur, x + Q);
            }
        }
    }

    // generic phase 0 front end: x[r] = (a[j], b[j]) * pre[j], j = t + T r  (pass 0: R = P, M = T); the row screening reduces
    // over the workgroup in here (`info` returns the pair's exponent fields)
    static CP_HD void load_input(int t, int t_real, const FftlogArgs& A, const double* __restrict__ ra, const double* __restrict__ rb, bool has_b,
                                 const double* __restrict__ pre, cplx* lds, unsigned& info, cplx* x) {
        const LogEnds ea = log_ends(ra, A), eb = log_ends(rb, A);
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int j = t + T * r;
            const double f = pre[j];
            x[r].re = fetch_log(ra, j, A, ea) * f;
            x[r].im = fetch_log(rb, j, A, eb) * f;  // an incomplete pair has row b aliased to row a (never stored)
        }
        if constexpr (SCREEN) screen_in_phase0<P>(t_real, A, ra, rb, pre, lds, info, x);
    }

    // OUT_HALF back end with the postfactors already in registers: the 16 stores go out back to back
    // nker > 1: the factors of the NEXT pair (kernel index nxt_ker) are loaded between the last use of fpost and the
    // stores, so that no load is ever issued behind a store (vmcnt retires in order).
    template <class ST>
    static CP_HD void store_output_half(int t, const FftlogArgs& A, double* __restrict__ oa, double* __restrict__ ob, bool has_b, int nxt_ker,
                                        ST& st, const cplx* x) {
        double ya[H], yb[H];
#pragma unroll
        for (int s = 0; s < H; ++s) {
            ya[s] = x[s + Q].re * st.fpost[s];
            yb[s] = x[s + Q].im * st.fpost[s];
        }
        if constexpr (SCREEN) fix_output<H>(st.info_cur, ya, yb);
        if (A.nker > 1) {
            CP_SCHED_FENCE();
            load_factors_half<!SCREEN_AHEAD_DEVICE>(t, A, nxt_ker, st);  // screen_prefetched has the next prefactors already
            CP_SCHED_FENCE();
        }
        if (CP_ABLATE & 16) {
            double acc = 0.;
#pragma unroll
            for (int s = 0; s < H; ++s) acc += ya[s] * yb[s];
            if (acc == 1.2345e301) oa[t] = acc;  // keeps the results alive, never taken
            return;
        }
        if constexpr (OUT_MODE == OUT_HALF_WINDOW) {  // column t + T s of the row, kept if inside the window
#pragma unroll
            for (int s = 0; s < H; ++s) {
                const int c = t + T * s;
                if (c >= A.out_first && c < A.out_last) {
                    if (A.stream_rows & 2) {
                        st_row_f64_nt(oa, (unsigned)t * 8u, (unsigned)(T * s) * 8u, ya[s]);
                        if (has_b) st_row_f64_nt(ob, (unsigned)t * 8u, (unsigned)(T * s) * 8u, yb[s]);
                    } else {
                        st_f64(oa, (unsigned)t * 8u, (unsigned)(T * s) * 8u, ya[s]);
                        if (has_b) st_f64(ob, (unsigned)t * 8u, (unsigned)(T * s) * 8u, yb[s]);
                    }
                }
            }
            return;
        }
#if defined(__HIP_DEVICE_COMPILE__) && CP_WIDE_IO
        if (T >= 2) {
            // 16-byte stores, mirror image of prefetch_rows: even lanes write (g_a[n], g_a[n+1]) to row a, odd lanes
            // (g_b[n], g_b[n+1]) to row b
            const bool odd = t & 1;
            const long long drow = reinterpret_cast<char*>(ob) - reinterpret_cast<char*>(oa);
            const unsigned voff = (unsigned)(t & ~1) * 8u + (odd ? (unsigned)drow : 0u);
            lane_transpose2_all<H>(ya, yb);
            if (has_b || !odd) {
#pragma unroll
                for (int s = 0; s < H; ++s) st_cplx(oa, voff, (unsigned)(T * s) * 8u, cplx{ya[s], yb[s]});
            }
            return;
        }
#endif
        if (A.stream_rows & 2) {  // wave-uniform (a kernel argument)
#pragma unroll
            for (int s = 0; s < H; ++s) st_row_f64_nt(oa, (unsigned)t * 8u, (unsigned)(T * s) * 8u, ya[s]);
            if (has_b) {
#pragma unroll
                for (int s = 0; s < H; ++s) st_row_f64_nt(ob, (unsigned)t * 8u, (unsigned)(T * s) * 8u, yb[s]);
            }
            return;
        }
#pragma unroll
        for (int s = 0; s < H; ++s) st_f64(oa, (unsigned)t * 8u, (unsigned)(T * s) * 8u, ya[s]);
        if (has_b) {
#pragma unroll
            for (int s = 0; s < H; ++s) st_f64(ob, (unsigned)t * 8u, (unsigned)(T * s) * 8u, yb[s]);
        }
    }

    // last phase back end: natural-order outputs n = t + T s -> crop, x post, split Re/Im to the two rows
    static CP_HD void store_output(int t, const FftlogArgs& A, double* __restrict__ oa, double* __restrict__ ob, bool has_b,
                                   const double* __restrict__ post, unsigned fix, const cplx* x) {
        if constexpr (HALF_OUT) {
            static_assert(!HALF_OUT, "OUT_HALF goes through store_output_half");
        } else {
#pragma unroll
            for (int s = 0; s < P; ++s) {
                const int nidx = t + T * s;
                const int o = nidx - A.out_off;
                if (o >= 0 && o < A.n_out) {
                    const double f = post[nidx];      // (requested point by point: all P together cost registers the log-extrapolating variant does not have -- 2.98 -> 3.10 ms, tools/bench_generic_fftlog.py)
                    double ya = x[s].re * f, yb = x[s].im * f;
                    if constexpr (SCREEN) fix_output<1>(fix, &ya, &yb);
                    oa[o] = ya;
                    if (has_b) ob[o] = yb;
                }
            }
        }
    }

    // ---- registers that live across phases (and pairs) -------------------------------------------------------
    // w     : the tables (twiddles or U) of the NEXT phase, loaded one phase ahead: the loads are issued right after
    //         the LDS writes of the previous phase, BEFORE the workgroup barrier, when x[] is dead -- so the L2
    //         latency overlaps the barrier and the LDS reads instead of sitting on the critical path of every phase.
    //         After the last phase w still holds the pass-0 twiddles, which are what the next pair's phase 0 needs.
    // fpre / fpost, va / vb : HALF modes only: pre / postfactors of the thread's 8 in-range points (pair-invariant
    //         when nker == 1) and the pair's rows, prefetched one whole pair ahead.
    struct State {
        int t0;  // pass0_thread(t)
        unsigned info_cur, info_nxt;  // row screening of the current / the next (prefetched) pair, wave-uniform
        cplx w[P];
        cplx wpin[KPIN > 0 ? KPIN : 1];
        double fpre[H], fpost[H];
        double va[H], vb[H];
#if defined(CP_STAMPS)
        unsigned long long fs[8], fs_last;  // fine stamps: [PH] LDS reads landed (PH 1..4), [5] U applied, [6] last twiddles applied
#endif
    };

    template <int I>
    static CP_HD void load_twiddles(int t, const FftlogArgs& A, cplx* w) {
        Pass<NP, P, I>::template twiddle_load<(I == 0 ? KPIN : 0)>(t, A.tw + PL::tw_offset(I), w);
    }
    template <class ST>
    static CP_HD void merge_pinned(const ST& st, cplx* wl) {
#pragma unroll
        for (int s = 0; s < P; ++s) wl[s] = (s >= 1 && s <= KPIN) ? st.wpin[s - 1] : st.w[s];
    }

    static CP_HD void load_u(int t, const FftlogArgs& A, int ker, cplx* w) {
        const cplx* __restrict__ u = A.u + (long long)ker * NP;
#pragma unroll
        for (int e = 0; e < P; ++e) {
            if (CP_ABLATE & 4) w[e] = cplx{1. + 1e-9 * t, 0.5 + e};
            else w[e] = ld_cplx(u, (unsigned)t * 16u, (unsigned)(e * T) * 16u);
        }
    }

    template <bool WITH_PRE = true>
    static CP_HD void load_factors_half(int t, const FftlogArgs& A, int ker, State& st) {
        const double* __restrict__ pre = A.pre + (long long)ker * NP;
        const double* __restrict__ post = A.post + (long long)ker * NP;
#pragma unroll
        for (int r = 0; r < H; ++r) {
#if defined(CP_DIAG_CONST_FACTORS)      // diagnostic builds (wrong results): the 32 registers of the factors given back -- an upper bound on what forming them from one
            // value per thread (they are power laws) and pinning more twiddles instead could return (tools/mb_pin_factors.sh)
            if (WITH_PRE) st.fpre[r] = 1.25;
            st.fpost[r] = 0.75;
#else
            if (WITH_PRE) st.fpre[r] = ld_f64(pre, (unsigned)t * 8u, (unsigned)(T * (r + Q)) * 8u);
            st.fpost[r] = ld_f64(post, (unsigned)t * 8u, (unsigned)(T * (r + Q)) * 8u);
#endif
        }
    }

    // once per workgroup: thread t copies its share of the middle-pass twiddle tables into LDS (a barrier follows)
    static CP_HD void fill_lds_tables(int t, const FftlogArgs& A, cplx* lds) {
        for (int i = t; i < LDS_TW_ENTRIES; i += T) lds[LDS_DATA + i] = A.tw[NP + i];
    }

    // SCREEN_AHEAD: tilt the rows in the prefetch registers (the NEXT pair; the products stay in va / vb for its phase 0) and
    // publish their magnitudes for the reduction over the workgroup.  Called in the phase in front of the last barrier of a pair,
    // where the prefetch (issued in phase 0, ahead of the U loads that phase LAST has already waited for) has long landed.
    // With several kernels the next pair's prefactors are fetched here (the current ones are dead after phase 0).
    static CP_HD void screen_prefetched(int t, int t0, const FftlogArgs& A, int nxt_ker, cplx* lds, State& st) {
#if defined(__HIP_DEVICE_COMPILE__)
        if constexpr (SCREEN_AHEAD) {
            if (A.nker > 1) {
                const double* __restrict__ pre = A.pre + (long long)nxt_ker * NP;
#pragma unroll
                for (int r = 0; r < H; ++r) st.fpre[r] = ld_f64(pre, (unsigned)t0 * 8u, (unsigned)(T * (r + Q)) * 8u);
            }
#pragma unroll
            for (int r = 0; r < H; ++r) {
                st.va[r] *= st.fpre[r];
                st.vb[r] *= st.fpre[r];
            }
            unsigned ma = 0, mb = 0;
            thread_max<H>(st.va, st.vb, ma, mb);
            screen_publish(t, lds, ma, mb);
        }
#endif
    }

    // before the first pair of a workgroup
    static CP_HD void init_state(int t, const FftlogArgs& A, const double* ra, const double* rb, int ker, State& st) {
        st.t0 = pass0_thread(t);
        if constexpr (NPASS > 1) load_twiddles<0>(st.t0, A, st.w);
        if constexpr (KPIN > 0) {
            const cplx* tw0 = A.tw + PL::tw_offset(0);
#pragma unroll
            for (int s = 1; s <= KPIN; ++s) st.wpin[s - 1] = ld_cplx(tw0, (unsigned)st.t0 * 16u, (unsigned)(s * T) * 16u);
        }
        if constexpr (HALF_IN) {
            load_factors_half(st.t0, A, ker, st);
            if constexpr (ROWS_FROM_MEMORY) prefetch_rows(st.t0, ra, rb, st.va, st.vb, A.stream_rows);
        }
    }

    // global tables of phase PHN into w (called at the end of phase PHN - 1): U for the middle phase, the pass-0
    // twiddles for the last phase (they then stay in w for the next pair's phase 0); the middle passes read LDS tables
    template <int PHN>
    static CP_HD void load_tables_for(int t, int t0, const FftlogArgs& A, int ker, cplx* w) {
        if constexpr (PHN == LAST) {
            load_u(t, A, ker, w);
        } else if constexpr (PHN == NPH - 1) {
#if defined(CP_DIAG_SKIP_TW0_RELOAD)      // diagnostic builds (wrong results): what the reload of the pass-0 twiddles in front of the last phase costs
            (void)t0;
#else
            load_twiddles<0>(t0, A, w);
#endif
        }
    }

    static CP_HD void mul_w(const cplx* w, cplx* x) {
        if (CP_ABLATE & 32) {
            x[1].re += w[1].re + w[P - 1].im;
            return;
        }
#pragma unroll
        for (int e = 0; e < P; ++e) x[e] = cmul(x[e], w[e]);
    }

    // one phase for thread t; lds holds NP complex slots (unused when NPASS == 1).
    // rb / ob always point at valid rows (the caller aliases them to row a when the pair is incomplete).
    // nra / nrb / nxt_ker: rows and kernel index of the pair this workgroup handles next (the current ones on its last pair).
    template <int PH>
    static CP_HD void phase(int t, const FftlogArgs& A, const double* ra, const double* rb, double* oa, double* ob, bool has_b, int ker,
                            cplx* lds, const double* nra, const double* nrb, int nxt_ker, State& st) {
        cplx x[P];
#if defined(__HIP_DEVICE_COMPILE__)
        // Launder the thread index once per phase: stops the compiler from sharing (and keeping
        // live, or hoisting out of the persistent loop) the per-phase LDS / table addresses across
        // phases, which otherwise costs >100 VGPRs and spills.  Addresses are cheap to recompute.
        asm volatile("" : "+v"(t));
#endif
        int t0 = st.t0;  // the thread's pass-0 butterfly (phases 0 and NPH - 1, pass-0 tables)
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(t0));
#endif
        const double* pre = A.pre + (long long)ker * NP;
        const double* post = A.post + (long long)ker * NP;
        CP_FS_BEGIN(st);
        if constexpr (NPASS == 1) {
            load_input(t0, t, A, ra, rb, has_b, pre, lds, st.info_cur, x);
            Pass<NP, P, 0>::butterflies(x);
            load_u(t0, A, ker, st.w);
            mul_w(st.w, x);
            Pass<NP, P, 0>::butterflies(x);
            store_output(t0, A, oa, ob, has_b, post, st.info_cur, x);
        } else if constexpr (PH == 0) {
            if constexpr (HALF_IN) {
#if defined(__HIP_DEVICE_COMPILE__)
                if constexpr (SCREEN_AHEAD) st.info_cur = gate(st.info_nxt);  // found a pair ahead (screen_prefetched); 0: nothing to fix
#endif
                load_input_half(t0, t, A, ra, rb, has_b, pre, lds, st, x);
                // The NEXT pair's rows are requested right here, as soon as the prefetch registers are free: a whole pair
                // before they are consumed, ahead of every other memory operation of this pair (vmcnt retires in order, so
                // the U / twiddle waits of phases 2 and 4 also retire them) and never behind this pair's stores.
                CP_SCHED_FENCE();
                if constexpr (ROWS_FROM_MEMORY) prefetch_rows(t0, nra, nrb, st.va, st.vb, A.stream_rows);
                CP_SCHED_FENCE();
            } else {
                load_input(t0, t, A, ra, rb, has_b, pre, lds, st.info_cur, x);
            }
            // IN_HALF_ZERO: points 0..3 and 12..15 are structural zeros
            if constexpr (KPIN > 0) {
                cplx wl[P];
                merge_pinned(st, wl);
                Pass<NP, P, 0>::template butterflies_store<ZERO_PADDED_IN, true>(t0, wl, lds, x);
            } else {
                Pass<NP, P, 0>::template butterflies_store<ZERO_PADDED_IN, true>(t0, st.w, lds, x);
            }
            load_tables_for<1>(t, t0, A, ker, st.w);
            // the LDS twiddles of phase 1 do not depend on the exchange: read them in front of the barrier (w is free), so
            // that only the 16 data reads are left for the burst behind it
            if constexpr (EARLY_TW1) Pass<NP, P, 1>::twiddle_load_lds(t, lds_tw<1>(lds), st.w);
        } else if constexpr (PH < LAST) {
            constexpr int I = (PH < LAST) ? PH : 0;
            // st.w is free during the middle phases (their tables live in LDS): it takes the twiddles, read right behind
            // the data so that the LDS latency hides under the butterflies
            Pass<NP, P, I>::load_lds(t, lds, x);
            if constexpr (!(EARLY_TW1 && PH == 1)) Pass<NP, P, I>::twiddle_load_lds(t, lds_tw<I>(lds), st.w);
            CP_SCHED_FENCE();
            CP_FS(st, PH);
            Pass<NP, P, I>::template butterflies_store<false, true>(t, st.w, lds, x);
            load_tables_for<PH + 1>(t, t0, A, ker, st.w);
        } else if constexpr (PH == LAST) {
            Pass<NP, P, LAST>::load_lds(t, lds, x);
            if constexpr (PH == NPH - 2) {
                CP_SCHED_FENCE();
                screen_prefetched(t, t0, A, nxt_ker, lds, st);
                CP_SCHED_FENCE();
            }
            CP_FS(st, PH);
            Pass<NP, P, LAST>::butterflies(x);  // M == 1: no twiddles
            mul_w(st.w, x);                     // U, digit-reversed order, 1/NP folded in
            CP_FS(st, 5);
            Pass<NP, P, LAST>::template butterflies_store<false, false>(t, st.w, lds, x);
            load_tables_for<PH + 1>(t, t0, A, ker, st.w);
        } else if constexpr (PH < NPH - 1) {
            constexpr int I = (PH > LAST && PH < NPH - 1) ? (NPH - 1 - PH) : 0;
            Pass<NP, P, I>::twiddle_load_lds(t, lds_tw<I>(lds), st.w);
            Pass<NP, P, I>::load_lds(t, lds, x);
            CP_SCHED_FENCE();
            // the screening of the next pair's rows (register-only work) goes behind the LDS reads of this phase: it runs while they land
            if constexpr (PH == NPH - 2) screen_prefetched(t, t0, A, nxt_ker, lds, st);
            CP_SCHED_FENCE();
            CP_FS(st, PH);
            Pass<NP, P, I>::twiddle_apply(st.w, x);
            Pass<NP, P, I>::template butterflies_store<false, false>(t, st.w, lds, x);
            load_tables_for<PH + 1>(t, t0, A, ker, st.w);
        } else {
            Pass<NP, P, 0>::load_lds(t0, lds, x);
#if defined(__HIP_DEVICE_COMPILE__)
            if constexpr (SCREEN_AHEAD) st.info_nxt = screen_collect(lds);  // published in front of the barrier that precedes this phase
#endif
            // No barrier between this pair and the next: the slots read here are exactly the slots this same thread writes in
            // the next pair's phase 0 (pass-0 shape, in place), the LDS executes one wave's instructions in order, and no other
            // thread touches them before the barrier that follows phase 0.
#if defined(__HIP_DEVICE_COMPILE__) && CP_INTERPAIR_BARRIER
            CP_FS(st, PH);
            if (!(CP_ABLATE & 2)) __syncthreads();
            CP_FS(st, 7);
#endif
            // Nothing is loaded after this pair's stores (w keeps the pass-0 twiddles for the next pair's phase 0), so the
            // stores stay in flight while the next pair starts.
            if constexpr (KPIN > 0) {
                cplx wl[P];
                merge_pinned(st, wl);
                Pass<NP, P, 0>::twiddle_apply(wl, x);
            } else {
                Pass<NP, P, 0>::twiddle_apply(st.w, x);
            }
            CP_FS(st, 6);
            Pass<NP, P, 0>::butterflies(x);
            if constexpr (HALF_IN && HALF_OUT) {
                store_output_half(t0, A, oa, ob, has_b, nxt_ker, st, x);
            } else {
                store_output(t0, A, oa, ob, has_b, post, st.info_cur, x);
            }
        }
    }
};

}  // namespace cpfft
