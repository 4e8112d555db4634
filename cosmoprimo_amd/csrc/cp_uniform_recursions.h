// cp_uniform_recursions.h -- the second derivatives of a cubic spline on a UNIFORMLY spaced stretch of knots, a lane per S consecutive knots in registers.
//
// There the system has constant coefficients, M_{i-1} + 4 M_i + M_{i+1} = (6 / h^2) r_i with the second differences r_i = y_{i+1} - 2 y_i + y_{i-1}, and
// the inverse of a constant tridiagonal matrix is two geometric tails: M_i = (6 kappa / h^2) sum_j p^|i-j| r_j, p = sqrt 3 - 2, kappa = 1 / (2 sqrt 3).
// A lane forms the second differences of its S knots, runs the anti-causal recursion g_t = r_t + p g_{t+1} over them and then the causal one in the same
// registers (r_t = g_t - p g_{t+1}: e_t = g_t + p f_{t-1} is the sum over the segment, f_t = e_t - p g_{t+1} its causal half), both from zero:
// `recursions`.  What the knots outside its segment add comes from the neighbours' segment totals -- G at the first knot of the next segment, F at the last
// knot of the one before --, which the site takes by one shift of the wave each way (`wave_from_right`, `wave_from_left`) and adds as two geometric
// carries: `add_carries`.  A segment away the weight is p^S.
//
// The per-lane arithmetic is plain C++ of a lane's own registers, no shift inside, compiled by hipcc into the kernels and by g++ for the CPU test
// (tests/host_emu/emu_uniform_recursions.cpp, tests/test_uniform_recursions_host.py: 64 emulated lanes against the same truncated sums in longdouble).
// Its users, each of which forms its own second differences and its own two carries:
//   cpdd::second_derivatives_and_box_recursive (cp_wallish_dd.h): S = 32, the ends by reflection (the mirror terms between the two calls) --
//     wallish_dd_box_kernel<32> (cp_bao.hip), dst_generate_kernel's box form, wallish_tail_kernel and wallish_full_kernel (cp_dst.hip, cp_wallish_tail.h);
//   cpsu::splice_uniform_kernel<S> (cp_splice_uniform.h): S = 33 .. 57, the ends by the window sums A, B (m_a sums[0], m_b sums[2]), the causal carry
//     cut at 36 knots;
//   tail_splice_row<SU> (cp_wallish_tail.h): the same row inside the fused tail of the filter;
//   brieden_resample_kernel<S, PEAKS, OPLDS> (cp_bao.hip): S = 3 .. 8, the totals of REACH lanes on either side weighted with p^(S m).
// (The geospline solve of cp_sigma.hip has different ratios to the left and to the right and carry weights from its plan: it takes the shifts only.)
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CPUR_HD __host__ __device__ __forceinline__
#else
#define CPUR_HD inline
#endif

namespace cpur {

constexpr double P = -0.26794919243112270647;         // sqrt 3 - 2
constexpr double KAPPA = 0.28867513459481288225;      // 1 / (2 sqrt 3): M = (6 KAPPA / h^2) x what the recursions return

constexpr double ipow(double x, int k) {
    double v = 1.;
    for (int i = 0; i < k; ++i) v *= x;
    return v;
}

#if defined(__HIPCC__)
// lane l receives the value of lane l - 1 (lane 0: zero) / of lane l + 1 (lane 63: zero): DPP shifts of the whole wave, no LDS
typedef int v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double wave_from_left(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    v2i w = __builtin_bit_cast(v2i, v);
    w.x = __builtin_amdgcn_update_dpp(0, w.x, 0x138, 0xf, 0xf, true);      // wave_shr:1
    w.y = __builtin_amdgcn_update_dpp(0, w.y, 0x138, 0xf, 0xf, true);
    return __builtin_bit_cast(double, w);
#else
    return v;
#endif
}
__device__ __forceinline__ double wave_from_right(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    v2i w = __builtin_bit_cast(v2i, v);
    w.x = __builtin_amdgcn_update_dpp(0, w.x, 0x130, 0xf, 0xf, true);      // wave_shl:1
    w.y = __builtin_amdgcn_update_dpp(0, w.y, 0x130, 0xf, 0xf, true);
    return __builtin_bit_cast(double, w);
#else
    return v;
#endif
}
#endif

// what a site reads of the two passes besides g itself: G at the segment's first and second knot after the anti-causal pass (the total its left neighbour
// takes; the mirror term of a reflected left end), F at its last and last-but-one knot (its right neighbour's; the mirror term of a reflected right end)
struct Totals {
    double g_first, g_second, f_last, f_before_last;
};

// g[S]: the lane's second differences on entry, the sums over its own segment sum_j p^|t-j| r_j on exit
template <int S>
CPUR_HD Totals recursions(double* g) {
    static_assert(S >= 2, "two knots per lane or more");
#pragma unroll
    for (int t = S - 2; t >= 0; --t) g[t] = fma(P, g[t + 1], g[t]);
    Totals out;
    out.g_first = g[0];
    out.g_second = g[1];
    out.f_before_last = 0.;
    double f = 0.;
#pragma unroll
    for (int t = 0; t < S; ++t) {
        const double e = fma(P, f, g[t]);
        f = t + 1 < S ? fma(-P, g[t + 1], e) : e;
        if (t == S - 2) out.f_before_last = f;
        g[t] = e;
    }
    out.f_last = f;
    return out;
}

// gin: G at the first knot of the next segment, carried downwards over all S knots; then fin: F at the last knot of the previous segment, carried
// upwards over the first NF knots (p^36 = 3e-21: splice_uniform_kernel stops there)
template <int S, int NF = S>
CPUR_HD void add_carries(double* g, double gin, double fin) {
    static_assert(NF <= S, "the carry stays inside the segment");
    double c = gin;
#pragma unroll
    for (int t = S - 1; t >= 0; --t) {
        c *= P;
        g[t] += c;
    }
    c = fin;
#pragma unroll
    for (int t = 0; t < NF; ++t) {
        c *= P;
        g[t] += c;
    }
}

}  // namespace cpur
