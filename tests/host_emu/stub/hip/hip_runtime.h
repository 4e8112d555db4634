// A stand-in for <hip/hip_runtime.h> (TEST HARNESS ONLY): what csrc/cp_math.h needs of it to compile, unchanged, with g++ for the CPU tests
// (tests/host_emu/emu_math.cpp, built with this directory first on the include path and -ffp-contract=off).
//
// rint, fma and ldexp are IEEE operations: the forms that use nothing else (exp_mid, exp_tab, exp10_mid, exp10_tab, sin_bounded) give on the host the
// bits the device gives.  The reciprocal and reciprocal-root estimates are NOT bit-faithful: the hardware's v_rcp_f64 / v_rsq_f64 are stood in for
// by the exact value rounded to a float's 24 bits (about their accuracy); recip, rsqrt_pos and log_pos are therefore emulated in their error, not in their bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#define __builtin_assume(c) ((void)0)

namespace cp_hip_stub {
struct Dim3 { unsigned x, y, z; };
inline double to24(double v) { int e; const double m = std::frexp(v, &e); return std::ldexp((double)(float)m, e); }      // (the mantissa of a float, the range of a double)
inline double rcp(double x) { return to24(1. / x); }
inline double rsq(double x) { return to24(1. / std::sqrt(x)); }
inline double frexp_mant(double x) { int e; return std::frexp(x, &e); }
inline int frexp_exp(double x) { int e; std::frexp(x, &e); return e; }
inline int hiint(double x) { std::int64_t b; std::memcpy(&b, &x, 8); return (int)(b >> 32); }
}  // namespace cp_hip_stub

static const cp_hip_stub::Dim3 blockDim = {256, 1, 1};
static const cp_hip_stub::Dim3 threadIdx = {0, 0, 0};

#define __builtin_amdgcn_rcp(x) cp_hip_stub::rcp(x)
#define __builtin_amdgcn_rsq(x) cp_hip_stub::rsq(x)
#define __builtin_amdgcn_frexp_mant(x) cp_hip_stub::frexp_mant(x)
#define __builtin_amdgcn_frexp_exp(x) cp_hip_stub::frexp_exp(x)
#define __double2hiint(x) cp_hip_stub::hiint(x)

using std::fabs;
using std::fma;
using std::fmax;
using std::fmin;
using std::ldexp;
using std::log;
using std::rint;
using std::sin;
