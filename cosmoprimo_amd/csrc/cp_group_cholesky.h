// cp_group_cholesky.h -- the Cholesky pieces of a group of G lanes (G a power of two <= 32, 64 / G groups per wave) that cp_lm.hip and cp_hmc.hip share:
// lane i of a group owns row i of the group's lower triangle, which sits in the wave's own LDS with the row stride G + 1 (row i, column j at
// L[i (G + 1) + j]).  A value goes from one lane of a group to all of them by __shfl; the LDS phases are separated by cp::wave_lds_phase().  Every lane
// of a wave must call these together (they shuffle).  Arithmetic: float64 operations rounded once, in the order written here (the including file sets
// `#pragma clang fp contract(off)` before it includes this header, and this header sets it again for itself); tests/lm_reference.py restates them.
#pragma once

#include <cfloat>

#include "cp_internal.h"

#pragma clang fp contract(off)

namespace cp {

__device__ __forceinline__ bool lm_finite(double v) { return fabs(v) <= DBL_MAX; }

// the value lane j of this lane's group holds
template <int G>
__device__ __forceinline__ double group_value(double v, int j) {
    return G == 1 ? v : __shfl(v, j, G);
}

// In place: the group's raw matrix in L (row i, column j at L[i (G + 1) + j]; the triangle j <= i is read) becomes its Cholesky factor.  diag: this
// lane's diagonal entry as the system takes it; held: the group's held parameters, a bit each.  lii: L[i][i].  Returns 0, or the 1-based column of the
// first pivot that is not > 0 or not finite (what follows it is then meaningless, and harmless).
template <int G>
__device__ __forceinline__ int lm_factor(double* L, const int i, const int n, const unsigned held, const double diag, double& lii) {
    constexpr int S = G + 1;
    const bool hi = (held >> i) & 1u;
    int bad = 0;
    lii = 1.;
    for (int j = 0; j < n; ++j) {
        double t = i == j ? diag : L[i * S + j];
        if (hi || ((held >> j) & 1u)) t = i == j ? 1. : 0.;
        for (int k = 0; k < j; ++k) t -= L[i * S + k] * L[j * S + k];
        const double d = group_value<G>(t, j);
        if (!bad && !(d > 0. && lm_finite(d))) bad = j + 1;
        const double r = sqrt(d);
        if (i == j) lii = r;
        if (i >= j) L[i * S + j] = i == j ? r : t / r;
        cp::wave_lds_phase();
    }
    return bad;
}

// y_i of L y = r by forward substitution, j ascending from `first`: r_i this lane's right-hand side with r_k = 0 for k < first; y is valid for i >= first
template <int G>
__device__ __forceinline__ double lm_forward(const double* L, const int i, const int n, const double lii, double r, const int first) {
    constexpr int S = G + 1;
    for (int j = first; j < n; ++j) {
        double q = 0.;
        if (i == j) q = r / lii;
        const double y = group_value<G>(q, j);
        if (i > j) r -= L[i * S + j] * y;
        else if (i == j) r = y;
    }
    return r;
}

// z_i of L^T z = r by back substitution, j descending to `first`; z is valid for i >= first
template <int G>
__device__ __forceinline__ double lm_backward(const double* L, const int i, const int n, const double lii, double r, const int first) {
    constexpr int S = G + 1;
    for (int j = n - 1; j >= first; --j) {
        double q = 0.;
        if (i == j) q = r / lii;
        const double z = group_value<G>(q, j);
        if (i < j) r -= L[j * S + i] * z;
        else if (i == j) r = z;
    }
    return r;
}

// z_i of L L^T z = r, r_i this lane's right-hand side with r_k = 0 for k < first; z is valid for i >= first (all of it with first = 0)
template <int G>
__device__ __forceinline__ double lm_solve(const double* L, const int i, const int n, const double lii, const double r, const int first) {
    return lm_backward<G>(L, i, n, lii, lm_forward<G>(L, i, n, lii, r, first), first);
}

// lanes per fit: the smallest power of two >= ndim
inline int lm_lanes_of(int ndim) {
    int G = 1;
    while (G < ndim) G *= 2;
    return G;
}

// threads of a workgroup: four waves, two at G = 32 (the static LDS stays under 64 KB)
constexpr int lm_threads(int G) { return G == 32 ? 128 : 256; }

}  // namespace cp
