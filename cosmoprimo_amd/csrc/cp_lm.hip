// cp_lm.hip -- what stands between two calls of cp_*_gauss_newton in a batch of Levenberg-Marquardt fits (cp_lm_step; cp_lm_step_velocity: the same
// kernel, which also writes the step it solved), the second-order correction of that step (cp_lm_accelerate: geodesic acceleration), and the covariance
// behind the last call (cp_spd_inverse): B independent fits of 1 <= ndim <= 32 parameters, one launch each, nothing read back.
// Mapping.  A fit is a group of G lanes, G the smallest power of two >= ndim: 64 / G fits per wave, four waves per workgroup (two at G = 32: the static
// LDS stays under 64 KB).  Lane i of a group owns parameter i and row i of the fit's lower triangle, in the wave's own LDS with the row stride G + 1
// (64 (G + 1) doubles per wave: 17 KB at G = 32; nothing of a row in registers, no scratch).  A value goes from one lane of a group to all of them by
// __shfl; the column steps of the factorisation are separated by cp::wave_lds_phase().  No workgroup barrier, no atomics: two calls give the same bits,
// and a fit reads and writes nothing of another.
// Arithmetic.  Every operation is a float64 operation rounded once, in a stated order (no contraction into FMAs: tests/lm_reference.py restates them in
// numpy); divisions and square roots are the correctly rounded ones.
//   factor: for columns j in order, t_i = A[i][j] - sum_{k < j, in order} L[i][k] L[j][k] for i >= j; the pivot d = t_j must be > 0 and finite;
//           L[j][j] = sqrt(d), L[i][j] = t_i / L[j][j].
//   solve:  L y = r with r_i -= L[i][j] y_j for j ascending, y_j = r_j / L[j][j]; then L^T z = y with r_i -= L[j][i] z_j for j DEscending.
//   A held parameter h of cp_lm_step is taken out of the system by A[h][h] = 1, A[h][.] = A[.][h] = 0, r_h = 0: the free parameters see exact zeros.
//   accelerate: a = solve(held ? 0 : -h) on the factor of F + lambda diag F; sa = sum_i (F_ii a_i) a_i and sv = sum_i (F_ii v_i) v_i over the free
//           parameters, i ascending, from 0.; the correction is taken if sv > 0, sa is finite and 4 sa <= (alpha alpha) sv; then
//           next_i = clip(x_i + (v_i + 0.5 a_i)), else clip(x_i + v_i): with the v of cp_lm_step_velocity, the bits of cp_lm_step's next.
#include <cfloat>

#include "cp_internal.h"

#pragma clang fp contract(off)

#include "cp_group_cholesky.h"      // group_value, lm_factor, lm_solve (lm_forward, then lm_backward): shared with cp_hmc.hip

namespace {

using cp::group_value;
using cp::lm_factor;
using cp::lm_finite;
using cp::lm_solve;
using cp::lm_threads;

struct LmArgs {
    long long B;
    int ndim;
    double *x, *fisher, *grad, *chi2, *lambda;
    int *status, *naccepted;
    const double *xt, *fisher_t, *grad_t, *chi2_t, *lo, *hi;
    double up, down, lmin, lmax, ftol;
    double* next;
    double* velocity;      // null: cp_lm_step
};

struct LmAccelArgs {
    long long B;
    int ndim;
    const double *x, *fisher, *grad, *lambda;
    const int* status;
    const double *lo, *hi, *velocity, *h;
    double alpha;
    double* next;
    int* naccelerated;
};

// a parameter on a bound with the gradient pointing out of the box: held, by cp_lm_step and by cp_lm_accelerate alike
__device__ __forceinline__ bool lm_on_bound(double x, double g, double lo, double hi) { return (x >= hi && g > 0.) || (x <= lo && g < 0.); }

// the held parameters of this lane's group, a bit each
template <int G>
__device__ __forceinline__ unsigned lm_held(bool hold, int lane, int i) {
    const unsigned long long all = __ballot(hold);
    return (unsigned)((all >> (lane - i)) & (G == 32 ? 0xffffffffull : (1ull << G) - 1ull));
}

template <int G>
__global__ __launch_bounds__(lm_threads(G)) void lm_step_kernel(const LmArgs a) {
    constexpr int S = G + 1, FPW = 64 / G, WAVES = lm_threads(G) / 64;
    __shared__ double lds[WAVES * 64 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & (G - 1), f = lane / G, n = a.ndim;
    const long long b = ((long long)blockIdx.x * WAVES + wave) * FPW + f;
    double* const L = lds + (wave * FPW + f) * (G * S);
    const bool fit = b < a.B, live = fit && i < n;
    const double inf = __builtin_huge_val();

    // the decision, every lane of the group alike
    int status = 1, nacc = 0;
    double chi = 0., chit = 0., lam = 1.;
    if (fit) status = a.status[b], nacc = a.naccepted[b], chi = a.chi2[b], chit = a.chi2_t[b], lam = a.lambda[b];
    const bool frozen = status != 0;
    const bool accept = !frozen && lm_finite(chit) && chit <= chi;
    if (accept) {
        if (lm_finite(chi) && chi - chit <= a.ftol * chi) status = 1;
        if (nacc > 0) {
            lam = lam * a.down;
            lam = lam < a.lmin ? a.lmin : lam;
        }
        ++nacc;
        chi = chit;
    } else if (!frozen) {
        if (chi == inf) {
            status = 3;
        } else {
            lam = lam * a.up;
            if (lam > a.lmax) lam = a.lmax, status = 2;
        }
    }

    // the trial into the state where it is accepted; the point the next step leaves from
    double xv = 0., gv = 0., lo = 0., hi = 0.;
    if (live) {
        xv = accept ? a.xt[b * n + i] : a.x[b * n + i];
        gv = accept ? a.grad_t[b * n + i] : a.grad[b * n + i];
        lo = a.lo[i], hi = a.hi[i];
        if (accept) a.x[b * n + i] = xv, a.grad[b * n + i] = gv;
    }
    if (fit) {
        const double* const from = (accept ? a.fisher_t : a.fisher) + b * n * n;
        for (int e = i; e < n * n; e += G) {
            const double v = from[e];
            if (accept) a.fisher[b * n * n + e] = v;
            L[(e / n) * S + e % n] = v;
        }
    }
    cp::wave_lds_phase();

    const bool hold = live && status == 0 && lm_on_bound(xv, gv, lo, hi);
    const unsigned held = lm_held<G>(hold, lane, i);
    const double fii = live ? L[i * S + i] : 1.;
    double lii;
    const int bad = lm_factor<G>(L, i, n, held, fii + lam * fii, lii);
    if (status == 0 && bad) status = 3;
    const double delta = lm_solve<G>(L, i, n, lii, hold ? 0. : gv, 0);

    if (live) {
        double v = xv;
        if (status == 0 && !hold) {
            v = xv + delta;
            v = v < lo ? lo : v;
            v = v > hi ? hi : v;
        }
        a.next[b * n + i] = v;
        if (a.velocity) a.velocity[b * n + i] = status == 0 && !hold ? delta : 0.;
    }
    if (fit && !frozen && i == 0) a.chi2[b] = chi, a.lambda[b] = lam, a.status[b] = status, a.naccepted[b] = nacc;
}

// The second-order correction of the step cp_lm_step left behind: see the head of this file for the arithmetic.
template <int G>
__global__ __launch_bounds__(lm_threads(G)) void lm_accelerate_kernel(const LmAccelArgs a) {
    constexpr int S = G + 1, FPW = 64 / G, WAVES = lm_threads(G) / 64;
    __shared__ double lds[WAVES * 64 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & (G - 1), f = lane / G, n = a.ndim;
    const long long b = ((long long)blockIdx.x * WAVES + wave) * FPW + f;
    double* const L = lds + (wave * FPW + f) * (G * S);
    const bool fit = b < a.B, live = fit && i < n;

    int status = 1;
    double lam = 1.;
    if (fit) status = a.status[b], lam = a.lambda[b];
    double xv = 0., gv = 0., lo = 0., hi = 0., vv = 0., hv = 0.;
    if (live) {
        xv = a.x[b * n + i], gv = a.grad[b * n + i], vv = a.velocity[b * n + i], hv = a.h[b * n + i];
        lo = a.lo[i], hi = a.hi[i];
    }
    if (fit)
        for (int e = i; e < n * n; e += G) L[(e / n) * S + e % n] = a.fisher[b * n * n + e];
    cp::wave_lds_phase();

    const bool hold = live && status == 0 && lm_on_bound(xv, gv, lo, hi);
    const unsigned held = lm_held<G>(hold, lane, i);
    const double fii = live ? L[i * S + i] : 1.;
    double lii;
    const int bad = lm_factor<G>(L, i, n, held, fii + lam * fii, lii);
    const double acc = lm_solve<G>(L, i, n, lii, hold ? 0. : -hv, 0);

    // the gate: both sums over the free parameters, ascending, every lane of the group alike
    const double ta = (fii * acc) * acc, tv = (fii * vv) * vv;
    double sa = 0., sv = 0.;
    for (int j = 0; j < n; ++j) {
        const double pa = group_value<G>(ta, j), pv = group_value<G>(tv, j);
        if (!((held >> j) & 1u)) sa = sa + pa, sv = sv + pv;
    }
    const bool running = status == 0 && !bad;
    const bool take = running && sv > 0. && lm_finite(sa) && 4. * sa <= (a.alpha * a.alpha) * sv;

    if (live) {
        double v = xv;
        if (running && !hold) {
            v = xv + (take ? vv + 0.5 * acc : vv);
            v = v < lo ? lo : v;
            v = v > hi ? hi : v;
        }
        a.next[b * n + i] = v;
    }
    if (fit && take && i == 0) a.naccelerated[b] = a.naccelerated[b] + 1;
}

template <int G>
__global__ __launch_bounds__(lm_threads(G)) void spd_inverse_kernel(const long long B, const int n, const double* a, double* inv, int* info) {
    constexpr int S = G + 1, FPW = 64 / G, WAVES = lm_threads(G) / 64;
    __shared__ double lds[WAVES * 64 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & (G - 1), f = lane / G;
    const long long b = ((long long)blockIdx.x * WAVES + wave) * FPW + f;
    double* const L = lds + (wave * FPW + f) * (G * S);
    const bool fit = b < B, live = fit && i < n;
    if (fit)
        for (int e = i; e < n * n; e += G) L[(e / n) * S + e % n] = a[b * n * n + e];
    cp::wave_lds_phase();
    double lii;
    const int bad = lm_factor<G>(L, i, n, 0u, live ? L[i * S + i] : 1., lii);
    const double nan = __builtin_nan("");
    for (int c = 0; c < n; ++c) {      // column c of the inverse, its rows i >= c; mirrored
        const double z = lm_solve<G>(L, i, n, lii, i == c ? 1. : 0., c);
        if (live && i >= c) {
            const double v = bad ? nan : z;
            inv[b * n * n + (long long)i * n + c] = v;
            inv[b * n * n + (long long)c * n + i] = v;
        }
    }
    if (fit && i == 0) info[b] = bad;
}

// what the entry points check first, in this order; *per_workgroup: fits of a workgroup
int lm_front(const char* who, long long B, int ndim, int* G, int* per_workgroup) {
    if (B < 0 || ndim < 1) return cp::fail(CP_EINVAL, "%s: %lld fits of %d parameters", who, B, ndim);
    if (ndim > 32) return cp::fail(CP_EUNSUPPORTED, "%s: %d parameters (at most 32)", who, ndim);
    *G = cp::lm_lanes_of(ndim);
    *per_workgroup = lm_threads(*G) / *G;
    if (B > 0x7fffffffLL * *per_workgroup)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld fits of %d parameters (at most 2^31 - 1 workgroups of %d fits)", who, B, ndim, *per_workgroup);
    return CP_OK;
}

}  // namespace

extern "C" int cp_lm_layout(int ndim, int* lanes_per_fit, int* fits_per_workgroup) {
    int G, per;
    const int status = lm_front("cp_lm_layout", 0, ndim, &G, &per);
    if (status != CP_OK) return status;
    if (!lanes_per_fit || !fits_per_workgroup) return cp::fail(CP_EINVAL, "cp_lm_layout: null pointer");
    *lanes_per_fit = G, *fits_per_workgroup = per;
    return CP_OK;
}

namespace {

// cp_lm_step and cp_lm_step_velocity: the checks in the stated order, then the one kernel
int lm_step_front(const char* who, const LmArgs& a, bool velocity, int device, void* stream) {
    int G, per;
    const int status = lm_front(who, a.B, a.ndim, &G, &per);
    if (status != CP_OK) return status;
    if (a.B == 0) return CP_OK;
    if (!a.x || !a.fisher || !a.grad || !a.chi2 || !a.lambda || !a.status || !a.naccepted || !a.xt || !a.fisher_t || !a.grad_t || !a.chi2_t || !a.lo || !a.hi || !a.next ||
        (velocity && !a.velocity))
        return cp::fail(CP_EINVAL, "%s: null pointer", who);
    if (!(a.up > 1.) || !(a.down > 0. && a.down <= 1.) || !(a.lmin > 0. && a.lmin <= a.lmax) || !(a.ftol >= 0.))
        return cp::fail(CP_EINVAL, "%s: up = %g (> 1), down = %g (in (0, 1]), lmin = %g, lmax = %g (0 < lmin <= lmax), ftol = %g (>= 0)", who, a.up, a.down, a.lmin, a.lmax,
                        a.ftol);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "%s: cannot select device %d", who, device);
    const unsigned grid = (unsigned)((a.B + per - 1) / per);
    cp::Launches on(who, stream);
    switch (G) {
        case 1: on.run<lm_step_kernel<1>>(grid, lm_threads(1), 0, a); break;
        case 2: on.run<lm_step_kernel<2>>(grid, lm_threads(2), 0, a); break;
        case 4: on.run<lm_step_kernel<4>>(grid, lm_threads(4), 0, a); break;
        case 8: on.run<lm_step_kernel<8>>(grid, lm_threads(8), 0, a); break;
        case 16: on.run<lm_step_kernel<16>>(grid, lm_threads(16), 0, a); break;
        default: on.run<lm_step_kernel<32>>(grid, lm_threads(32), 0, a); break;
    }
    return on.status();
}

}  // namespace

extern "C" int cp_lm_step(long long B, int ndim, double* d_x, double* d_fisher, double* d_grad, double* d_chi2, double* d_lambda, int* d_status, int* d_naccepted,
                          const double* d_xt, const double* d_fisher_t, const double* d_grad_t, const double* d_chi2_t, const double* d_lo, const double* d_hi, double up,
                          double down, double lmin, double lmax, double ftol, double* d_next, int device, void* stream) {
    const LmArgs a{B, ndim, d_x, d_fisher, d_grad, d_chi2, d_lambda, d_status, d_naccepted, d_xt, d_fisher_t, d_grad_t, d_chi2_t, d_lo, d_hi, up, down, lmin, lmax, ftol, d_next,
                   nullptr};
    return lm_step_front("cp_lm_step", a, false, device, stream);
}

extern "C" int cp_lm_step_velocity(long long B, int ndim, double* d_x, double* d_fisher, double* d_grad, double* d_chi2, double* d_lambda, int* d_status,
                                   int* d_naccepted, const double* d_xt, const double* d_fisher_t, const double* d_grad_t, const double* d_chi2_t, const double* d_lo,
                                   const double* d_hi, double up, double down, double lmin, double lmax, double ftol, double* d_next, double* d_velocity, int device,
                                   void* stream) {
    const LmArgs a{B, ndim, d_x, d_fisher, d_grad, d_chi2, d_lambda, d_status, d_naccepted, d_xt, d_fisher_t, d_grad_t, d_chi2_t, d_lo, d_hi, up, down, lmin, lmax, ftol, d_next,
                   d_velocity};
    return lm_step_front("cp_lm_step_velocity", a, true, device, stream);
}

extern "C" int cp_lm_accelerate(long long B, int ndim, const double* d_x, const double* d_fisher, const double* d_grad, const double* d_lambda, const int* d_status,
                                const double* d_lo, const double* d_hi, const double* d_velocity, const double* d_h, double alpha, double* d_next, int* d_naccelerated,
                                int device, void* stream) {
    int G, per;
    const int status = lm_front("cp_lm_accelerate", B, ndim, &G, &per);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_x || !d_fisher || !d_grad || !d_lambda || !d_status || !d_lo || !d_hi || !d_velocity || !d_h || !d_next || !d_naccelerated)
        return cp::fail(CP_EINVAL, "cp_lm_accelerate: null pointer");
    if (!(alpha > 0. && alpha <= DBL_MAX)) return cp::fail(CP_EINVAL, "cp_lm_accelerate: alpha = %g (finite and > 0)", alpha);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_lm_accelerate: cannot select device %d", device);
    const LmAccelArgs a{B, ndim, d_x, d_fisher, d_grad, d_lambda, d_status, d_lo, d_hi, d_velocity, d_h, alpha, d_next, d_naccelerated};
    const unsigned grid = (unsigned)((B + per - 1) / per);
    cp::Launches on("cp_lm_accelerate", stream);
    switch (G) {
        case 1: on.run<lm_accelerate_kernel<1>>(grid, lm_threads(1), 0, a); break;
        case 2: on.run<lm_accelerate_kernel<2>>(grid, lm_threads(2), 0, a); break;
        case 4: on.run<lm_accelerate_kernel<4>>(grid, lm_threads(4), 0, a); break;
        case 8: on.run<lm_accelerate_kernel<8>>(grid, lm_threads(8), 0, a); break;
        case 16: on.run<lm_accelerate_kernel<16>>(grid, lm_threads(16), 0, a); break;
        default: on.run<lm_accelerate_kernel<32>>(grid, lm_threads(32), 0, a); break;
    }
    return on.status();
}

extern "C" int cp_spd_inverse(long long B, int ndim, const double* d_a, double* d_inv, int* d_info, int device, void* stream) {
    int G, per;
    const int status = lm_front("cp_spd_inverse", B, ndim, &G, &per);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_a || !d_inv || !d_info) return cp::fail(CP_EINVAL, "cp_spd_inverse: null pointer");
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_spd_inverse: cannot select device %d", device);
    const unsigned grid = (unsigned)((B + per - 1) / per);
    cp::Launches on("cp_spd_inverse", stream);
    switch (G) {
        case 1: on.run<spd_inverse_kernel<1>>(grid, lm_threads(1), 0, B, ndim, d_a, d_inv, d_info); break;
        case 2: on.run<spd_inverse_kernel<2>>(grid, lm_threads(2), 0, B, ndim, d_a, d_inv, d_info); break;
        case 4: on.run<spd_inverse_kernel<4>>(grid, lm_threads(4), 0, B, ndim, d_a, d_inv, d_info); break;
        case 8: on.run<spd_inverse_kernel<8>>(grid, lm_threads(8), 0, B, ndim, d_a, d_inv, d_info); break;
        case 16: on.run<spd_inverse_kernel<16>>(grid, lm_threads(16), 0, B, ndim, d_a, d_inv, d_info); break;
        default: on.run<spd_inverse_kernel<32>>(grid, lm_threads(32), 0, B, ndim, d_a, d_inv, d_info); break;
    }
    return on.status();
}
