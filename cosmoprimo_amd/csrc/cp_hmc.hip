// cp_hmc.hip -- what stands between two calls of cp_*_gauss_newton in a batch of Hamiltonian Monte Carlo chains of exp(-chi2 / 2) inside a box
// (cp_hmc_step: kick, drift and box test of a leapfrog step; once per trajectory the accept / reject, the sample and the momenta of the next one) and
// the Cholesky factor of the chains' mass matrices (cp_hmc_factor): B independent chains of 1 <= ndim <= 32 parameters, one launch each, nothing read back.
// Mapping: cp_lm.hip's.  A chain is a group of G lanes, G the smallest power of two >= ndim: 64 / G chains per wave, four waves per workgroup (two at
// G = 32).  Lane i of a group owns parameter i and row i of the chain's factor L (metric = L L^T), in the wave's own LDS with the row stride G + 1.  A
// value goes from one lane of a group to all of them by __shfl; LDS phases are separated by cp::wave_lds_phase().  No workgroup barrier, no atomics: two
// calls give the same bits, and a chain reads and writes nothing of another.
// Arithmetic.  Every operation but log, sin, cos and sqrt (the library's) is a float64 operation rounded once, in the stated order (no contraction
// into FMAs: tests/hmc_reference.py restates them in numpy).  The momentum is kept whitened: p = L z, K = z.z / 2; a kick is z += e L^-1 g (forward
// substitution, ascending) with g = -1/2 d chi2 / d theta, a drift x += e L^-T z (back substitution, descending).
// Random numbers: Philox4x32-10 written out below (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; round r uses
// key + r increment), key = (seed low, seed high), counter = (b low, b high, t, slot) for chain b, trajectory t and slot: a chain's stream depends on
// (seed, b, t) only.  Words w0..w3 -> u_a = min(((w0 >> 5) 2^26 + (w1 >> 6) + 0.5) 2^-53, 1 - 2^-53), u_b likewise from w2, w3: strictly inside (0, 1)
// (the minimum binds for the one largest 53-bit integer, which the rounded sum takes to 2^53).  Slots 0..15: the normals of parameters 2 s and 2 s + 1,
// r = sqrt(-2 log u_a), angle = 6.283185307179586 u_b, r cos(angle) and r sin(angle).  Slot 16: the step jitter u_j = u_a and the acceptance variate
// e = -log(u_b).
#include <cfloat>
#include <cstdint>

#include "cp_internal.h"

#pragma clang fp contract(off)

#include "cp_group_cholesky.h"

namespace {

using cp::group_value;
using cp::lm_backward;
using cp::lm_factor;
using cp::lm_finite;
using cp::lm_forward;
using cp::lm_threads;

struct HmcArgs {
    long long B;
    int ndim;
    long long t_close, t_open;      // < 0: the call does not close, does not open
    double *x, *grad, *chi2;
    int *status, *naccepted, *nout;
    double *z, *h0, *eps;
    int* out;
    const double *xt, *grad_t, *chi2_t, *factor, *lo, *hi, *step;
    double jitter;
    unsigned long long seed;
    double *next, *sample, *sample_chi2;      // the last two null together
};

struct Philox {
    uint32_t w[4];
};

__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0, c1 = lo1, c2 = n2, c3 = lo0;
        k0 += W0, k1 += W1;
    }
    return Philox{{c0, c1, c2, c3}};
}

// strictly inside (0, 1): see the head of this file
__device__ __forceinline__ double hmc_uniform(uint32_t wa, uint32_t wb) {
    const double k = (double)(wa >> 5) * 67108864. + (double)(wb >> 6);
    const double u = (k + 0.5) * 0x1p-53;
    return u < 0x1.fffffffffffffp-1 ? u : 0x1.fffffffffffffp-1;
}

// whether `flag` holds on any lane of this lane's group
template <int G>
__device__ __forceinline__ bool group_any(bool flag, int lane, int i) {
    const unsigned long long all = __ballot(flag);
    return ((all >> (lane - i)) & (G == 32 ? 0xffffffffull : (1ull << G) - 1ull)) != 0ull;
}

// sum_i z_i z_i with i ascending, from 0., every lane of the group alike
template <int G>
__device__ __forceinline__ double group_square(double z, int n) {
    const double q = z * z;
    double s = 0.;
    for (int j = 0; j < n; ++j) s = s + group_value<G>(q, j);
    return s;
}

template <int G>
__global__ __launch_bounds__(lm_threads(G)) void hmc_step_kernel(const HmcArgs a) {
    constexpr int S = G + 1, FPW = 64 / G, WAVES = lm_threads(G) / 64;
    __shared__ double lds[WAVES * 64 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & (G - 1), f = lane / G, n = a.ndim;
    const long long b = ((long long)blockIdx.x * WAVES + wave) * FPW + f;
    double* const L = lds + (wave * FPW + f) * (G * S);
    const bool chain = b < a.B, live = chain && i < n;
    const bool closing = a.t_close >= 0, opening = a.t_open >= 0;      // the same for every lane of the launch

    int status = 1, nacc = 0, nout = 0, out = 0;
    double chi = 0., chit = 0., h0 = 0., eps = 0., step = 0.;
    if (chain) {
        status = a.status[b], nacc = a.naccepted[b], nout = a.nout[b], out = a.out[b];
        chi = a.chi2[b], chit = a.chi2_t[b], h0 = a.h0[b], eps = a.eps[b], step = a.step[b];
    }
    const bool frozen = status != 0;
    double xv = 0., gv = 0., zv = 0., xtv = 0., gtv = 0., lo = 0., hi = 0.;
    if (live) {
        xv = a.x[b * n + i], gv = a.grad[b * n + i], zv = a.z[b * n + i], xtv = a.xt[b * n + i], gtv = a.grad_t[b * n + i];
        lo = a.lo[i], hi = a.hi[i];
    }
    if (chain)
        for (int e = i; e < n * n; e += G) L[(e / n) * S + e % n] = a.factor[b * n * n + e];
    cp::wave_lds_phase();
    const double lii = live ? L[i * S + i] : 1.;

    double nextv = xv;      // rule 1, a close without an open, a failed open
    bool accept = false;
    if (closing || !opening) {      // the trial's kick: a whole one inside a trajectory, half a one at its end
        const double y = lm_forward<G>(L, i, n, lii, gtv, 0);
        const double ke = closing ? 0.5 * eps : eps;
        if (!frozen && !out) zv = zv + ke * y;
    }
    if (!closing && !opening) {      // rule 2
        const double v = lm_backward<G>(L, i, n, lii, zv, 0);
        const double cand = xtv + eps * v;
        const bool leaves = group_any<G>(live && !(lm_finite(cand) && cand >= lo && cand <= hi), lane, i);
        if (!frozen) {
            nextv = out || leaves ? xtv : cand;
            if (leaves) out = 1;
        }
    }
    if (closing) {      // rule 3
        const double k1 = 0.5 * group_square<G>(zv, n);
        const double h1 = 0.5 * chit + k1;
        const Philox w = philox4x32_10((uint32_t)b, (uint32_t)((unsigned long long)b >> 32), (uint32_t)a.t_close, 16u, (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
        const double e = -log(hmc_uniform(w.w[2], w.w[3]));
        if (!frozen) {
            if (out) ++nout;
            else accept = lm_finite(chit) && lm_finite(h1) && h1 - h0 < e;
        }
        if (accept) {
            xv = xtv, gv = gtv, chi = chit, ++nacc;
            if (live) a.x[b * n + i] = xv, a.grad[b * n + i] = gv;
        }
        if (a.sample) {
            if (live) a.sample[b * n + i] = xv;
            if (chain && i == 0) a.sample_chi2[b] = chi;
        }
        nextv = xv;
    }
    if (opening) {      // rule 4
        const bool good = lm_finite(step) && step > 0.;
        const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32), b0 = (uint32_t)b, b1 = (uint32_t)((unsigned long long)b >> 32), t = (uint32_t)a.t_open;
        const Philox w = philox4x32_10(b0, b1, t, (uint32_t)(i >> 1), k0, k1);
        const double r = sqrt(-2. * log(hmc_uniform(w.w[0], w.w[1])));
        const double angle = 6.283185307179586 * hmc_uniform(w.w[2], w.w[3]);
        const double drawn = i & 1 ? r * sin(angle) : r * cos(angle);
        const Philox wj = philox4x32_10(b0, b1, t, 16u, k0, k1);
        const double uj = hmc_uniform(wj.w[0], wj.w[1]);
        const double eps_new = step * (1. + a.jitter * (2. * uj - 1.));
        const double h0_new = 0.5 * chi + 0.5 * group_square<G>(drawn, n);
        const double y = lm_forward<G>(L, i, n, lii, gv, 0);
        const double z_new = drawn + (0.5 * eps_new) * y;
        const double v = lm_backward<G>(L, i, n, lii, z_new, 0);
        const double cand = xv + eps_new * v;
        const bool leaves = group_any<G>(live && !(lm_finite(cand) && cand >= lo && cand <= hi), lane, i);
        if (!frozen) {
            if (!good) {
                status = 3;
            } else {
                zv = z_new, eps = eps_new, h0 = h0_new, out = leaves ? 1 : 0;
                nextv = leaves ? xv : cand;
            }
        }
    }

    if (live) {
        a.next[b * n + i] = nextv;
        if (!frozen) a.z[b * n + i] = zv;
    }
    if (chain && !frozen && i == 0) {
        a.chi2[b] = chi, a.status[b] = status, a.naccepted[b] = nacc, a.nout[b] = nout;
        a.h0[b] = h0, a.eps[b] = eps, a.out[b] = out;
    }
}

template <int G>
__global__ __launch_bounds__(lm_threads(G)) void hmc_factor_kernel(const long long B, const int n, const double* metric, double* factor, int* status) {
    constexpr int S = G + 1, FPW = 64 / G, WAVES = lm_threads(G) / 64;
    __shared__ double lds[WAVES * 64 * S];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & (G - 1), f = lane / G;
    const long long b = ((long long)blockIdx.x * WAVES + wave) * FPW + f;
    double* const L = lds + (wave * FPW + f) * (G * S);
    const bool chain = b < B, live = chain && i < n;
    if (chain)
        for (int e = i; e < n * n; e += G) L[(e / n) * S + e % n] = metric[b * n * n + e];
    cp::wave_lds_phase();
    double lii;
    const int bad = lm_factor<G>(L, i, n, 0u, live ? L[i * S + i] : 1., lii);
    if (live)
        for (int j = 0; j < n; ++j) factor[b * n * n + (long long)i * n + j] = j <= i ? L[i * S + j] : 0.;
    if (chain && bad && i == 0) status[b] = 3;
}

// what the entry points check first, in this order; *per_workgroup: chains of a workgroup
int hmc_front(const char* who, long long B, int ndim, int* G, int* per_workgroup) {
    if (B < 0 || ndim < 1) return cp::fail(CP_EINVAL, "%s: %lld chains of %d parameters", who, B, ndim);
    if (ndim > 32) return cp::fail(CP_EUNSUPPORTED, "%s: %d parameters (at most 32)", who, ndim);
    *G = cp::lm_lanes_of(ndim);
    *per_workgroup = lm_threads(*G) / *G;
    if (B > 0x7fffffffLL * *per_workgroup)
        return cp::fail(CP_EUNSUPPORTED, "%s: %lld chains of %d parameters (at most 2^31 - 1 workgroups of %d chains)", who, B, ndim, *per_workgroup);
    return CP_OK;
}

}  // namespace

extern "C" int cp_hmc_factor(long long B, int ndim, const double* d_metric, double* d_factor, int* d_status, int device, void* stream) {
    int G, per;
    const int status = hmc_front("cp_hmc_factor", B, ndim, &G, &per);
    if (status != CP_OK) return status;
    if (B == 0) return CP_OK;
    if (!d_metric || !d_factor || !d_status) return cp::fail(CP_EINVAL, "cp_hmc_factor: null pointer");
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_hmc_factor: cannot select device %d", device);
    const unsigned grid = (unsigned)((B + per - 1) / per);
    cp::Launches on("cp_hmc_factor", stream);
    switch (G) {
        case 1: on.run<hmc_factor_kernel<1>>(grid, lm_threads(1), 0, B, ndim, d_metric, d_factor, d_status); break;
        case 2: on.run<hmc_factor_kernel<2>>(grid, lm_threads(2), 0, B, ndim, d_metric, d_factor, d_status); break;
        case 4: on.run<hmc_factor_kernel<4>>(grid, lm_threads(4), 0, B, ndim, d_metric, d_factor, d_status); break;
        case 8: on.run<hmc_factor_kernel<8>>(grid, lm_threads(8), 0, B, ndim, d_metric, d_factor, d_status); break;
        case 16: on.run<hmc_factor_kernel<16>>(grid, lm_threads(16), 0, B, ndim, d_metric, d_factor, d_status); break;
        default: on.run<hmc_factor_kernel<32>>(grid, lm_threads(32), 0, B, ndim, d_metric, d_factor, d_status); break;
    }
    return on.status();
}

extern "C" int cp_hmc_step(long long B, int ndim, long long t_close, long long t_open, double* d_x, double* d_grad, double* d_chi2, int* d_status, int* d_naccepted,
                           int* d_nout, double* d_z, double* d_h0, double* d_eps, int* d_out, const double* d_xt, const double* d_grad_t, const double* d_chi2_t,
                           const double* d_factor, const double* d_lo, const double* d_hi, const double* d_step, double jitter, unsigned long long seed,
                           double* d_next, double* d_sample, double* d_sample_chi2, int device, void* stream) {
    int G, per;
    const int status = hmc_front("cp_hmc_step", B, ndim, &G, &per);
    if (status != CP_OK) return status;
    if (t_close >= (1LL << 32) || t_open >= (1LL << 32))
        return cp::fail(CP_EUNSUPPORTED, "cp_hmc_step: trajectories %lld and %lld (below 2^32)", t_close, t_open);
    if (B == 0) return CP_OK;
    if (!d_x || !d_grad || !d_chi2 || !d_status || !d_naccepted || !d_nout || !d_z || !d_h0 || !d_eps || !d_out || !d_xt || !d_grad_t || !d_chi2_t || !d_factor || !d_lo ||
        !d_hi || !d_step || !d_next || !d_sample != !d_sample_chi2)
        return cp::fail(CP_EINVAL, "cp_hmc_step: null pointer");
    if (!(jitter >= 0. && jitter < 1.)) return cp::fail(CP_EINVAL, "cp_hmc_step: jitter = %g (in [0, 1))", jitter);
    cp::DeviceScope scope(device);
    if (!scope.ok()) return cp::fail(CP_EDEVICE, "cp_hmc_step: cannot select device %d", device);
    const HmcArgs a{B,    ndim,     t_close,  t_open,   d_x,  d_grad, d_chi2, d_status, d_naccepted, d_nout, d_z,    d_h0,     d_eps,
                    d_out, d_xt,    d_grad_t, d_chi2_t, d_factor, d_lo, d_hi,  d_step,   jitter,      seed,   d_next, d_sample, d_sample_chi2};
    const unsigned grid = (unsigned)((B + per - 1) / per);
    cp::Launches on("cp_hmc_step", stream);
    switch (G) {
        case 1: on.run<hmc_step_kernel<1>>(grid, lm_threads(1), 0, a); break;
        case 2: on.run<hmc_step_kernel<2>>(grid, lm_threads(2), 0, a); break;
        case 4: on.run<hmc_step_kernel<4>>(grid, lm_threads(4), 0, a); break;
        case 8: on.run<hmc_step_kernel<8>>(grid, lm_threads(8), 0, a); break;
        case 16: on.run<hmc_step_kernel<16>>(grid, lm_threads(16), 0, a); break;
        default: on.run<hmc_step_kernel<32>>(grid, lm_threads(32), 0, a); break;
    }
    return on.status();
}
