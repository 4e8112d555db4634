// tools/fftlog_microbench.hip -- diagnostic timing harness for the flagship kernel instantiation
// (NP = 4096, zero-padded, cropped).  Built once per -DCP_ABLATE=<mask> (see cp_fft_core.h); prints the
// average kernel time so that differences between masks show what the kernel waits on.  Not part of the library.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DCP_ABLATE=0 -o mb0 tools/fftlog_microbench.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../cosmoprimo_amd/csrc/cp_fftlog_kernel.h"

using namespace cpfft;

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e = (x);                                                       \
        if (e != hipSuccess) {                                                    \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));                \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

#ifndef MB_NP
#define MB_NP 4096
#endif
#ifndef MB_P
#define MB_P 16
#endif
#ifndef MB_GENERIC  // 1: the generic front / back ends; 2: the HALF front end with 'edge' padding; 0: HALF_ZERO (flagship)
#define MB_GENERIC 0
#endif
#ifndef MB_STREAM_ROWS  // non-temporal row accesses, bit 0 loads, bit 1 stores (3: what cp_fftlog_execute selects for launches of this size)
#define MB_STREAM_ROWS 3
#endif
#ifndef MB_WGS_PER_CU
#define MB_WGS_PER_CU 2
#endif

int main(int argc, char** argv) {
    constexpr int NP = MB_NP, P = MB_P, N = NP / 2;
    const long long nbatch = argc > 1 ? atoll(argv[1]) : 100000;
    const int reps = argc > 2 ? atoi(argv[2]) : 20;
    const int warm = argc > 3 ? atoi(argv[3]) : 300;  // (a counter pass needs no settled clock: 0)
    std::vector<double> in((size_t)nbatch * N), pre(NP), post(NP), u(2 * (NP / 2 + 1));
    for (size_t i = 0; i < in.size(); ++i) in[i] = 1. + 1e-3 * (double)(i % 977);
    for (int i = 0; i < NP; ++i) pre[i] = 1. + 1e-4 * i, post[i] = 1. - 1e-5 * i;
    for (int i = 0; i <= NP / 2; ++i) u[2 * i] = 0.6, u[2 * i + 1] = (i == 0 || i == NP / 2) ? 0. : 0.8;
    std::vector<cplx> tw, ul(NP);
    build_twiddles<NP, P>(tw);
    build_u_layout<NP, P>(u.data(), ul.data());
    double *d_in, *d_out, *d_pre, *d_post;
    cplx *d_u, *d_tw;
    CHECK(hipMalloc(&d_in, in.size() * 8));
    CHECK(hipMalloc(&d_out, in.size() * 8));
    CHECK(hipMalloc(&d_pre, NP * 8));
    CHECK(hipMalloc(&d_post, NP * 8));
    CHECK(hipMalloc(&d_u, NP * 16));
    CHECK(hipMalloc(&d_tw, tw.size() * 16));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_pre, pre.data(), NP * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_post, post.data(), NP * 8, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_u, ul.data(), NP * 16, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_tw, tw.data(), tw.size() * 16, hipMemcpyHostToDevice));
    FftlogArgs A;
    A.in = d_in; A.out = d_out; A.nbatch = nbatch; A.nker = 1; A.n = N; A.in_left = NP / 4; A.out_off = NP / 4; A.n_out = N;
    A.ext_l = A.ext_r = MB_GENERIC == 2 ? 1 : 0; A.val_l = A.val_r = 0.; A.stream_rows = MB_STREAM_ROWS; A.pre = d_pre; A.post = d_post; A.u = d_u; A.tw = d_tw;
#if defined(CP_STAMPS)
    unsigned long long* d_stamp;
    const size_t nstamp = (size_t)2048 * 8 * 16;
    CHECK(hipMalloc(&d_stamp, nstamp * 8));
    CHECK(hipMemset(d_stamp, 0, nstamp * 8));
    A.val_stamp = reinterpret_cast<double*>(d_stamp);
#endif
    int ncu = 0;
    CHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, 0));
    const int grid = ncu * MB_WGS_PER_CU;
#if defined(CP_STAMPS)
    // barrier log (cp_fftlog_kernel.h): every launch rewrites all of it, the last one is read back
    const int log_pairs = (int)(((nbatch + 1) / 2 + grid - 1) / grid);
    const size_t log_stride = 2 + 2 * (size_t)log_pairs;
    CHECK(hipMalloc(&A.bar_log, (size_t)grid * log_stride * 8));
    CHECK(hipMemset(A.bar_log, 0, (size_t)grid * log_stride * 8));
    A.bar_log_pairs = log_pairs;
#endif
    CHECK(hipMalloc(&A.cu_ticket, CP_CU_SLOTS * sizeof(unsigned)));
    CHECK(hipMemset(A.cu_ticket, 0, CP_CU_SLOTS * sizeof(unsigned)));
    constexpr int T = Plan<NP, P>::T, lds = Fftlog<NP, P>::LDS_BYTES + CP_BALANCE_LDS;  // (the ticket word: the headline variant uses it)
#if MB_GENERIC == 2  // 'edge' padding through the HALF front end
    auto kern = fftlog_kernel<NP, P, IN_HALF, OUT_HALF>;
#elif MB_GENERIC
    auto kern = fftlog_kernel<NP, P, IN_GENERIC, OUT_GENERIC>;
#else
    auto kern = fftlog_kernel<NP, P, IN_HALF_ZERO, OUT_HALF>;
#endif
    if (lds > 64 * 1024) CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    // reach the sustained device state first: the first tens of milliseconds of load after an idle period run ~10 % slower (clock ramp)
    for (int i = 0; i < warm; ++i) hipLaunchKernelGGL(kern, dim3(grid), dim3(T), lds, 0, A);
    CHECK(hipDeviceSynchronize());
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(kern, dim3(grid), dim3(T), lds, 0, A);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    ms /= reps;
    printf("ablate=%d np=%d grid=%d rows=%lld  %.4f ms  %.2f Mtransforms/s  %.0f GB/s\n", CP_ABLATE, NP, grid, nbatch, ms, nbatch / ms * 1e-3,
           nbatch * 16. * N / ms * 1e-6);
#if defined(CP_STAMPS)
    {
        constexpr int NPH = Fftlog<NP, P>::NPH, W = T / 64, K = 2 * NPH + 1 + 8;
        std::vector<unsigned long long> h((size_t)grid * W * K);
        CHECK(hipMemcpy(h.data(), d_stamp, h.size() * 8, hipMemcpyDeviceToHost));
        std::vector<double> avg(K, 0.);
        for (size_t i = 0; i < (size_t)grid * W; ++i)
            for (int k = 0; k < K; ++k) avg[k] += (double)h[i * K + k] / ((double)grid * W);
        const double npw = (double)((nbatch + 1) / 2) / grid;  // pairs per workgroup
        printf("per pair per wave [s_memtime ticks]: ");
        for (int ph = 0; ph < NPH; ++ph) printf(" work%d=%.0f bar%d=%.0f |", ph, avg[2 * ph] / npw, ph, avg[2 * ph + 1] / npw);
        printf(" total=%.0f (whole kernel %.0f ticks = %.4f ms -> %.1f MHz)\n", avg[2 * NPH] / npw, avg[2 * NPH], ms, avg[2 * NPH] / ms * 1e-3);
        printf("fine: reads landed ph1..4 = %.0f %.0f %.0f %.0f | U applied %.0f | last twiddles applied %.0f | barrier in last phase %.0f\n",
               avg[2 * NPH + 2] / npw, avg[2 * NPH + 3] / npw, avg[2 * NPH + 4] / npw, avg[2 * NPH + 5] / npw, avg[2 * NPH + 6] / npw,
               avg[2 * NPH + 7] / npw, avg[2 * NPH + 8] / npw);
        // ---- the same by wave index within the workgroup: do the four waves of a workgroup reach the LDS together? -----------
        if constexpr (NPH == 5) {
            const long long npairs_all = (nbatch + 1) / 2;
            std::vector<double> byw((size_t)W * K, 0.);
            std::vector<double> simd((size_t)W * 4, 0.);
            int nwg = 0;
            for (int b = 0; b < grid && b < npairs_all; ++b) {
                const double np_b = (double)((npairs_all - b + grid - 1) / grid);
                for (int w = 0; w < W; ++w) {
                    const unsigned long long* q = &h[((size_t)b * W + w) * K];
                    for (int k = 0; k < K; ++k) byw[(size_t)w * K + k] += (double)q[k] / np_b;
                    simd[(size_t)w * 4 + (q[2 * NPH + 1] & 3)] += 1.;
                }
                ++nwg;
            }
            printf("by wave index within the workgroup (skew=%d order=0x%x; ticks per pair, mean over %d workgroups):\n", CP_WAVE_SKEW, CP_WAVE_ORDER, nwg);
            printf("  wave | on SIMD 0 1 2 3 [share]   | reads landed ph1   ph2   ph3   ph4 | work0 work1 work2 work3 work4 | bar0  bar3 | pair\n");
            for (int w = 0; w < W && nwg; ++w) {
                const double* a = &byw[(size_t)w * K];
                printf("  %4d | %.2f %.2f %.2f %.2f             | %16.0f %5.0f %5.0f %5.0f | %5.0f %5.0f %5.0f %5.0f %5.0f | %5.0f %5.0f | %.0f\n", w,
                       simd[w * 4] / nwg, simd[w * 4 + 1] / nwg, simd[w * 4 + 2] / nwg, simd[w * 4 + 3] / nwg, a[2 * NPH + 2] / nwg, a[2 * NPH + 3] / nwg,
                       a[2 * NPH + 4] / nwg, a[2 * NPH + 5] / nwg, a[0] / nwg, a[2] / nwg, a[4] / nwg, a[6] / nwg, a[8] / nwg, a[1] / nwg, a[7] / nwg,
                       a[2 * NPH] / nwg);
            }
        }
        // ---- offset between the workgroups that share a CU (last launch) ---------------------------------------------------
        std::vector<unsigned long long> lg((size_t)grid * log_stride);
        CHECK(hipMemcpy(lg.data(), A.bar_log, lg.size() * 8, hipMemcpyDeviceToHost));
        const long long npairs = (nbatch + 1) / 2;
        auto pairs_of = [&](int b) { return (int)((npairs - b + grid - 1) / grid); };
        std::map<unsigned long long, std::vector<int>> by_cu;
        for (int b = 0; b < grid && b < npairs; ++b) by_cu[lg[(size_t)b * log_stride]].push_back(b);
        int share[4] = {0, 0, 0, 0};  // CUs holding 1, 2, 3, more workgroups
        for (auto& kv : by_cu) share[std::min<size_t>(kv.second.size(), 4) - 1]++;
        // period of a pair and of a phase from the log itself
        double period = 0;
        long long nper = 0;
        for (int b = 0; b < grid && b < npairs; ++b) {
            const int np_b = pairs_of(b);
            if (np_b < 2) continue;
            const unsigned long long* q = &lg[(size_t)b * log_stride + 2];
            period += (double)(q[2 * (np_b - 1)] - q[0]) / (np_b - 1);
            ++nper;
        }
        period = nper ? period / nper : 1.;
        const double phase_len = period / NPH;
        constexpr int NB = 10;
        long long h_pair[NB] = {0}, h_phase[NB] = {0}, nobs = 0;
        const int marks[] = {0, 1, 2, 5, 10, 20, 50, 97};
        double abs_at[8] = {0}, fold_at[8] = {0};
        long long n_at[8] = {0};
        for (auto& kv : by_cu) {
            if (kv.second.size() != 2) continue;
            const int a = kv.second[0], b = kv.second[1];
            const int np_ab = std::min(pairs_of(a), pairs_of(b));
            for (int k = 0; k < np_ab; ++k)
                for (int w = 0; w < 2; ++w) {  // both barriers of the pair
                    const double d = (double)(long long)(lg[(size_t)a * log_stride + 2 + 2 * k + w] - lg[(size_t)b * log_stride + 2 + 2 * k + w]);
                    double fp = std::fmod(std::fabs(d), period) / period;        // in pairs, folded to [0, 1/2]
                    if (fp > 0.5) fp = 1. - fp;
                    double fh = std::fmod(std::fabs(d), phase_len) / phase_len;  // in phases, folded to [0, 1/2]
                    if (fh > 0.5) fh = 1. - fh;
                    h_pair[std::min(NB - 1, (int)(fp * 2 * NB))]++;
                    h_phase[std::min(NB - 1, (int)(fh * 2 * NB))]++;
                    ++nobs;
                    if (w == 0)
                        for (int m = 0; m < 8; ++m)
                            if (marks[m] == k) abs_at[m] += std::fabs(d), fold_at[m] += fh, n_at[m]++;
                }
        }
        // ---- do the two workgroups of a CU advance at the same rate?  (the last barrier of a workgroup's last pair = its end)
        double alone = 0, per_fast = 0, per_slow = 0, older_first = 0, t_fast = 0, t_slow = 0;
        long long h_alone[NB] = {0}, ncu2 = 0;
        for (auto& kv : by_cu) {
            if (kv.second.size() != 2) continue;
            int a = kv.second[0], b = kv.second[1];
            auto end_of = [&](int w) { return lg[(size_t)w * log_stride + 2 + 2 * (pairs_of(w) - 1) + 1]; };
            auto start_of = [&](int w) { return lg[(size_t)w * log_stride + 1]; };
            if (pairs_of(a) < 42 || pairs_of(b) < 42) continue;
            if (end_of(a) > end_of(b)) std::swap(a, b);  // a finishes first
            const unsigned long long t0 = std::min(start_of(a), start_of(b));
            const double T = (double)(end_of(b) - t0), fa = (double)(end_of(b) - end_of(a)) / T;
            alone += fa;
            h_alone[std::min(NB - 1, (int)(fa * 2 * NB))]++;
            auto per = [&](int w) { return (double)(lg[(size_t)w * log_stride + 2 + 2 * 40] - lg[(size_t)w * log_stride + 2 + 2 * 5]) / 35.; };
            per_fast += per(a), per_slow += per(b);
            t_fast += (double)(end_of(a) - t0), t_slow += T;
            older_first += start_of(a) <= start_of(b) ? 1. : 0.;
            ++ncu2;
        }
        if (ncu2) {
            printf("rates of the two workgroups of a CU (%lld CUs): the first to finish takes %.0f ticks, the other %.0f; the CU holds ONE workgroup for %.3f of its time\n",
                   ncu2, t_fast / ncu2, t_slow / ncu2, alone / ncu2);
            printf("  pair period over pairs 5..40: first finisher %.0f ticks, the other %.0f; the first finisher is the one that started first on %.2f of the CUs\n",
                   per_fast / ncu2, per_slow / ncu2, older_first / ncu2);
            printf("  share of CUs by the fraction of time spent with one workgroup, bins of 0.05 from 0:");
            for (int i = 0; i < NB; ++i) printf(" %.3f", (double)h_alone[i] / ncu2);
            printf("\n");
        }
        printf("CU sharing: %d CUs hold 1 workgroup, %d hold 2, %d hold 3, %d more | pair period %.0f ticks, phase %.0f\n", share[0], share[1], share[2],
               share[3], period, phase_len);
        printf("offset between the two workgroups of a CU, same pair index and barrier, %lld observations; share per bin, uniform = %.3f\n", nobs, 1. / NB);
        printf("  modulo a pair,  folded to [0, 1/2] pair,  bins of 1/%d:", 2 * NB);
        for (int i = 0; i < NB; ++i) printf(" %.3f", nobs ? (double)h_pair[i] / nobs : 0.);
        printf("\n  modulo a phase, folded to [0, 1/2] phase, bins of 1/%d:", 2 * NB);
        for (int i = 0; i < NB; ++i) printf(" %.3f", nobs ? (double)h_phase[i] / nobs : 0.);
        printf("\n  by pair index (first barrier): index / mean |offset| ticks / mean folded phase offset (uniform = 0.25):");
        for (int m = 0; m < 8; ++m)
            if (n_at[m]) printf("  %d / %.0f / %.3f", marks[m], abs_at[m] / n_at[m], fold_at[m] / n_at[m]);
        printf("\n");
        printf("JSON {\"ms\": %.4f, \"cus_with_2\": %d, \"first_finisher_ticks\": %.0f, \"other_ticks\": %.0f, \"one_workgroup_fraction\": %.3f, \"pair_ticks\": %.0f, \"reads_landed_ph1_3\": [%.0f, %.0f, %.0f], \"offset_mod_phase_hist\": [", ms, share[1], ncu2 ? t_fast / ncu2 : 0., ncu2 ? t_slow / ncu2 : 0.,
               ncu2 ? alone / ncu2 : 0., period,
               avg[2 * NPH + 2] / npw, avg[2 * NPH + 3] / npw, avg[2 * NPH + 4] / npw);
        for (int i = 0; i < NB; ++i) printf("%s%.4f", i ? ", " : "", nobs ? (double)h_phase[i] / nobs : 0.);
        printf("], \"offset_mod_pair_hist\": [");
        for (int i = 0; i < NB; ++i) printf("%s%.4f", i ? ", " : "", nobs ? (double)h_pair[i] / nobs : 0.);
        printf("]}\n");
    }
#endif
    return 0;
}
