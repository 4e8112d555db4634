// Host access to the table interpolation of csrc/cp_interp_table.h for the CPU tests (TEST HARNESS ONLY): the law of a table's knots as the library
// finds it, and the kernel's per-sample code run over an array of samples on an exact-size pair table.  tests/test_interp_table_host.py checks both
// against numpy.interp; tests/host_san/san_driver.cpp runs them under the sanitizers.  tests/test_interp_truth_host.py runs the kernel's four-in-flight loop
// (cpit::interp_samples) for a small grid of threads.  Build with -ffp-contract=off (numpy's arithmetic).
#include <vector>

#include "../../cosmoprimo_amd/csrc/cp_interp_table.h"

extern "C" int emu_interp_law(long long n, const double* x, int* law, long long* first, double* a, double* b) {
    const cpit::Law L = cpit::find_law(x, n);
    *law = L.law; *first = L.first; *a = L.a; *b = L.b;
    return 0;
}

// out[i] = numpy.interp(xq[i], x, f) through the law (law 1 or 2; given, so that a test may hand over a law the table does not follow: the walk
// must still end on numpy's interval); returns 1 when a sample lies outside the table or is NaN
extern "C" int emu_interp_apply(long long n, const double* x, const double* f, int law, long long first, double a, double b, long long nx, const double* xq,
                                double* out) {
    std::vector<cpit::Pair> xf((size_t)n);      // exactly n pairs: a walk past either end is a heap overflow for the sanitizer
    for (long long i = 0; i < n; ++i) xf[(size_t)i] = cpit::Pair{x[i], f[i]};
    bool outside = false;
    for (long long i = 0; i < nx; ++i)
        out[i] = law == 2 ? cpit::interp_sample<2>(xf.data(), n, first, a, b, x[0], x[first], x[n - 1], xq[i], &outside)
                          : cpit::interp_sample<1>(xf.data(), n, first, a, b, x[0], x[first], x[n - 1], xq[i], &outside);
    return outside ? 1 : 0;
}

// The four-in-flight loop of interp_table_kernel (csrc/cp_interp.hip) run thread by thread for a grid of T threads: thread t takes i = t, t + 4 T, ... and
// holds the samples i + u T, u = 0 ... 3, of a trip together (cpit::interp_samples<LAW, 4>); a slot is live while i + u T < nx, a dead slot reads sample i and
// stores nothing.  A thread's flag is its own, the result their OR (the kernel's atomicOr).  With T = 8 a few dozen samples reach every slot and trip edge.
namespace {

template <int LAW, typename real>
int samples_loop(const cpit::Pair* xf, long long n, long long first, double a, double b, long long nx, const real* x, real* out, long long T) {
    const double x0 = xf[0].x, xn = xf[n - 1].x;
    const double xfirst = xf[first].x;
    constexpr int U = 4;
    const long long stride = T;
    bool any = false;
    for (long long t = 0; t < T; ++t) {
        bool outside = false;
        for (long long i = t; i < nx; i += U * stride) {
            double v[U], r[U];
            bool live[U];
            for (int u = 0; u < U; ++u) {
                live[u] = i + u * stride < nx;
                v[u] = (double)x[live[u] ? i + u * stride : i];
            }
            cpit::interp_samples<LAW, U>(xf, n, first, a, b, x0, xfirst, xn, v, live, r, &outside);
            for (int u = 0; u < U; ++u)
                if (live[u]) out[i + u * stride] = (real)r[u];
        }
        any |= outside;
    }
    return any ? 1 : 0;
}

template <typename real>
int samples_entry(long long n, const double* x, const double* f, int law, long long first, double a, double b, long long nx, const real* xq, real* out, long long T) {
    std::vector<cpit::Pair> xf((size_t)n);
    for (long long i = 0; i < n; ++i) xf[(size_t)i] = cpit::Pair{x[i], f[i]};
    return law == 2 ? samples_loop<2, real>(xf.data(), n, first, a, b, nx, xq, out, T) : samples_loop<1, real>(xf.data(), n, first, a, b, nx, xq, out, T);
}

}  // namespace

extern "C" int emu_interp_samples(long long n, const double* x, const double* f, int law, long long first, double a, double b, long long nx, const double* xq,
                                  double* out, long long T) {
    return samples_entry<double>(n, x, f, law, first, a, b, nx, xq, out, T);
}

extern "C" int emu_interp_samples_f32(long long n, const double* x, const double* f, int law, long long first, double a, double b, long long nx, const float* xq,
                                      float* out, long long T) {
    return samples_entry<float>(n, x, f, law, first, a, b, nx, xq, out, T);
}
