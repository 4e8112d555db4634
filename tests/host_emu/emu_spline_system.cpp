// Host access to csrc/cp_spline_system.h for the CPU tests (TEST HARNESS ONLY): the elimination factors of a spline's system for the second
// derivatives, the halo its sweeps need, and the intervals and weights of queries, as plain arrays.  tests/test_spline_system_host.py checks them.
#include "../../cosmoprimo_amd/csrc/cp_spline_system.h"

extern "C" int emu_spline_increasing(int n, const double* x) { return cpss::increasing(n, x) ? 1 : 0; }

// ends: 0 natural, 1 clamped, 2 not-a-knot.  h, inv, c, q: (n); fix: (4).  Returns the halo (above 128: the plans refuse the knots).
extern "C" int emu_spline_factors(int n, const double* x, int ends, double* h, double* inv, double* c, double* q, double* fix) {
    const cpss::System s = cpss::factors(n, x, ends == 0 ? cpss::NATURAL : (ends == 1 ? cpss::CLAMPED : cpss::NOT_A_KNOT));
    for (int i = 0; i < n; ++i) {
        h[i] = s.h[i];
        inv[i] = s.inv[i];
        c[i] = s.c[i];
        q[i] = s.q[i];
    }
    for (int i = 0; i < 4; ++i) fix[i] = s.fix[i];
    return cpss::halo_of(s);
}

// qj: (nq) intervals, -1 outside; qw: (nq, 4) weights, zeros where qj is -1
extern "C" void emu_spline_queries(int n, const double* x, int nq, const double* xq, int extrapolate, int* qj, double* qw) {
    const std::vector<double> h = cpss::spacings(n, x);
    for (int k = 0; k < nq; ++k) {
        qj[k] = cpss::interval_of(n, x, xq[k], extrapolate != 0);
        for (int i = 0; i < 4; ++i) qw[4 * k + i] = 0.;
        if (qj[k] >= 0) cpss::weights_of(x, h.data(), qj[k], xq[k], qw + 4 * k);
    }
}
