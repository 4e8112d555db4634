// cp_spline_system.h -- the host arithmetic of the spline plans that solve for the second derivatives M at the knots (cp_spline_rows_plan_create,
// cp_splice_plan_create, cpsu::build), written once: the tridiagonal system and its elimination factors, how far a sweep of that elimination
// remembers its start, and a query's interval and weights.  Plain C++, no HIP header: compiled by hipcc into the library and by g++ for the CPU tests
// (tests/host_emu/emu_spline_system.cpp).  The sweeps that use the factors are in cp_spline_sweeps.h.  How a plan lays the factors out in its table
// is the plan's own business (the slot layouts differ), and so is the one place where the two plans round differently: 6. / h[i] in the rows plan,
// 6. * (1. / h[i]) in the splice plan.
#pragma once

#include <algorithm>
#include <cmath>
#include <vector>

namespace cpss {

enum Ends { NATURAL, CLAMPED, NOT_A_KNOT };

inline bool increasing(int n, const double* x) {
    for (int i = 0; i + 1 < n; ++i)
        if (!(x[i + 1] > x[i])) return false;
    return true;
}

// h_i = x_{i+1} - x_i, the last one repeated (it never multiplies anything that is used: s_{n-1} = 0, and M_{n-1} has no successor)
inline std::vector<double> spacings(int n, const double* x) {
    std::vector<double> h(n);
    for (int i = 0; i + 1 < n; ++i) h[i] = x[i + 1] - x[i];
    h[n - 1] = h[n - 2];
    return h;
}

// The system sub_i M_{i-1} + diag_i M_i + sup_i M_{i+1} = 6 (s_i - s_{i-1}), s_i = (y_{i+1} - y_i) / h_i, s_{-1} = s_{n-1} = 0, and the factors of its
// elimination: inv_i = 1 / pivot_i, c_i = sup_i / pivot_i (what the back substitution multiplies by), q_i = sub_i / pivot_i (the forward sweep).
// Interior rows: sub_i = h_{i-1}, diag_i = 2 (h_{i-1} + h_i), sup_i = h_i.
// clamped: 2 h_0 M_0 + h_0 M_1 = 6 s_0 and its mirror image; natural: M_0 = M_{n-1} = 0 (inv = 0 in the outermost rows, which are not equations of the
// system); not-a-knot (n >= 5): the outermost unknowns eliminated through M_0 = fix[0] M_1 + fix[1] M_2 and M_{n-1} = fix[2] M_{n-2} + fix[3] M_{n-3}
// (continuity of the third derivative at the second and the last-but-one knot; inv = 0 again, the ends filled in afterwards), which modifies rows 1 and n - 2.
struct System {
    std::vector<double> h, inv, c, q;
    double fix[4] = {0., 0., 0., 0.};
};

inline System factors(int n, const double* x, Ends ends) {
    System s;
    s.h = spacings(n, x);
    const std::vector<double>& h = s.h;
    std::vector<double> sub(n), diag(n), sup(n);
    for (int i = 1; i < n - 1; ++i) {
        sub[i] = h[i - 1];
        diag[i] = 2. * (h[i - 1] + h[i]);
        sup[i] = h[i];
    }
    sub[0] = 0.; diag[0] = 2. * h[0]; sup[0] = h[0];
    sub[n - 1] = h[n - 2]; diag[n - 1] = 2. * h[n - 2]; sup[n - 1] = 0.;
    const bool open_ends = ends != CLAMPED;
    if (ends == NOT_A_KNOT) {
        double* fix = s.fix;
        fix[0] = 1. + h[0] / h[1]; fix[1] = -h[0] / h[1];
        fix[2] = 1. + h[n - 2] / h[n - 3]; fix[3] = -h[n - 2] / h[n - 3];
        diag[1] += h[0] * fix[0]; sup[1] += h[0] * fix[1]; sub[1] = 0.;
        diag[n - 2] += h[n - 2] * fix[2]; sub[n - 2] += h[n - 2] * fix[3]; sup[n - 2] = 0.;
    }
    s.inv.resize(n); s.c.resize(n); s.q.resize(n);
    s.inv[0] = open_ends ? 0. : 1. / diag[0];
    s.c[0] = sup[0] * s.inv[0];
    s.q[0] = 0.;
    for (int i = 1; i < n; ++i) {
        s.inv[i] = (open_ends && i == n - 1) ? 0. : 1. / (diag[i] - sub[i] * s.c[i - 1]);
        s.c[i] = sup[i] * s.inv[i];
        s.q[i] = sub[i] * s.inv[i];
    }
    return s;
}

// How far a sweep remembers its start -- the forward one by q_i per knot, the backward one by c_i --: the smallest multiple of 8 knots after which
// less than 1e-18 is left anywhere (or the first one >= n: nothing to forget).  Above 128 the search stops; the callers refuse such knots.
inline int halo_of(const System& s) {
    const int n = (int)s.q.size();
    for (int halo = 8;; halo += 8) {
        if (halo > 128) return halo;
        double worst = 0.;
        for (int i = halo; i < n; ++i) {
            double f = 1., b = 1.;
            for (int t = 0; t < halo; ++t) {
                f *= std::fabs(s.q[i - t]);
                b *= std::fabs(s.c[i - t - 1]);
            }
            worst = std::max(worst, std::max(f, b));
        }
        if (worst < 1e-18) return halo;
    }
}

// the interval j (x_j <= v, the last one for v = x_{n-1}) of a query; -1 for one outside the knots that is not evaluated: a NaN always, one beyond an
// end unless `extrapolate` continues the cubic of the end interval
inline int interval_of(int n, const double* x, double v, bool extrapolate) {
    if (!(v >= x[0] && v <= x[n - 1]) && !(extrapolate && v == v)) return -1;
    const int j = (int)(std::upper_bound(x, x + n, v) - x) - 1;
    return j > n - 2 ? n - 2 : (j < 0 ? 0 : j);
}

// w[4] = A, B, (A^3 - A) h^2 / 6, (B^3 - B) h^2 / 6 of the query v in interval j: the spline there is A y_j + B y_{j+1} + w[2] M_j + w[3] M_{j+1}
inline void weights_of(const double* x, const double* h, int j, double v, double* w) {
    const double a = (x[j + 1] - v) / h[j], b = (v - x[j]) / h[j];
    w[0] = a;
    w[1] = b;
    w[2] = (a * a * a - a) * (h[j] * h[j]) / 6.;
    w[3] = (b * b * b - b) * (h[j] * h[j]) / 6.;
}

}  // namespace cpss
