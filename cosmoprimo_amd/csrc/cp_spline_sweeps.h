// cp_spline_sweeps.h -- the two sweeps of the segmented elimination of a spline's tridiagonal system in LDS, written once for spline_rows_kernel<R>
// (cp_spline_rows.hip) and splice_kernel (cp_bao.hip).  The factors they use come from cp_spline_system.h (host).
//
// A row's knot values lie in `buf` with the end values repeated beyond either end (so no index is ever clamped), and `coef[slot_of(i)]` holds
// (6 / h_i, 1 / pivot_i, h_{i-1} / pivot_i, h_i / pivot_i) of knot i.  A lane owns the S knots from `own` on.  The eliminated right-hand sides d, then
// the second derivatives M, take the places of the values in the same buffer.  Both sweeps start `halo` knots outside the lane's segment from zero: a
// sweep forgets where it started at the rate its factors decay, and the plan chose the halo so that 1e-18 of the start is left
// (cpss::halo_of).  The run-in stores nothing.
// The lanes of a row belong to ONE wave, which executes its LDS instructions in order; cp::wave_lds_phase keeps the compiler to that order.  The
// phases between the two sweeps and behind them stay with the caller, and so do its diagnostic switches.
#pragma once
#include <hip/hip_runtime.h>

#include "cp_internal.h"

namespace cpsweep {

// Forward: d_i = P_i - Q_i d_{i-1}, P_i = (sigma_i - sigma_{i-1}) / pivot_i, sigma_i = (y_{i+1} - y_i) 6 / h_i, Q_i = h_{i-1} / pivot_i: the dependent
// chain is one FMA per knot.  On return buf[own .. own + S) holds d.
template <int UNROLL, class SlotOf>
__device__ __forceinline__ void forward(const SlotOf& slot_of, double* buf, const double4* coef, int own, int S, int halo) {
    const double beyond = buf[own + S];      // the next segment's first knot, before its owner writes there
    const int start = own - halo;
    double y0 = buf[start], d = 0.;
    double sigma_m = (y0 - buf[start - 1]) * coef[slot_of(start - 1)].x;
#pragma unroll UNROLL
    for (int t = 0; t < halo; ++t) {             // towards the segment: nothing stored
        const int i = start + t;
        const double4 c = coef[slot_of(i)];
        const double yp = buf[i + 1];
        const double sigma = (yp - y0) * c.x;
        d = fma(-c.z, d, c.y * (sigma - sigma_m));
        sigma_m = sigma;
        y0 = yp;
    }
    cp::wave_lds_phase();      // run-ins done before the neighbours' knot values become d
#pragma unroll UNROLL
    for (int t = 0; t < S - 1; ++t) {
        const int i = own + t;
        const double4 c = coef[slot_of(i)];
        const double yp = buf[i + 1];
        const double sigma = (yp - y0) * c.x;
        d = fma(-c.z, d, c.y * (sigma - sigma_m));
        buf[i] = d;                              // (segments past the last knot: slots nobody uses)
        sigma_m = sigma;
        y0 = yp;
    }
    {
        const int i = own + S - 1;
        const double4 c = coef[slot_of(i)];
        const double sigma = (beyond - y0) * c.x;
        buf[i] = fma(-c.z, d, c.y * (sigma - sigma_m));
    }
}

// Back substitution, the same shape from the right: M_i = d_i - (h_i / pivot_i) M_{i+1} below knot `last`, the last knot of the row, and M_i = d_i from
// there on (beyond the last knot: M_last = d_last when the sweep gets there).  The caller has separated it from the forward sweep by a phase (d
// complete).  On return buf[own .. own + S) holds M; a phase before anyone gathers across segments.
template <int UNROLL, class SlotOf>
__device__ __forceinline__ void backward(const SlotOf& slot_of, double* buf, const double4* coef, int own, int S, int halo, int last) {
    double m = 0.;
    // the segment's last knot, named once for both loops on purpose: written out in each (own + S - 1 - t), the compiler folds the -1 into the counter
    // while the function still stands alone, which the old text, inside its kernel, did not do -- and spline_rows_kernel measured 0.5 % slower
    const int seg = own + S - 1;
#pragma unroll UNROLL
    for (int t = 0; t < halo; ++t) {
        const int i = seg + halo - t;
        const double d = buf[i];
        m = i >= last ? d : fma(-coef[slot_of(i)].w, m, d);
    }
    cp::wave_lds_phase();      // run-ins done before the neighbours' d become M
#pragma unroll UNROLL
    for (int t = 0; t < S; ++t) {
        const int i = seg - t;
        const double d = buf[i];
        m = i >= last ? d : fma(-coef[slot_of(i)].w, m, d);
        buf[i] = m;
    }
}

}  // namespace cpsweep
