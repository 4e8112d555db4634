// Host access to csrc/cp_math.h for the CPU tests (TEST HARNESS ONLY): the header compiled unchanged by g++ over tests/host_emu/stub/hip/hip_runtime.h
// (-Itests/host_emu/stub first, -ffp-contract=off so that only the fma() the header writes are fused), evaluated on an array with the switch of
// csrc/cp_math_eval.hip.  The forms built of rint / fma / ldexp alone give the device's bits; the hardware reciprocal and reciprocal-root estimates are
// stood in for by the exact value rounded to float, which is NOT bit-faithful (recip, rsqrt_pos, log_pos: the error is emulated, not the bits).
// tests/test_math_truth_host.py checks the result and the two tables against longdouble.
#include <hip/hip_runtime.h>

#include "../../cosmoprimo_amd/csrc/cp_math.h"

// kind: enum cp_math_function of include/cosmoprimo_amd.h.  Returns 0, or 1 for an unknown kind.
extern "C" int emu_math(int kind, const double* x, double* y, long long n) {
    if (kind < 0 || kind > 8) return 1;
    static cpmath::MathTables mt;
    for (int i = 0; i < 64; ++i) mt.exp2[i] = cpmath::exp2_table[i];
    for (int i = 0; i < 128; ++i) mt.logc[i] = cpmath::log_table[i];
    for (long long i = 0; i < n; ++i) {
        const double v = x[i];
        double r;
        switch (kind) {
            case 0: r = cpmath::exp_mid(v); break;
            case 1: r = cpmath::exp_tab(v, &mt); break;
            case 2: r = cpmath::log_pos(v); break;
            case 3: r = cpmath::log_tab_any(v, &mt); break;
            case 4: r = cpmath::exp10_mid(v); break;
            case 5: r = cpmath::exp10_tab(v, mt.exp2); break;
            case 6: r = cpmath::sin_bounded(v); break;
            case 7: r = cpmath::recip(v); break;
            default: r = cpmath::rsqrt_pos(v); break;
        }
        y[i] = r;
    }
    return 0;
}

extern "C" const double* emu_math_exp2_table() { return cpmath::exp2_table; }
extern "C" const double* emu_math_log_table() { return cpmath::log_table; }
