// Host access to csrc/cp_uniform_recursions.h for the CPU tests (TEST HARNESS ONLY): `recursions` and `add_carries` run for the 64 lanes of a wave, the
// harness doing what a kernel does by one shift each way -- lane l receives the total of lane l -+ 1, the two end lanes zero.
// tests/test_uniform_recursions_host.py checks the result against the same truncated sums in longdouble.
#include "../../cosmoprimo_amd/csrc/cp_uniform_recursions.h"

namespace {

template <int S, int NF>
void wave(const double* r, double* out, bool swapped) {
    double g[64][S], gin[64], fin[64];
    cpur::Totals totals[64];
    for (int l = 0; l < 64; ++l) {
        for (int t = 0; t < S; ++t) g[l][t] = r[S * l + t];
        totals[l] = cpur::recursions<S>(g[l]);
    }
    for (int l = 0; l < 64; ++l) {
        gin[l] = l < 63 ? totals[l + 1].g_first : 0.;
        fin[l] = l > 0 ? totals[l - 1].f_last : 0.;
    }
    for (int l = 0; l < 64; ++l) {
        if (swapped) cpur::add_carries<S, NF>(g[l], fin[l], gin[l]);      // (a mistake the test must see; never made in the library)
        else cpur::add_carries<S, NF>(g[l], gin[l], fin[l]);
        for (int t = 0; t < S; ++t) out[S * l + t] = g[l][t];
    }
}

}  // namespace

// r, out: (64 S).  S = 32, 33 or 57; NF = S or, for 33 and 57, 36.  Returns 0, or 1 for sizes that are not built.
extern "C" int emu_uniform_recursions(int S, int NF, const double* r, double* out, int swapped) {
    if (S == 32 && NF == 32) wave<32, 32>(r, out, swapped != 0);
    else if (S == 33 && NF == 33) wave<33, 33>(r, out, swapped != 0);
    else if (S == 57 && NF == 57) wave<57, 57>(r, out, swapped != 0);
    else if (S == 57 && NF == 36) wave<57, 36>(r, out, swapped != 0);
    else return 1;
    return 0;
}

extern "C" double emu_uniform_recursions_p() { return cpur::P; }
