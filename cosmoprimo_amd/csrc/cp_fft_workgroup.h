// cp_fft_workgroup.h -- the complex FFT of N points by one workgroup of N / P threads, as the paired real-row transforms run it (cp_rfft.hip, cp_dst.hip,
// cp_wallish_tail.h): pass 0 from registers, the remaining DIF passes through LDS, the result left in LDS in digit-reversed order.  The passes are those of
// the FFTLog kernel (cp_fft_core.h: radix-16 butterflies in registers, swizzled LDS exchanges); the twiddles of the passes behind the first are resident in
// LDS behind the data.  Device code (barriers, register constraints): not part of cp_fft_core.h, which the host tests compile.
//
// Every kernel that uses this keeps the instructions it had with its own copy (tools/compare_device_code.py), which decides the form of what is here:
// forward() takes the twiddles by reference, so that a field of the kernel's arguments is read where pass 0 needs it; the copy of the twiddles into LDS
// (`for (i = t; i < TW_SLOTS; i += T) ltw[i] = tw[N + i]`) stays a loop in each kernel, and cp_rfft.hip reads lds[swz(pos_of_freq(k))] without at():
// inlined from here, either moved the kernels' blocks or registers.
#pragma once

#include "cp_fft_core.h"

namespace cpfft {

template <int N, int P>
struct WorkgroupFft {
    using PL = Plan<N, P>;
    static constexpr int T = PL::T;
    // dynamic LDS: the data slots of one transform (padded layout for N = 4096), the twiddles of passes 1 .., then `extra` bytes of the kernel's own
    static constexpr int DATA_SLOTS = lds_data_slots(N, P), TW_SLOTS = PL::TW_TOTAL - N;
    static constexpr int lds_bytes(int extra = 0) { return (DATA_SLOTS + TW_SLOTS) * (int)sizeof(cplx) + extra; }
    static __device__ __forceinline__ cplx* twiddles(cplx* lds) { return lds + DATA_SLOTS; }

    // LDS position of frequency k after the full DIF network (digit reversal of the mixed-radix plan) ...
    static __device__ __forceinline__ int pos_of_freq(int k) {
        int pos = 0;
#pragma unroll
        for (int i = 0; i < PL::NPASS; ++i) {
            const int R = PL::radix(i), M = PL::len(i) / R;
            pos += (k % R) * M;
            k /= R;
        }
        return pos;
    }
    // ... and the read of a position through the swizzle: frequency k is at(lds, pos_of_freq(k))
    static __device__ __forceinline__ cplx at(const cplx* lds, int pos) { return lds[swz<N, P>(pos)]; }

    template <int I>
    static __device__ __forceinline__ void rest(int t, cplx* lds, const cplx* ltw) {
        if constexpr (I < PL::NPASS) {
            cplx x[P];
            __syncthreads();
            asm volatile("" : "+v"(t));  // no address sharing across passes (register pressure, see cp_fftlog_body.h)
            Pass<N, P, I>::load_lds(t, lds, x);
            Pass<N, P, I>::butterflies(x);
            Pass<N, P, I>::twiddle_apply_lds(t, ltw + (PL::tw_offset(I) - N), x);
            Pass<N, P, I>::store_lds(t, lds, x);
            rest<I + 1>(t, lds, ltw);
        }
    }

    // forward transform of the N points held as x[r] = z[t + T r]; tw: the plan's twiddles in memory, ltw: those of passes 1 .. in LDS (twiddles(lds)).
    // Behind the barrier that ends it frequency k is at(lds, pos_of_freq(k)).
    static __device__ __forceinline__ void forward(int t, const cplx* const& tw, cplx* x, cplx* lds, const cplx* ltw) {
        Pass<N, P, 0>::butterflies(x);
        cplx w[P];
        Pass<N, P, 0>::twiddle_load(t, tw + PL::tw_offset(0), w);
        Pass<N, P, 0>::twiddle_apply(w, x);
        Pass<N, P, 0>::store_lds(t, lds, x);
        rest<1>(t, lds, ltw);
        __syncthreads();
    }
};

}  // namespace cpfft
