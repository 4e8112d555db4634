// cp_internal.h -- what the translation units of libcosmoprimo_amd.so share with each other besides the public C ABI (not installed, not part
// of the ABI): views of plan internals for kernels that fuse several stages (cp_sigma.hip).
#pragma once
#include <atomic>
#include <hip/hip_runtime.h>
#include <memory>

#include "../../include/cosmoprimo_amd.h"
#include "cp_device_array.h"
#include "cp_error.h"

namespace cpfft {
struct cplx;
}
namespace cp {
class Launches;      // the launches of one entry point (below)
}

// device tables of a fused-kernel FFTLog plan (npad <= 8192); false for plans of the general-size path
struct cp_fftlog_tables_view {
    int n, npad, nker, device, in_left, out_left;
    const double* d_pre;
    const double* d_post;
    const cpfft::cplx* d_u;
    const cpfft::cplx* d_tw;
};
bool cp_fftlog_plan_view(const cp_fftlog_plan* plan, cp_fftlog_tables_view* out);

// band form of a spline / operator plan: wb (bw, nq) band-major weights (padded entries are zero), j0 (nq) first knot of each band, -1 for a
// query outside the knots
struct cp_spline_band_view {
    int n, nq, bw, device;
    const double* d_wb;
    const int* d_j0;
};
bool cp_spline_plan_view(const cp_spline_plan* plan, cp_spline_band_view* out);

// The constants of a batch of cosmologies for the evaluation of engine `engine` (cppower::CosmoConsts: fit coefficients of EH98 / no-wiggle, Gamma of
// BBKS, the primordial constants of pk_params -- NULL: transfer functions only) into d_work (cp_power_workspace_bytes(ncosmo) bytes): the first of
// the two kernels cp_power_eval launches.  A launch among its caller's (`on`) and nothing else: the caller (a public entry point) has validated the arguments
// (nsp from cpcosmo::ncdm_species), holds the cp::DeviceScope, has fetched the knots (cpcosmo::ncdm_knots) and reads the launch status once, behind its own kernel.
// d_k / d_ln_k (n wavenumbers; optional): extra workgroups of the same launch write the (3, n) table log k, k^1.08, k^1.4 of the kernels that evaluate on
// a shared grid (cp_power_eval.h: powers_of_wavenumber) -- a launch of their own for 1024 values was 3 % of the fused sigma(r, z) call
void cp_power_coefficients(int engine, long long ncosmo, const cp_param* bg_params, int second_is_omega_m, const cp_ncdm* ncdm, int nsp, const double* knots,
                           const cp_param* pk_params, void* d_work, cp::Launches& on, const double* d_k = nullptr, double* d_ln_k = nullptr, int n = 0);

// the one-kernel route of cp_sigma_rz_analytic (cp_sigma.hip), called by it with its arguments checked (nsp from cpcosmo::ncdm_species): opens the scope and reads the launch status under its name
int cp_sigma_rz_fused(int engine, long long ncosmo, const cp_param* bg_params, int second_is_omega_m, const cp_ncdm* ncdm, int nsp, const cp_param* pk_params,
                      const double* d_k, const cp_fftlog_plan* fftlog, const cp_spline_plan* spline, const double* d_growth_sq, int nz, double* d_out,
                      double* d_pk_out, void* d_work, int device, void* stream);

// a cp_spline_rows plan seen from cp_spline.hip: its queries as (interval, four weights) per query -- A y_j + B y_{j+1} + wM0 M_j + wM1 M_{j+1}, the
// second derivatives M from cp_spline_rows_second_derivatives -- for the kernel that evaluates the k direction of (z, k) tables itself
struct cp_spline_rows_view {
    int n, nq, first_knot, nknots, device;
    const int* d_qj;        // (nq) interval relative to first_knot, -1: outside the knots
    const double* d_qw;     // (nq, 4)
};
bool cp_spline_rows_plan_view(const cp_spline_rows_plan* plan, cp_spline_rows_view* out);

// the uniform-stretch scheme of a splice plan (cp_splice_uniform_plan.h: its tables with their device pointers) for the kernel that runs the spline step
// of wallish2018 behind the inverse transform (cp_dst.hip: wallish_tail_kernel); false when the plan does not run that scheme
namespace cpsu {
struct Tables;
}
bool cp_splice_plan_uniform_view(const cp_splice_plan* plan, cpsu::Tables* out, int* device);

// What the Gauss-Newton entry points (cp_mlp_gauss_newton.hip, cp_taylor_gauss_newton.hip: entry points only; their kernels are variants of the one
// __global__ template of cp_mlp_tangent.h and of cp_taylor_gemm.h, which is how kernels share source here and still keep their instructions; the row
// transforms share inlined functions that keep them, cp_fft_workgroup.h) take
// from the engines' files: the checks of mlp_front / taylor_front under the caller's name, the network's layout, and the launch of the kernel that
// cp_*_predict_columns launches, among the caller's launches (cp::Launches, below): inside its device scope, under its name, its status the caller's to read.
namespace cp {
// the layout of a network, the one list of its fields (cp_mlp_tangent.h: MlpNet is this and the count of parameters); at most 8 hidden layers
struct MlpLayout {
    int ndim, L, M, nr;      // nr: rows of an LDS buffer (the widest layer rounded up to 8)
    int d[10];               // ndim, the widths, M
    int act[8];
    long long off[9];        // start of layer l in the packed buffer (l = L: the output layer)
};
int mlp_front_layout(const char* who, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M, int yfunction, long long col0,
                     long long ncols, MlpLayout* layout);
int mlp_predict_launch(Launches& on, const double* d_x, long long B, int ndim, int nlayers, const int* widths, const int* activations, int M,
                       const double* d_params, const double* d_xoffset, const double* d_xscale, const double* d_yoffset, const double* d_yscale, int yfunction,
                       long long col0, long long ncols, double* d_out, long long ldo);
int taylor_front_checks(const char* who, long long B, int ndim, int T, int max_power, int M, long long col0, long long ncols, long long ld, const char* what);
int taylor_predict_launch(Launches& on, const double* d_x, long long B, const double* d_center, const int* d_powers, int ndim, int T, const double* d_derivatives,
                          int M, long long col0, long long ncols, double* d_out, long long ldo);

// The calling thread on `device` for the lifetime of the scope, and back on the device it came from on every way out.  A call on the device that
// is already current costs one hipGetDevice and nothing else; ok() is false only when a switch was needed and failed.
class DeviceScope {
    int prev_ = -1;
    bool switched_ = false, ok_ = true;

public:
    explicit DeviceScope(int device) {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        if (prev_ != device) ok_ = switched_ = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() {
        if (switched_ && prev_ >= 0) (void)hipSetDevice(prev_);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
    bool ok() const { return ok_; }
};

// What every cp_*_destroy does: the plan's DeviceArray members (cp_device_array.h) are freed with the plan's device current.
template <class Plan>
int destroy_plan(Plan* p) {
    if (!p) return CP_OK;
    DeviceScope scope(p->device);
    delete p;
    return CP_OK;
}
// a plan under construction: destroyed that way on every way out of its constructor but release()
struct PlanDelete {
    template <class Plan>
    void operator()(Plan* p) const {
        (void)destroy_plan(p);
    }
};
template <class Plan>
using PlanPtr = std::unique_ptr<Plan, PlanDelete>;

// The workspace of the entries that evaluate spectra themselves: the cosmologies' constants, 64-byte aligned, and -- for the kernels that evaluate on a
// shared grid of nk wavenumbers -- the (3, nk) table cp_power_coefficients writes, 64-byte aligned behind them.
inline char* align64(void* p) {
    char* c = static_cast<char*>(p);
    return c + ((64 - (reinterpret_cast<unsigned long long>(c) & 63u)) & 63u);
}
struct CoefWorkspace {
    char* coef;
    double* ln_k;
};
inline CoefWorkspace coef_workspace(void* d_work, long long ncosmo) {
    char* coef = align64(d_work);
    return CoefWorkspace{coef, reinterpret_cast<double*>(coef + ((cp_power_workspace_bytes(ncosmo) + 63) / 64) * 64)};
}
inline long long coef_workspace_bytes(long long ncosmo, long long nk) {      // what coef_workspace() may touch of a workspace that starts anywhere
    return 64 + ((cp_power_workspace_bytes(ncosmo) + 63) / 64) * 64 + 3 * nk * (long long)sizeof(double);
}

// compute units of `device` (256 where the runtime does not say)
inline int cu_count(int device) {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
    return ncu;
}

// The grid of a persistent kernel that takes a pair of rows per iteration, `resident` workgroups fitting on the chip: every workgroup the same number of
// pairs (5000 pairs on 1024 resident workgroups would leave a fifth of the chip idle in the last round).  *rounds: pairs per workgroup.
inline int balanced_grid(long long npairs, long long resident, long long* rounds = nullptr) {
    const long long r = (npairs + resident - 1) / resident;
    if (rounds) *rounds = r;
    return (int)((npairs + r - 1) / r);
}

// the status of entry point `who` whose launches ended with `e`
inline int launch_status(const char* who, hipError_t e) {
    return e == hipSuccess ? CP_OK : fail(CP_EDEVICE, "%s: launch failed: %s", who, hipGetErrorString(e));
}

// Dynamic LDS above 64 KB is an opt-in per kernel AND per device (hipFuncAttributeMaxDynamicSharedMemorySize).  Raises the limit of `kernel` on the
// device that is current to the whole 160 KB of a CU less the kernel's static LDS (the limit covers both: a kernel with __shared__ variables of its
// own gets what they leave).
inline hipError_t allow_full_lds(const void* kernel) {
    hipFuncAttributes attr;
    const hipError_t e = hipFuncGetAttributes(&attr, kernel);
    return e != hipSuccess ? e : hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - (int)attr.sharedSizeBytes);
}
// ... the first time KERNEL is launched on the device that is current (once per (kernel, device): a multi-GPU process configures every device it
// launches on, and a later launch with more LDS than the first finds the limit already at the maximum)
template <auto KERNEL>
inline hipError_t allow_full_lds() {
    static std::atomic<bool> configured[64];      // (zero-initialised; two threads may both set the same attribute to the same value: harmless, and no data race)
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && configured[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = allow_full_lds(reinterpret_cast<const void*>(KERNEL));
    if (e == hipSuccess && dev >= 0 && dev < 64) configured[dev].store(true, std::memory_order_release);
    return e;
}

// The launches of entry point `who` on `stream` (the void* of the ABI), inside its DeviceScope.  run<KERNEL> opts in to the full LDS of the
// instantiation it launches when the launch asks for more than 64 KB, so no site names a kernel twice or reasons about its LDS; at most 64 KB it
// is the launch and nothing else.  A failed opt-in stops the entry point: neither that kernel nor any later one of this object is launched, and
// status() reports it as it does a failed launch, with the opt-in's error.  status() reads (and clears) the runtime's last error: once per entry
// point, behind its last launch.
class Launches {
    const char* who_;
    hipStream_t stream_;
    hipError_t refused_ = hipSuccess;

public:
    Launches(const char* who, void* stream) : who_(who), stream_(static_cast<hipStream_t>(stream)) {}
    Launches(const Launches&) = delete;
    Launches& operator=(const Launches&) = delete;
    const char* who() const { return who_; }
    template <auto KERNEL, class... Args>
    void run(dim3 grid, dim3 block, size_t lds, const Args&... args) {
        if (refused_ != hipSuccess || (lds > 64 * 1024 && (refused_ = allow_full_lds<KERNEL>()) != hipSuccess)) return;
        KERNEL<<<grid, block, lds, stream_>>>(args...);
    }
    int status() {
        const hipError_t last = hipGetLastError();
        return launch_status(who_, refused_ != hipSuccess ? refused_ : last);
    }
};

// Kernels that hand data from lane to lane of ONE wave through LDS without a workgroup barrier (the tridiagonal eliminations of cp_bao.hip and
// cp_spline_rows.hip): the hardware executes a wave's LDS instructions in order; this pins the compiler to the same order between the phases
// (staging, forward sweep, backward sweep, evaluation): no LDS access moves across it.  At wavefront scope neither the fences nor the barrier
// emit an instruction.
// the value lane `src` (the same for the whole wave) holds, in every lane
__device__ __forceinline__ double lane_value(double v, int src) {
    const long long bits = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits >> 32), src);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// a value every lane holds alike, moved to scalar registers (first active lane's)
__device__ __forceinline__ double wave_uniform(double v) {
    const long long bits = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)bits), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(bits >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ void wave_lds_phase() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// where the spline kernels (cp_spline.hip, cp_spline_rows.hip) store the value of (row, query): (nrows, nq) row-major, or -- group > 0 --
// (nrows / group, nq, group): the rows of a group (the redshifts of one table) become the fastest axis, i.e. the (nz, nr) -> (nr, nz) transposition
// of sigma_rz is part of the store
__device__ __forceinline__ long long out_index(long long row, int q, int nq, int group) {
    if (group <= 0) return row * nq + q;
    const long long b = row / group;
    return (b * nq + q) * group + (row - b * group);
}
}  // namespace cp
