// cp_device_array.h -- the owner of a plan's device tables, and the one answer of a plan constructor that cannot place them.  Host code only (the
// runtime's API header, nothing device-side): tests/host_san/device_array_driver.cpp compiles it with g++ against a stub runtime that fails on request.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <type_traits>

#include "../../include/cosmoprimo_amd.h"
#include "cp_error.h"

namespace cp {

// One hipMalloc'd array of T, freed when its owner dies -- on the device that is current then: a plan is deleted under a DeviceScope of its device
// (cp_internal.h: destroy_plan).  upload / alloc / zeros replace what the array held; on failure they return the runtime's error and leave it empty.
// Reads as the pointer it holds, so kernel arguments and views are filled from it as from the raw pointer it replaces.
template <typename T>
class DeviceArray {
    T* p_ = nullptr;

    hipError_t emptied(hipError_t e) {
        if (e != hipSuccess) reset();
        return e;
    }

public:
    DeviceArray() = default;
    ~DeviceArray() { reset(); }
    DeviceArray(const DeviceArray&) = delete;
    DeviceArray& operator=(const DeviceArray&) = delete;

    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    hipError_t alloc(size_t count) {      // scratch: contents undefined
        reset();
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, count * sizeof(T));
        if (e == hipSuccess) p_ = static_cast<T*>(p);
        return e;
    }
    hipError_t upload(const T* host, size_t count) {      // synchronous: the host array may die behind the call
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : emptied(hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice));
    }
    hipError_t zeros(size_t count) {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : emptied(hipMemset(p_, 0, count * sizeof(T)));
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    // for tables that live as long as the process (cp_background.hip): the array is the caller's from here on
    T* release() {
        T* p = p_;
        p_ = nullptr;
        return p;
    }
};
// plans keep the layout they had with raw pointers (tests fabricate the head of a cp_dst_plan from ctypes)
static_assert(sizeof(DeviceArray<double>) == sizeof(double*) && std::is_standard_layout<DeviceArray<double>>::value, "a DeviceArray is one pointer");

// The status of plan constructor `who` when the runtime answered `e` to placing its tables on `device`.  hipErrorOutOfMemory is CP_ENOMEM
// (MemoryError in Python), everything else -- a failed copy, a lost device -- CP_EDEVICE.
inline int place_status(const char* who, int device, hipError_t e) {
    return fail(e == hipErrorOutOfMemory ? CP_ENOMEM : CP_EDEVICE, "%s: cannot place the tables on device %d: %s", who, device, hipGetErrorString(e));
}

}  // namespace cp
