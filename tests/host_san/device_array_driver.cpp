// device_array_driver.cpp -- cp::DeviceArray and cp::place_status (csrc/cp_device_array.h) under AddressSanitizer + UndefinedBehaviorSanitizer against a
// stub of the runtime: hipMalloc / hipFree / hipMemcpy / hipMemset over malloc, which count the live allocations and fail the k-th call (a malloc
// with hipErrorOutOfMemory, a copy or a memset with hipErrorInvalidValue).  Linked against no HIP runtime; built and run by
// tests/test_host_sanitizers.py.  A struct of five arrays of mixed types is filled in sequence, as a plan constructor fills its plan, for every k
// from 0 (no failure) to the number of calls: the first failure's error is the one that comes back, nothing is allocated behind it, nothing is live
// once the struct is dead, and place_status maps the error as the plans' one rule says.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>

#include "../../cosmoprimo_amd/csrc/cp_device_array.h"

namespace {
std::set<void*> live;
int calls = 0, fail_at = 0;      // fail_at: the 1-based call that fails; 0: none
bool failed_a_malloc = false;

bool fails() { return ++calls == fail_at; }
}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) {
    *ptr = reinterpret_cast<void*>(0x1);      // a failed call leaves garbage behind: the array must not keep it
    if (fails()) {
        failed_a_malloc = true;
        return hipErrorOutOfMemory;
    }
    *ptr = size ? malloc(size) : nullptr;
    if (*ptr) live.insert(*ptr);
    return hipSuccess;
}
hipError_t hipFree(void* ptr) {
    if (!ptr) return hipSuccess;
    if (!live.erase(ptr)) {
        fprintf(stderr, "hipFree of %p, which is not live\n", ptr);
        abort();
    }
    free(ptr);
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t size, hipMemcpyKind kind) {
    if (kind != hipMemcpyHostToDevice) abort();
    if (fails()) return hipErrorInvalidValue;
    if (size) memcpy(dst, src, size);      // (ASan checks both ranges)
    return hipSuccess;
}
hipError_t hipMemset(void* dst, int value, size_t size) {
    if (fails()) return hipErrorInvalidValue;
    if (size) memset(dst, value, size);
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : e == hipErrorInvalidValue ? "invalid argument" : "other"; }
}

namespace {

struct Consts {
    double a[3];
    int n;
};
struct Plan {
    int device = 3;
    cp::DeviceArray<double> d_tab;
    cp::DeviceArray<int> d_index;
    cp::DeviceArray<Consts> d_consts;
    cp::DeviceArray<unsigned> d_ticket;
    cp::DeviceArray<float> d_work;
};

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "line %d (k = %d): %s\n", __LINE__, fail_at, #cond); \
            return 1;                                                            \
        }                                                                        \
    } while (0)

// what a constructor does: uploads in sequence, the first failure through place_status
int fill(Plan* p, hipError_t* error) {
    const double tab[5] = {1., 2., 3., 4., 5.};
    const int index[7] = {0, 1, 2, 3, 4, 5, 6};
    const Consts consts = {{1., 2., 3.}, 4};
    hipError_t e = p->d_tab.upload(tab, 5);
    if (e == hipSuccess) e = p->d_index.upload(index, 7);
    if (e == hipSuccess) e = p->d_consts.upload(&consts, 1);
    if (e == hipSuccess) e = p->d_ticket.zeros(9);
    if (e == hipSuccess) e = p->d_work.alloc(11);
    *error = e;
    return e == hipSuccess ? CP_OK : cp::place_status("cp_some_plan_create", p->device, e);
}

int run() {
    static_assert(sizeof(Plan) == 8 + 5 * sizeof(void*), "a plan of DeviceArrays keeps the layout of a plan of pointers");
    const int ncalls = 9;      // 3 uploads (malloc + copy), zeros (malloc + memset), alloc (malloc)
    for (int k = 0; k <= ncalls + 1; ++k) {
        calls = 0;
        fail_at = k;
        failed_a_malloc = false;
        cp::error_buffer()[0] = 0;
        {
            std::unique_ptr<Plan> p(new Plan());
            hipError_t e;
            const int status = fill(p.get(), &e);
            if (k == 0 || k > ncalls) {
                CHECK(status == CP_OK && e == hipSuccess && calls == ncalls && live.size() == 5);
                CHECK(p->d_tab.get()[4] == 5. && p->d_index[6] == 6 && p->d_consts.get()->n == 4 && p->d_ticket[8] == 0u && p->d_work.get());
                // an array that is filled again frees what it held
                const double again[2] = {7., 8.};
                fail_at = 0;
                CHECK(p->d_tab.upload(again, 2) == hipSuccess && live.size() == 5 && p->d_tab[1] == 8.);
                CHECK(p->d_tab.alloc(0) == hipSuccess && !p->d_tab && live.size() == 4);
            } else {
                CHECK(calls == k);      // nothing is asked of the runtime behind the first failure
                CHECK(e == (failed_a_malloc ? hipErrorOutOfMemory : hipErrorInvalidValue));
                CHECK(status == (failed_a_malloc ? CP_ENOMEM : CP_EDEVICE));
                char expected[256];
                snprintf(expected, sizeof(expected), "cp_some_plan_create: cannot place the tables on device 3: %s", failed_a_malloc ? "out of memory" : "invalid argument");
                CHECK(!strcmp(cp::error_buffer(), expected));
                // the arrays filled before the failure are held, the one that failed and those behind it are empty
                const void* held[5] = {p->d_tab.get(), p->d_index.get(), p->d_consts.get(), p->d_ticket.get(), p->d_work.get()};
                const int filled = k <= 6 ? (k - 1) / 2 : k <= 8 ? 3 : 4;
                for (int i = 0; i < 5; ++i) CHECK((held[i] != nullptr) == (i < filled));
                CHECK((int)live.size() == filled);
            }
        }
        CHECK(live.empty());      // the struct is dead
    }
    // release(): the array is the caller's
    fail_at = 0;
    double* kept;
    {
        cp::DeviceArray<double> a;
        CHECK(a.zeros(3) == hipSuccess);
        kept = a.release();
        CHECK(!a.get());
    }
    CHECK(live.size() == 1 && kept[2] == 0.);
    CHECK(hipFree(kept) == hipSuccess && live.empty());
    return 0;
}

}  // namespace

int main() {
    if (run()) return 1;
    printf("ok\n");
    return 0;
}
