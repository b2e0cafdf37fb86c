// gzpx_own.h -- host-side owners of what gzpx_api.cpp takes from the HIP runtime: groups of allocations that live
// and die together, events, streams.  The kernels keep seeing raw pointers in the plain structs of gzpx_device.h;
// who frees them is decided here, once.  Nothing in this header is copyable, and none of it may be a static object:
// a destructor that ran at process exit would call into a HIP runtime that is already gone (process-lifetime state
// is held through a pointer that is never deleted).  The device the handles belong to must be current whenever one
// of these is created, released or destroyed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/gzpx.h"

// (GZPX_TRACE in the environment: the failing runtime call is named on stderr)
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess) {                                                                         \
            if (getenv("GZPX_TRACE")) fprintf(stderr, "gzpx: %s:%d %s -> %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return GZPX_ERR_DEVICE;                                                                     \
        }                                                                                               \
    } while (0)

// the same early return for calls that already speak GZPX_* codes
#define GZPX_TRY(expr)                     \
    do {                                   \
        const int _rc = (expr);            \
        if (_rc != GZPX_OK) return _rc;    \
    } while (0)

namespace gzpx {

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// A group of device / pinned allocations with one lifetime.  It remembers WHERE each pointer it handed out is kept
// (a member of a struct that never moves, declared in front of the group), so release() leaves every one of them
// null and a pointer cannot be freed in one place and forgotten in another.
struct Allocs : NoCopy {
    template <class T>
    int dev(T *&p, size_t bytes) {
        HIP_TRY(hipMalloc((void **)&p, bytes));
        held.push_back({(void **)&p, false});
        return GZPX_OK;
    }
    template <class T>
    int pinned(T *&p, size_t bytes) {
        HIP_TRY(hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
        held.push_back({(void **)&p, true});
        return GZPX_OK;
    }
    void release() {
        for (const Held &h : held) {
            (void)(h.pinned ? hipHostFree(*h.at) : hipFree(*h.at));
            *h.at = nullptr;
        }
        held.clear();
    }
    ~Allocs() { release(); }

private:
    struct Held {
        void **at;
        bool pinned;
    };
    std::vector<Held> held;
};

// The grow-on-demand block: a group whose arrays hold `cap` items is asked for `need`.  Too small: everything is
// released FIRST and `fill(new_cap)` allocates afterwards (old and new arrays never exist side by side: peak HBM).
// When that fails the group is left empty with cap 0, so the next call tries again.
template <class Cap, class Fill>
int grow(Allocs &g, Cap &cap, size_t need, size_t new_cap, Fill &&fill) {
    if (need <= cap) return GZPX_OK;
    g.release();
    cap = 0;
    const int rc = fill(new_cap);
    if (rc != GZPX_OK) {
        g.release();
        return rc;
    }
    cap = (Cap)new_cap;
    return GZPX_OK;
}

// An event, with timing or (the default) with hipEventDisableTiming.  Converts to the raw handle for the runtime
// and the launch wrappers.
struct Event : NoCopy {
    hipEvent_t h = nullptr;
    int create(bool timing = false) {
        if (h) return GZPX_OK;  // (a lazily created set is entered again when a later member of it failed)
        if (timing) HIP_TRY(hipEventCreate(&h));
        else HIP_TRY(hipEventCreateWithFlags(&h, hipEventDisableTiming));
        return GZPX_OK;
    }
    operator hipEvent_t() const { return h; }
    ~Event() {
        if (h) (void)hipEventDestroy(h);
    }
};

// A non-blocking stream.  `lowest`: at the lowest priority the device offers -- the workgroups of a side stream are
// only meant to fill what the main stream's kernels leave free.
struct Stream : NoCopy {
    hipStream_t h = nullptr;
    bool made = false;  // (a handle may legitimately read null: the CPU emulator's do)
    int create(bool lowest = false) {
        if (lowest) {
            int least = 0, greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
            HIP_TRY(hipStreamCreateWithPriority(&h, hipStreamNonBlocking, least));
        } else {
            HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
        }
        made = true;
        return GZPX_OK;
    }
    void sync() const {
        if (made) (void)hipStreamSynchronize(h);
    }
    operator hipStream_t() const { return h; }
    ~Stream() {
        if (made) (void)hipStreamDestroy(h);
    }
};

}  // namespace gzpx
