// Run on a handle's device and restore the caller's current device: every entry point that allocates or launches, of the
// planner (plan_host.h), the replay buffer (k_buffer.hip) and the optimiser (k_optim.hip).  A C caller with several GPUs may have
// another one current.
#pragma once
#include <hip/hip_runtime.h>

namespace tdk {

struct DevGuard {
    int prev = -1;
    bool ok = true;
    explicit DevGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) cur = -1;
        if (cur != dev) {
            ok = hipSetDevice(dev) == hipSuccess;
            if (ok) prev = cur;
        }
    }
    ~DevGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DevGuard(const DevGuard &) = delete;
    DevGuard &operator=(const DevGuard &) = delete;
};

}  // namespace tdk
