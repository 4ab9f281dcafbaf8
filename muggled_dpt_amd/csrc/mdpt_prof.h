// Optional per-launch HIP-event profiler (off by default; bench.py turns it on for the timed region).
// Events are recorded on the SAME stream the kernel is launched on, so durations are device-side and need no host sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>

int mdpt_prof_begin(const char* name, double flops, hipStream_t stream);  // returns this scope's record handle = (profiling generation, index); -1: profiling off
void mdpt_prof_end(int record, hipStream_t stream);
bool mdpt_prof_on();

// Each scope closes ITS OWN record (nested scopes and launches from several host threads - the two half-batch streams of one forward are
// driven by one thread, but two handles may run on two threads - cannot close each other's); the record table is guarded by a mutex.
struct MdptProfScope {
    hipStream_t s;
    int rec;
    MdptProfScope(const char* name, double flops, hipStream_t stream) : s(stream), rec(mdpt_prof_on() ? mdpt_prof_begin(name, flops, stream) : -1) {}
    ~MdptProfScope() {
        if (rec >= 0) mdpt_prof_end(rec, s);
    }
};

// The launch prologue of a kernel with more than 64 KiB of dynamic LDS: raise the kernel's limit, once per kernel instantiation (a failure
// is returned as the hipError_t and the next call tries again) ...
template <auto Kernel>
inline int mdpt_lds_limit(unsigned bytes) {
    static bool done = false;
    if (done) return 0;
    const hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    done = e == hipSuccess;
    return (int)e;
}
// ... and the instantiation's profiler label, formatted on the first call
template <auto Kernel, typename... Args>
inline const char* mdpt_kernel_label(const char* fmt, Args... args) {
    static char name[112] = "";
    if (!name[0]) snprintf(name, sizeof(name), fmt, args...);
    return name;
}
