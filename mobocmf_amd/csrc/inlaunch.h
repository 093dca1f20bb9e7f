// Waits between the workgroups of ONE ordinary launch (internal): the one-launch Cholesky (chol.hip potrf_coop_kernel), the
// cooperative step (coop_step.hip) and the conditioned iteration of the one-workgroup kernel (tiny_step.hip, MOBOCMF_STEP_COUPLED).
// The contract (include/mobocmf_hip.h, mobocmf_check_info):
//  - the host checks that every workgroup of the launch is resident at once (il_guard); every wait is still bounded, by
//    IL_WAIT_SECONDS of wall clock (the tick count is a kernel argument, il_guard's wait_ticks);
//  - a wait that gives up is reported ONLY by an atomic OR into a status word (il_abandon); nothing else clears it;
//  - a wait releases only while that word is zero: after a give-up every later wait that reads the word fails at its first
//    poll, in this launch and, where the words persist across launches, in every later one until the host clears them.
// Ordering: one lane arrives or polls; __threadfence() before arriving / publishing and after leaving (the workgroups sit on
// different XCDs); the poll is a relaxed agent-scope load of the word and of the status, issued together, and s_sleep(SLEEP).
#pragma once

#include <mutex>
#include <vector>

#include "common.h"

constexpr int IL_WAIT_SECONDS = 1;      // the bound of every in-launch wait

// ---------------------------------------------------------------------------------------------------- device side
__device__ __forceinline__ void il_abandon(unsigned* status, unsigned bit) { atomicOr(status, bit); }

// one poll, no wait (the panel workgroup's look-ahead fetch: it has other work while the word is short)
__device__ __forceinline__ bool il_poll_ge(unsigned long long* w, unsigned long long target) {
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target;
}

// the poll loop, per lane: true once *w >= target; false when the status word is set or `ticks` of wall clock went by
template <int SLEEP>
__device__ __forceinline__ bool il_spin_ge(unsigned long long* w, unsigned long long target, unsigned* status, uint64_t ticks) {
    const uint64_t t0 = wall_clock64();
    for (;;) {
        const unsigned long long v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned st = __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (st) return false;
        if (v >= target) return true;
        if (wall_clock64() - t0 > ticks) return false;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

// the workgroup waits until *w >= target (thread 0 polls); false: abandoned (reported in the status word), leave the kernel
template <int SLEEP>
__device__ __forceinline__ bool il_wait_ge(unsigned long long* w, unsigned long long target, unsigned* status, uint64_t ticks,
                                           int* flag_lds) {
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool ok = il_spin_ge<SLEEP>(w, target, status, ticks);
        if (!ok) il_abandon(status, 1);
        __threadfence();
        *flag_lds = ok;
    }
    __syncthreads();
    return *flag_lds != 0;
}

// barrier of n workgroups on a monotonic arrival counter (a multiple of n between barriers); n <= 1: no-op
template <int SLEEP>
__device__ __forceinline__ bool il_barrier(unsigned long long* cnt, unsigned n, unsigned* status, uint64_t ticks, int* flag_lds) {
    __syncthreads();
    if (n <= 1) return true;
    if (threadIdx.x == 0) {
        __threadfence();
        const unsigned long long old = atomicAdd(cnt, 1ull), target = (old / n + 1ull) * n;
        const bool ok = il_spin_ge<SLEEP>(cnt, target, status, ticks);
        if (!ok) il_abandon(status, 1);
        __threadfence();
        *flag_lds = ok;
    }
    __syncthreads();
    return *flag_lds != 0;
}

// publish what the workgroup wrote so far: all its stores are issued (barrier), then one agent-scope release by thread 0
__device__ __forceinline__ void il_publish_store(unsigned long long* w, unsigned long long v) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        __hip_atomic_store(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------------------------------- host side
struct IlGuard {
    int64_t resident;        // workgroups of this kernel, thread count and LDS size the device holds at once
    uint64_t wait_ticks;     // IL_WAIT_SECONDS in wall_clock64() ticks of the device
};

// The launch guard of a kernel whose workgroups wait for each other: returns the residency and the wait bound, queried once
// per (device, kernel, threads, shm), and sets the dynamic-LDS attribute to `lds_attr` bytes with that first query when `shm`
// exceeds the default 64 KB (the same value for every shape of a kernel: setting it again is idempotent).  Writes no device
// memory (safe while a stream is captured).
inline int il_guard(const void* kfn, int threads, size_t shm, int lds_attr, IlGuard& out) {
    struct Seen { int dev; const void* kfn; int threads; size_t shm; IlGuard g; };
    static std::mutex mu;
    static std::vector<Seen> seen;
    static thread_local Seen last = {-1, nullptr, 0, 0, {0, 0}};      // (a step launches the same shape every time: no lock)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return MOBOCMF_HIP_ERROR;
    if (last.dev == dev && last.kfn == kfn && last.threads == threads && last.shm == shm) {
        out = last.g;
        return MOBOCMF_OK;
    }
    std::lock_guard<std::mutex> lock(mu);
    for (const Seen& s : seen)
        if (s.dev == dev && s.kfn == kfn && s.threads == threads && s.shm == shm) {
            out = (last = s).g;
            return MOBOCMF_OK;
        }
    if (shm > 64 * 1024 && hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr) != hipSuccess)
        return MOBOCMF_HIP_ERROR;
    int per_cu = 0, cus = 0, khz = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, threads, shm) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
        return MOBOCMF_HIP_ERROR;
    const IlGuard g = {(int64_t)per_cu * cus, (uint64_t)khz * 1000u * IL_WAIT_SECONDS};
    seen.push_back({dev, kfn, threads, shm, g});
    last = seen.back();
    out = g;
    return MOBOCMF_OK;
}
