// Host-side helpers shared by the launchers of cmdiad_amd: the launch of a kernel with dynamic LDS, and the readers of the
// library's environment switches (listed in INTEGRATION.md, "Environment switches").
#pragma once
#include <stdlib.h>

#include <atomic>
#include <mutex>

#include "common.h"

// Launch Kernel with lds bytes of dynamic LDS.  A kernel that asks for more than 64 KiB needs
// hipFuncAttributeMaxDynamicSharedMemorySize raised first, and the attribute belongs to the function ON THE CURRENT DEVICE:
// one slot per (kernel instantiation, device) holds the largest size set so far.  A fixed size is set on the kernel's first
// launch on a device, a size that depends on the arguments (scan.hip, post.hip) only when it grows.  The fast path is
// hipGetDevice and one atomic load; the first launches of two host threads meet at the mutex, which also keeps a smaller
// size from being set after a larger one.  Devices past kLaunchDevices are served without a slot (the attribute is set on
// every launch).  who = the entry point, for the error text.  Returns CMDIAD_OK or, with the error text set,
// CMDIAD_ERR_LAUNCH; the launch itself is checked by the caller (CMDIAD_CHECK_LAUNCH).
// Kernels with static LDS only are launched with hipLaunchKernelGGL directly.
constexpr int kLaunchDevices = 32;

template <auto Kernel, class... Args>
int launch_lds(const char* who, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args)
{
    static std::atomic<size_t> set_bytes[kLaunchDevices];   // zero-initialised
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        cmdiad_set_error("%s: hipGetDevice failed", who);
        return CMDIAD_ERR_LAUNCH;
    }
    std::atomic<size_t>* slot = dev >= 0 && dev < kLaunchDevices ? &set_bytes[dev] : nullptr;
    if (!slot || slot->load(std::memory_order_acquire) < lds) {
        std::lock_guard<std::mutex> lock(mu);
        if (!slot || slot->load(std::memory_order_relaxed) < lds) {
            if (hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                cmdiad_set_error("%s: hipFuncSetAttribute(MaxDynamicSharedMemorySize=%zu) failed", who, lds);
                return CMDIAD_ERR_LAUNCH;
            }
            if (slot) slot->store(lds, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, stream, args...);
    return CMDIAD_OK;
}

// Environment switches.  A switch that tests and tools change between calls is read on every call that consults it; one that is
// fixed for the process is written `static const int x = env_int(...)` at its site.  The selection switches of the GEMM family are
// read by gemm_plan.h (plan::switches, where each rule consults them) through env_switches() below.
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
inline bool env_is(const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; }   // set, and starts with c

// The test-only build (make ab) is the one in which CMDIAD_GEMM_WIDE, CMDIAD_PP3_GRID, CMDIAD_L2_TILE=2 and the CMDIAD_STAGE1_*
// switches act.
#ifdef CMDIAD_AB_VARIANTS
constexpr bool kAbBuild = true;
#else
constexpr bool kAbBuild = false;
#endif

inline plan::switches env_switches() { return {[](const char* name) -> const char* { return getenv(name); }}; }

// the distance GEMM's: CMDIAD_L2_SPLITS and CMDIAD_L2_QGROUP are fixed for the process
inline plan::switches l2_switches()
{
    static const int splits = env_int("CMDIAD_L2_SPLITS", 0), qgroup = env_int("CMDIAD_L2_QGROUP", 0);
    return {env_switches().get, splits, qgroup};
}
