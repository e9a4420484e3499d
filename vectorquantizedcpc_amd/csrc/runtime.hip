// runtime.hip -- what every part of libvqcpc_hip.so shares at run time: the per-thread error string, the ABI version and
// the device query (the library is built for gfx950 only and has no CPU fallback).
#include "common.h"
#include <atomic>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static thread_local char g_err[512] = "";
void vq_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}
extern "C" const char *vqcpc_last_error(void) { return g_err; }
extern "C" int vqcpc_abi_version(void) { return VQCPC_ABI_VERSION; }
extern "C" int vqcpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

// Device and pinned bytes the library holds: every DevBuf / HostBuf reports what it allocates and frees (one atomic add per
// (re)allocation, nothing on a call that grows no buffer).  Test surface beside vqcpc_probe_gates, not in include/vqcpc.h:
// once every handle made since a reading is destroyed, both counts are back at that reading, exactly.
static std::atomic<long long> g_live_bytes[2];
void vq_count_bytes(bool pinned, long long delta) { g_live_bytes[pinned].fetch_add(delta, std::memory_order_relaxed); }
extern "C" int vqcpc_debug_live_bytes(uint64_t *device, uint64_t *pinned) {
    VQ_REQUIRE(device && pinned, "vqcpc_debug_live_bytes: null argument");
    *device = (uint64_t)g_live_bytes[0].load(std::memory_order_relaxed);
    *pinned = (uint64_t)g_live_bytes[1].load(std::memory_order_relaxed);
    return VQCPC_OK;
}

int vq_require_gfx950() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        vq_set_error("no HIP device: libvqcpc_hip has no CPU fallback");
        return VQCPC_ERR_NO_DEVICE;
    }
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, dev));
    if (strncmp(p.gcnArchName, "gfx950", 6) != 0) {
        vq_set_error("device %d is %s; this library is built for gfx950 (MI355X) only", dev, p.gcnArchName);
        return VQCPC_ERR_NO_DEVICE;
    }
    return VQCPC_OK;
}
