// optim.hip -- vqcpc_adam_step (include/vqcpc.h): one Adam update of a list of tensors in one launch per
// VQCPC_ADAM_TABLE tensors.  The table of a launch -- four pointers, numel and a chunk prefix per tensor -- is a kernel argument
// passed by value: nothing is allocated and nothing is copied to the device.  The host arithmetic is optim_plan.hip's.
//
// The statement order, per element (every operation one fp32 operation, rounded once; the file is compiled with
// -ffp-contract=off and says so again below, so no two of them become a fused multiply-add; square root and division are the
// correctly rounded ones):
//     m' = m + (g - m) * w1
//     v' = v * c2 + (g * g) * w2
//     d  = sqrt(v') / rb + e
//     p' = p - ss * (m' / d)
// Memory bound: 16 bytes read and 12 written per element.  A workgroup of 256 threads covers VQCPC_ADAM_CHUNK = 4096 elements of
// one tensor: four 16-byte vectors per thread and array, each wave-instruction 1 KiB contiguous; a whole chunk issues its sixteen
// loads before the first result is needed.  The last chunk of a tensor runs the vectors that are left and then a scalar tail of
// numel % 4 elements.
#include "optim.h"

#pragma clang fp contract(off)

constexpr int AT = 256;                                  // threads of a workgroup
constexpr int AV = VQCPC_ADAM_CHUNK / 4 / AT;            // 16-byte vectors per thread and array
static_assert(AV * 4 * AT == VQCPC_ADAM_CHUNK, "a chunk is a whole number of vectors per thread");

__device__ __forceinline__ void adam_update(float &p, const float g, float &m, float &v, const AdamScalars &k) {
    m = m + (g - m) * k.w1;
    v = v * k.c2 + (g * g) * k.w2;
    // sqrtf and / are the correctly rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt: v_sqrt_f32 with its two
    // fma corrections, v_div_scale / v_div_fmas / v_div_fixup).  NOT __fsqrt_rn: that compiles to the bare 1-ulp v_sqrt_f32 here,
    // which tests/test_gpu_adam.py caught on 2 of 4095 elements.
    const float d = sqrtf(v) / k.rb + k.e;
    p = p - k.ss * (m / d);
}

__device__ __forceinline__ void adam_update4(f32x4 &p, const f32x4 g, f32x4 &m, f32x4 &v, const AdamScalars &k) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float pc = p[c], mc = m[c], vc = v[c];
        adam_update(pc, g[c], mc, vc, k);
        p[c] = pc; m[c] = mc; v[c] = vc;
    }
}

__global__ __launch_bounds__(AT) void adam_kernel(const AdamTable tab, const AdamScalars k) {
    const unsigned blk = blockIdx.x;
    int lo = 0, hi = tab.n;                              // the tensor of this workgroup: the last i with first[i] <= blk
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first[mid] <= blk) lo = mid; else hi = mid;
    }
    const uint64_t base = (uint64_t)(blk - tab.first[lo]) * VQCPC_ADAM_CHUNK;
    const uint64_t left = tab.numel[lo] - base;          // >= 1: the prefix gives a tensor ceil(numel / CHUNK) workgroups
    float *__restrict__ p = tab.p[lo] + base;
    const float *__restrict__ g = tab.g[lo] + base;
    float *__restrict__ m = tab.m[lo] + base;
    float *__restrict__ v = tab.v[lo] + base;
    const unsigned tid = threadIdx.x;
    if (left >= VQCPC_ADAM_CHUNK) {                      // a whole chunk: all loads first
        f32x4 P[AV], G[AV], M[AV], V[AV];
#pragma unroll
        for (int j = 0; j < AV; ++j) {
            const unsigned i = tid + j * AT;
            P[j] = ((const f32x4 *)p)[i]; G[j] = ((const f32x4 *)g)[i]; M[j] = ((const f32x4 *)m)[i]; V[j] = ((const f32x4 *)v)[i];
        }
#pragma unroll
        for (int j = 0; j < AV; ++j) {
            const unsigned i = tid + j * AT;
            adam_update4(P[j], G[j], M[j], V[j], k);
            ((f32x4 *)p)[i] = P[j]; ((f32x4 *)m)[i] = M[j]; ((f32x4 *)v)[i] = V[j];
        }
        return;
    }
    const unsigned cnt = (unsigned)left, nvec = cnt >> 2; // the last chunk of the tensor: cnt < CHUNK elements
    for (unsigned i = tid; i < nvec; i += AT) {
        f32x4 P = ((const f32x4 *)p)[i], M = ((const f32x4 *)m)[i], V = ((const f32x4 *)v)[i];
        adam_update4(P, ((const f32x4 *)g)[i], M, V, k);
        ((f32x4 *)p)[i] = P; ((f32x4 *)m)[i] = M; ((f32x4 *)v)[i] = V;
    }
    const unsigned i = (nvec << 2) + tid;                // the scalar tail: cnt % 4 elements
    if (i < cnt) {
        float P = p[i], M = m[i], V = v[i];
        adam_update(P, g[i], M, V, k);
        p[i] = P; m[i] = M; v[i] = V;
    }
}

extern "C" int vqcpc_adam_step(const vqcpc_adam_tensor *tensors, int n_tensors, const vqcpc_adam_hyper *h, void *stream) {
    TRY(adam_validate(tensors, n_tensors, h));
    TRY(vq_require_gfx950());
    for (int i = 0; i < n_tensors; ++i) {                // the memory of the first tensor belongs to the current device
        if (tensors[i].numel == 0) continue;
        int dev = 0;
        hipPointerAttribute_t at;
        HIP_TRY(hipGetDevice(&dev));
        const hipError_t e = hipPointerGetAttributes(&at, tensors[i].param);
        if (e != hipSuccess) (void)hipGetLastError();
        VQ_REQUIRE(e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == dev,
                   "vqcpc_adam_step: tensor %d is not memory of the current device (%d)", i, dev);
        break;
    }
    const AdamScalars k = adam_scalars(*h);
    int next = 0;
    while (next < n_tensors) {
        AdamTable tab{};
        const uint32_t groups = adam_fill(tensors, n_tensors, &next, tab);
        if (groups == 0) break;
        hipLaunchKernelGGL(adam_kernel, dim3(groups), dim3(AT), 0, (hipStream_t)stream, tab, k);
        HIP_TRY(hipGetLastError());                      // a launch that failed is reported before the next one is enqueued
    }
    return VQCPC_OK;
}
