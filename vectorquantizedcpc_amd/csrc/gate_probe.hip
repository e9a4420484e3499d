// Element-wise probe of the gate non-linearities (test surface, not on any decode path): the hardware gates of the sample loop's
// GRU cell update (gate_sigmoid / gate_tanh, ar_shared.h) and the libm gates of scan.hip's sequence scans (sigmoidf_ / tanhf),
// evaluated exactly as the kernels inline them, so a test can compare them with a float64 reference over every fp32 range.
#include "ar_shared.h"

__global__ void __launch_bounds__(256) probe_gates_kernel(const float *__restrict__ v, int n, float *__restrict__ out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float x = v[i];
        out[i] = gate_sigmoid(x);
        out[(size_t)n + i] = gate_tanh(x);
        out[2 * (size_t)n + i] = sigmoidf_(x);
        out[3 * (size_t)n + i] = tanhf(x);
    }
}

// out (4, n): rows gate_sigmoid, gate_tanh, sigmoidf_, tanhf of v (n device floats); enqueued on `stream`, no synchronisation.
extern "C" int vqcpc_probe_gates(const float *v, int n, float *out, void *stream) {
    VQ_REQUIRE(v && out && n > 0, "vqcpc_probe_gates: bad argument");
    const int blocks = n / 256 + 1 < 4096 ? n / 256 + 1 : 4096;
    hipLaunchKernelGGL(probe_gates_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, v, n, out);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
