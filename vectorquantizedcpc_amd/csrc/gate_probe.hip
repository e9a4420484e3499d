// Probes of device helpers (test surface, not on any decode path).  Element-wise, the gate non-linearities: the hardware gates of
// the sample loop's GRU cell update (gate_sigmoid / gate_tanh, ar_shared.h) and the libm gates of scan.hip's sequence scans
// (sigmoidf_ / tanhf), evaluated exactly as the kernels inline them, so a test can compare them with a float64 reference over every
// fp32 range.
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

// The resident decoders' draw (first_max_8lanes, ar_shared.h): one wave per case, its 8 scores placed where chain_combine leaves them
// -- classes 0..3 in lanes 0..3, 4..7 in lanes 32..35 -- and +inf in every other lane, which must not matter.
__global__ void __launch_bounds__(64) probe_draw_kernel(const float *__restrict__ sc, int n, int *__restrict__ cls, unsigned *__restrict__ bits) {
    const unsigned lane = threadIdx.x;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const bool holds = (lane & 0x1Cu) == 0;
        const float v = holds ? sc[(size_t)i * 8 + ((lane >> 5) << 2) + (lane & 3u)] : __builtin_inff();
        float best;
        int kb;
        first_max_8lanes(v, best, kb);
        if (lane == 0) { cls[i] = kb; bits[i] = __float_as_uint(best); }
    }
}

// sc (n, 8) device floats -> cls (n) int32, bits (n) uint32: the winning class and its score's bits; enqueued on `stream`.
extern "C" int vqcpc_probe_draw(const float *sc, int n, int *cls, unsigned *bits, void *stream) {
    VQ_REQUIRE(sc && cls && bits && n > 0, "vqcpc_probe_draw: bad argument");
    hipLaunchKernelGGL(probe_draw_kernel, dim3(n < 4096 ? n : 4096), dim3(64), 0, (hipStream_t)stream, sc, n, cls, bits);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

// The resident decoders' 4-byte exchange words (xd_word_h / xd_word_a and their readers, ar_shared.h), element-wise over fp32 bit
// patterns: for each pattern and each parity the word, whether the value fits, the parity bit as the reader sees it, and the value the
// reader takes out.
__global__ void __launch_bounds__(256) probe_words_kernel(const unsigned *__restrict__ bits, int n, int is_a, unsigned *__restrict__ out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float v = __uint_as_float(bits[i]);
        for (unsigned par = 0; par < 2; ++par) {
            const unsigned w = is_a ? xd_word_a(v, par) : xd_word_h(v, par);
            unsigned *o = out + ((size_t)par * 4) * n + i;
            o[0] = w;
            o[(size_t)n] = (is_a ? xd_word_a_fits(v) : xd_word_h_fits(v)) ? 1u : 0u;
            // which parity the reader accepts: 0, 1, or 2 if it accepts both or none
            const bool k0 = is_a ? xd_word_a_ok(w, 0u) : xd_word_h_ok(w, 0u), k1 = is_a ? xd_word_a_ok(w, 1u) : xd_word_h_ok(w, 1u);
            o[2 * (size_t)n] = k0 == k1 ? 2u : (k1 ? 1u : 0u);
            o[3 * (size_t)n] = __float_as_uint(is_a ? xd_word_a_value(w) : xd_word_h_value(w));
        }
    }
}

// bits (n) device uint32 -> out (2 parities, 4, n) uint32: rows word, fits, parity read back, value bits; enqueued on `stream`.
extern "C" int vqcpc_probe_words(const unsigned *bits, int n, int is_a, unsigned *out, void *stream) {
    VQ_REQUIRE(bits && out && n > 0, "vqcpc_probe_words: bad argument");
    const int blocks = n / 256 + 1 < 4096 ? n / 256 + 1 : 4096;
    hipLaunchKernelGGL(probe_words_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, bits, n, is_a, out);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
