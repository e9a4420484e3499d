// The fixed-order sums over rows that every recurrent backward ends with (context_grad.hip, vocoder_grad.hip, prenet_grad.hip), on
// plain row-major operands: the kernels of grad_slab.h (the orders: there) with every row read as it stands.
#include "grad_slab.h"

namespace {

struct PlainAtb {
    const float *A; int lda;
    const float *Bm; int ldb;
    float *out; int ldo;
    int R;
    __device__ float a(int r, int m) const { return A[(size_t)r * lda + m]; }
    __device__ float b(int r, int c) const { return Bm[(size_t)r * ldb + c]; }
    __device__ void put(int m, int c, float v) const { float *o = out + (size_t)m * ldo + c; *o = *o + v; }
};
struct PlainRows {
    __device__ long long src(int r) const { return r; }
    __device__ float value(int, int, float v) const { return v; }
};

}  // namespace

void vq_grad_atb(const float *A, int lda, const float *Bm, int ldb, float *out, int ldo, int R, int Na, int Nb, hipStream_t s) {
    hipLaunchKernelGGL(grad_atb_kernel<PlainAtb>, dim3(Nb / 16, Na / 64), dim3(256), 0, s, PlainAtb{A, lda, Bm, ldb, out, ldo, R});
}
void vq_grad_colsum(const float *A, int lda, float *out, int R, int Na, hipStream_t s) {
    hipLaunchKernelGGL(grad_colsum_kernel<PlainAtb>, dim3(Na / 64), dim3(256), 0, s, PlainAtb{A, lda, nullptr, 0, out, 0, R});
}
void vq_grad_rows_w(const float *A, const float *W, int ldw, float *out, int R, int K, int N, hipStream_t s) {
    hipLaunchKernelGGL(grad_rows_w_kernel<PlainRows>, dim3((unsigned)((R + 15) / 16), N / 16), dim3(256), 0, s, A, W, ldw, out, R, K, N, PlainRows{});
}
