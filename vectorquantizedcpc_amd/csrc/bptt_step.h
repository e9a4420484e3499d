// One step of back-propagation through time where every step is a launch: the statements shared by ctx_bwd_step_kernel
// (context_grad.hip, LSTM), voc_bwd_step_kernel (vocoder_grad.hip, GRU) and pre_bwd_step_kernel (prenet_grad.hip, bi-GRU), so that
// the three scans sum in ONE order because they run one piece of code.  256 threads; workgroup = 16 hidden units x 16 utterances.
#pragma once
#include "ar_shared.h"

// dh_rec[b, u] = sum_k W_hh[k, u] d[t + 1][b, k] over the K = 64 NS gate rows, on v_mfma_f32_16x16x4_f32.  Wave w takes k in
// [w K / 4, (w + 1) K / 4) in NS super-steps s of 16 k; inside a super-step MFMA c (c = 0 .. 3) takes k = 16 (w NS + s) + 4 q + c,
// q = 0 .. 3 summed in that order inside the instruction; c even goes to accumulator 0, c odd to accumulator 1, s ascending
// (mfma_k4); the wave's sum is a0 + a1, and the four waves are combined ((w0 + w1) + w2) + w3 (sum4).
// w(s), d(s): this lane's float4 of super-step s -- W_hh[16 (w NS + s) + 4 (lane >> 4) + 0 .. 3][unit lane & 15] and
// d[utterance lane & 15][the same four k]; the lanes of a masked utterance return exact zeros and load nothing (an output column
// depends on its own input column only).  Returns the sum of thread (utterance tid >> 4, unit tid & 15).  Every thread of the
// workgroup calls it (one barrier).  UNROLL: the loop's unroll factor, which changes no sum.
template <int NS, int UNROLL, class FW, class FD>
__device__ __forceinline__ float bptt_step_product(FW w, FD d) {
    __shared__ float red[4][16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll UNROLL
    for (int s = 0; s < NS; ++s) {
        const float4 d4 = d(s);
        mfma_k4(a0, a1, w(s), d4);
    }
    const f32x4 acc = a0 + a1;                       // row = unit 4 (lane >> 4) + r, column = utterance lane & 15
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) * 4 + r][lane & 15] = acc[r];
    __syncthreads();
    const int ul = tid & 15, bl = tid >> 4;
    return sum4(red[0][ul][bl], red[1][ul][bl], red[2][ul][bl], red[3][ul][bl]);
}

// Backward of the GRU cell h = n + z (h_prev - n), n = tanh(gi_n + r gh_n), gate order r, z, n, from dh = the whole gradient that
// reaches h: the gradients of the three input pre-activations (gr, gz, gn), of gh_n (gn_r = gn r; gh_r and gh_z receive gr and
// gz) and the part of dh that h_prev receives directly (carry = dh z).  Each operation is one rounded fp32 operation.
struct GruCellGrad { float gr, gz, gn, gn_r, carry; };
__device__ __forceinline__ GruCellGrad gru_cell_bwd(float r, float z, float gh_n, float n, float h_prev, float dh) {
    const float dn = dh * (1.0f - z), dz = dh * (h_prev - n);
    const float gn = dn * (1.0f - n * n), gz = dz * (z * (1.0f - z)), gr = (gn * gh_n) * (r * (1.0f - r));
    return GruCellGrad{gr, gz, gn, gn * r, dh * z};
}
