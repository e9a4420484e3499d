// CPC scoring: the forward value of CPCLoss (model.py:191-316) under no_grad, one fused launch per batch.
//
// cpc_score_kernel, grid (ceil(L / 16), N, n_steps), 256 threads: a workgroup owns 16 anchors (n, t0 .. t0 + 15) of one
// utterance at one prediction step k.
//   1. Wc = predictors[k-1](c[n, t0 .. t0 + 15])  (model.py:229) on the matrix pipe, fp32 in and out:
//      v_mfma_f32_16x16x4_f32, wave w owns output features 16 w .. 16 w + 15, two accumulators that take the even / odd
//      components of each 16-byte fragment and are added once at the end, then + bias.  Wc lives in LDS only.
//   2. scores (model.py:291): thread (j, t) gathers row j of anchor t -- j = 0 the positive z[n, t + k], j >= 1 negative j
//      -- and runs ONE instruction sequence against Wc[t]: four fma chains over d = 0, 1, 2, 3 (mod 4), combined
//      (a0 + a1) + (a2 + a3), times 0.125.  Every row of a position meets the same Wc values in the same order, so
//      bit-equal rows (z is quantised: neighbouring frames share codes) give bit-equal scores, and a negative that ties
//      the positive leaves the position correct as torch's first-maximum argmax does (model.py:307).
//      Negative indices: the caller's arrays, or drawn here from the protocol of cpc_protocol.h (no index tensor exists).
//   3. per position: logsumexp_j f - f[0] with the maximum subtracted (expf / logf of OCML, not the hardware
//      approximations), correct = no negative scored > the positive; the 16 positions are added in t order in double
//      and go to the workspace as one partial per workgroup.
// cpc_finish_kernel, one workgroup: adds the partials of each step in a fixed order (strided per thread, then an LDS
// tree) -- no float atomics anywhere, so equal inputs give equal bits.  Correct counts are integers.
#include "cpc_tile.h"                // steps 1-3 and the finish kernel as shared device code (cpc_grad.hip runs the same statements)

namespace {

__global__ __launch_bounds__(256) void cpc_score_kernel(CpcArgs a) {
    __shared__ __attribute__((aligned(16))) float wc[CPC_TT][CPC_WCS];
    __shared__ float sc[CPC_MAXJ][CPC_TT];
    __shared__ float pos_loss[CPC_TT];
    __shared__ int pos_correct[CPC_TT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, n = blockIdx.y, k = blockIdx.z + 1;
    const int t0 = tile * CPC_TT;

    cpc_wc_tile(a, wc, lane, wave, n, k, t0);
    __syncthreads();
    cpc_score_pairs(a, wc, sc, tid, tile, n, k, nullptr, nullptr, nullptr);
    __syncthreads();
    if (tid < CPC_TT) cpc_position(a, sc, pos_loss, pos_correct, tid, t0, n, k, nullptr, nullptr);
    __syncthreads();
    if (tid == 0) cpc_tile_partial(a, pos_loss, pos_correct, tile, n, k);
}

}  // namespace

extern "C" void vqcpc_cpc_destroy(vqcpc_cpc *cpc) { delete cpc; }

static int cpc_create_impl(const vqcpc_cpc_weights *w, vqcpc_cpc *h) {
    h->n_steps = w->n_steps; h->Spk = w->n_speakers; h->Utt = w->n_utterances; h->Neg = w->n_negatives; h->C = w->c_dim;
    HIP_TRY(hipGetDevice(&h->device));
    const size_t wb = (size_t)CPC_D * h->C * sizeof(float), bb = CPC_D * sizeof(float);
    TRY(h->W.reserve(wb * h->n_steps));
    TRY(h->bias.reserve(bb * h->n_steps));
    for (int k = 0; k < h->n_steps; ++k) {
        HIP_TRY(hipMemcpy((char *)h->W.p + wb * k, w->weight[k], wb, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy((char *)h->bias.p + bb * k, w->bias[k], bb, hipMemcpyDeviceToDevice));
    }
    HIP_TRY(hipDeviceSynchronize());
    return VQCPC_OK;
}

extern "C" int vqcpc_cpc_create(const vqcpc_cpc_weights *w, vqcpc_cpc **out) {
    VQ_REQUIRE(w && out, "vqcpc_cpc_create: null argument");
    *out = nullptr;
    TRY(vq_require_gfx950());
    VQ_REQUIRE(w->z_dim == CPC_D, "vqcpc_cpc_create: z_dim must be 64, got %d", w->z_dim);
    VQ_REQUIRE(w->c_dim == 64 || w->c_dim == 128 || w->c_dim == 256 || w->c_dim == 512,
               "vqcpc_cpc_create: c_dim must be 64, 128, 256 or 512, got %d", w->c_dim);
    VQ_REQUIRE(w->n_steps >= 1 && w->n_steps <= 16, "vqcpc_cpc_create: n_steps (n_prediction_steps / 2) must be 1..16, got %d", w->n_steps);
    VQ_REQUIRE(w->n_negatives >= 1 && w->n_negatives <= CPC_MAXJ - 1, "vqcpc_cpc_create: n_negatives must be 1..64, got %d", w->n_negatives);
    VQ_REQUIRE(w->n_speakers >= 1 && w->n_utterances >= 1 && (long long)w->n_speakers * w->n_utterances <= 65535,
               "vqcpc_cpc_create: n_speakers, n_utterances must be >= 1 and their product <= 65535");
    for (int k = 0; k < w->n_steps; ++k) VQ_REQUIRE(w->weight[k] && w->bias[k], "vqcpc_cpc_create: predictor %d is null", k);
    vqcpc_cpc *h = new vqcpc_cpc();
    int rc = cpc_create_impl(w, h);
    if (rc != VQCPC_OK) { vqcpc_cpc_destroy(h); return rc; }
    *out = h;
    return VQCPC_OK;
}

extern "C" int vqcpc_cpc_score(vqcpc_cpc *cpc, const float *z, const float *c, int T, const int64_t *utt_index,
                               const int64_t *seq_index, uint64_t seed, uint32_t stream_id, float *loss, float *step_loss,
                               float *accuracy, uint8_t *correct, float *scores, void *stream) {
    VQ_REQUIRE(cpc && z && c && loss && step_loss && accuracy, "vqcpc_cpc_score: null argument");
    CpcArgs a;
    size_t P = 0;
    TRY(cpc_begin(cpc, "vqcpc_cpc_score", z, c, T, nullptr, nullptr, utt_index, seq_index, seed, stream_id, a, P));
    a.scores = scores; a.correct = correct;
    const int K = cpc->n_steps, N = a.Spk * a.Utt;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cpc_score_kernel, dim3(a.tiles, N, K), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cpc_finish_kernel, dim3(1), dim3(256), 0, s, a.part_loss, a.part_correct, K, (int)P, N * a.L, loss, step_loss,
                       accuracy);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
