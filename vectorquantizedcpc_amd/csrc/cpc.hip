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
#include "cpc_protocol.h"
#include "ar_shared.h"

namespace {

constexpr int CPC_TT = 16;           // anchors per workgroup
constexpr int CPC_D = 64;            // z_dim
constexpr int CPC_WCS = CPC_D + 4;   // LDS row stride of Wc: 16-byte reads of 16 different t fall on 16 different bank quads
constexpr int CPC_MAXJ = 65;         // 1 + Neg

struct CpcArgs {
    const float *z, *c, *W, *bias;             // W (n_steps, 64, C), bias (n_steps, 64): the handle's copies
    const int64_t *utt_index, *seq_index;      // both null: protocol mode
    float *scores;                             // (n_steps, N, 1 + Neg, L) or null
    uint8_t *correct;                          // (n_steps, N, L) or null
    double *part_loss;                         // (n_steps, N, tiles)
    int *part_correct;
    int T, L, C, Spk, Utt, Neg, tiles;
    unsigned stream_id, key0, key1;
};

__global__ __launch_bounds__(256) void cpc_score_kernel(CpcArgs a) {
    __shared__ __attribute__((aligned(16))) float wc[CPC_TT][CPC_WCS];
    __shared__ float sc[CPC_MAXJ][CPC_TT];
    __shared__ float pos_loss[CPC_TT];
    __shared__ int pos_correct[CPC_TT];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, n = blockIdx.y, k = blockIdx.z + 1;
    const int t0 = tile * CPC_TT, N = a.Spk * a.Utt;
    const int spk = n / a.Utt, utt = n - spk * a.Utt;
    const int L = a.L, C = a.C;

    // ---- 1. Wc tile: A = W_k rows (feature 16 wave + lane & 15), B = c rows (anchor lane & 15); component q of the fragment at
    // column 16 s + 4 (lane >> 4) is the k-slot lane >> 4 of MFMA (s, q).  Anchors past L read row L - 1 and are masked below.
    {
        const int ta = min(t0 + (lane & 15), L - 1);
        const float4 *wp = (const float4 *)(a.W + ((size_t)(k - 1) * CPC_D + wave * 16 + (lane & 15)) * C) + (lane >> 4);
        const float4 *cp = (const float4 *)(a.c + ((size_t)n * a.T + ta) * C) + (lane >> 4);
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < (C >> 4); ++s) mfma_k4(a0, a1, wp[s * 4], cp[s * 4]);
        const f32x4 acc = a0 + a1;                       // C/D map: column = lane & 15 (anchor), row = 4 (lane >> 4) + r (feature)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = wave * 16 + (lane >> 4) * 4 + r;
            wc[lane & 15][d] = acc[r] + a.bias[(k - 1) * CPC_D + d];
        }
    }
    __syncthreads();

    // ---- 2. scores: pair p = (j = p >> 4, t = p & 15)
    const int J = 1 + a.Neg;
    for (int p = tid; p < J * CPC_TT; p += 256) {
        const int j = p >> 4, tl = p & 15;
        const int t = min(t0 + tl, L - 1);
        size_t row;
        if (j == 0) {
            row = (size_t)n * a.T + t + k;               // positive (model.py:222)
        } else {
            int u, s;
            const unsigned iu = (unsigned)(utt * a.Neg + (j - 1));
            const size_t is = ((size_t)n * a.Neg + (j - 1)) * L + t;
            if (a.utt_index) {                           // clamped: a bad index cannot read out of bounds (the wrapper rejects it)
                const long long uu = a.utt_index[(size_t)(k - 1) * a.Utt * a.Neg + iu];
                const long long ss = a.seq_index[(size_t)(k - 1) * N * a.Neg * L + is];
                u = (int)min(max(uu, 0ll), (long long)(a.Utt - 1));
                s = (int)min(max(ss, 0ll), (long long)(L - 1));
            } else {
                u = cpc_draw_utt(k, iu, a.Utt, a.stream_id, a.key0, a.key1);
                s = cpc_draw_seq(k, (unsigned)is, t, L, a.stream_id, a.key0, a.key1);
            }
            row = ((size_t)spk * a.Utt + u) * a.T + s + k;           // model.py:282 on z_shift = z[:, :, k : L + k]
        }
        const float4 *zp = (const float4 *)(a.z + row * CPC_D);
        const float4 *wp = (const float4 *)&wc[tl][0];
        float4 zv[CPC_D / 4];
#pragma unroll
        for (int q = 0; q < CPC_D / 4; ++q) zv[q] = zp[q];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int q = 0; q < CPC_D / 4; ++q) {
            const float4 w = wp[q];
            s0 = fmaf(zv[q].x, w.x, s0);
            s1 = fmaf(zv[q].y, w.y, s1);
            s2 = fmaf(zv[q].z, w.z, s2);
            s3 = fmaf(zv[q].w, w.w, s3);
        }
        const float f = ((s0 + s1) + (s2 + s3)) * 0.125f;            // / sqrt(64), exact
        sc[j][tl] = f;
        if (a.scores && t0 + tl < L) a.scores[(((size_t)(k - 1) * N + n) * J + j) * L + t0 + tl] = f;
    }
    __syncthreads();

    // ---- 3. cross entropy against label 0 and first-maximum argmax, one thread per position
    if (tid < CPC_TT) {
        const float f0 = sc[0][tid];
        float m = f0;
        int ok = 1;
        for (int j = 1; j < J; ++j) {
            const float f = sc[j][tid];
            ok &= !(f > f0);
            m = fmaxf(m, f);
        }
        float e = 0.f;
        for (int j = 0; j < J; ++j) e += expf(sc[j][tid] - m);
        pos_loss[tid] = (m + logf(e)) - f0;
        pos_correct[tid] = ok;
        if (a.correct && t0 + tid < L) a.correct[((size_t)(k - 1) * N + n) * L + t0 + tid] = (uint8_t)ok;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        int cnt = 0;
        const int nv = min(CPC_TT, L - t0);
        for (int t = 0; t < nv; ++t) { sum += (double)pos_loss[t]; cnt += pos_correct[t]; }
        const size_t o = ((size_t)(k - 1) * N + n) * a.tiles + tile;
        a.part_loss[o] = sum;
        a.part_correct[o] = cnt;
    }
}

// One workgroup; P partials per step; positions = N * L.
__global__ __launch_bounds__(256) void cpc_finish_kernel(const double *part_loss, const int *part_correct, int n_steps, int P,
                                                         int positions, float *loss, float *step_loss, float *accuracy) {
    __shared__ double rs[256];
    __shared__ int rc[256];
    const int tid = threadIdx.x;
    double total = 0.0;                                  // thread 0 only
    for (int k = 0; k < n_steps; ++k) {
        double s = 0.0;
        int c = 0;
        for (int i = tid; i < P; i += 256) { s += part_loss[(size_t)k * P + i]; c += part_correct[(size_t)k * P + i]; }
        rs[tid] = s; rc[tid] = c;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (tid < h) { rs[tid] += rs[tid + h]; rc[tid] += rc[tid + h]; }
            __syncthreads();
        }
        if (tid == 0) {
            const float sl = (float)(rs[0] / (double)positions);         // F.cross_entropy's mean (model.py:305)
            step_loss[k] = sl;
            accuracy[k] = (float)rc[0] / (float)positions;              // model.py:308
            total += (double)sl;
        }
        __syncthreads();
    }
    if (tid == 0) *loss = (float)(total / (double)n_steps);             // model.py:315
}

}  // namespace

struct vqcpc_cpc {
    int device = 0;
    int n_steps = 0, Spk = 0, Utt = 0, Neg = 0, C = 0;
    float *W = nullptr, *bias = nullptr;
    DevBuf part_loss, part_correct;
};

extern "C" void vqcpc_cpc_destroy(vqcpc_cpc *cpc) {
    if (!cpc) return;
    if (cpc->W) (void)hipFree(cpc->W);
    if (cpc->bias) (void)hipFree(cpc->bias);
    cpc->part_loss.release();
    cpc->part_correct.release();
    delete cpc;
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
    h->n_steps = w->n_steps; h->Spk = w->n_speakers; h->Utt = w->n_utterances; h->Neg = w->n_negatives; h->C = w->c_dim;
    (void)hipGetDevice(&h->device);
    const size_t wb = (size_t)CPC_D * h->C * sizeof(float), bb = CPC_D * sizeof(float);
    bool ok = hipMalloc((void **)&h->W, wb * h->n_steps) == hipSuccess && hipMalloc((void **)&h->bias, bb * h->n_steps) == hipSuccess;
    for (int k = 0; ok && k < h->n_steps; ++k)
        ok = hipMemcpy((char *)h->W + wb * k, w->weight[k], wb, hipMemcpyDeviceToDevice) == hipSuccess &&
             hipMemcpy((char *)h->bias + bb * k, w->bias[k], bb, hipMemcpyDeviceToDevice) == hipSuccess;
    if (ok) ok = hipDeviceSynchronize() == hipSuccess;
    if (!ok) {
        vq_set_error("vqcpc_cpc_create: device allocation or copy failed: %s", hipGetErrorString(hipGetLastError()));
        vqcpc_cpc_destroy(h);
        return VQCPC_ERR_ALLOC;
    }
    *out = h;
    return VQCPC_OK;
}

extern "C" int vqcpc_cpc_score(vqcpc_cpc *cpc, const float *z, const float *c, int T, const int64_t *utt_index,
                               const int64_t *seq_index, uint64_t seed, uint32_t stream_id, float *loss, float *step_loss,
                               float *accuracy, uint8_t *correct, float *scores, void *stream) {
    VQ_REQUIRE(cpc && z && c && loss && step_loss && accuracy, "vqcpc_cpc_score: null argument");
    VQ_REQUIRE((utt_index == nullptr) == (seq_index == nullptr), "vqcpc_cpc_score: give utt_index and seq_index together, or neither");
    const int K = cpc->n_steps;
    VQ_REQUIRE(T >= K + 2, "vqcpc_cpc_score: T = %d, need at least n_steps + 2 = %d frames (model.py:259 draws from [1, T - n_steps))", T, K + 2);
    const int L = T - K, N = cpc->Spk * cpc->Utt;
    VQ_REQUIRE((long long)N * cpc->Neg * L < (1ll << 31), "vqcpc_cpc_score: Spk * Utt * Neg * L = %lld does not fit the draw counter",
               (long long)N * cpc->Neg * L);
    int dev = -1;
    HIP_TRY(hipGetDevice(&dev));
    VQ_REQUIRE(dev == cpc->device, "vqcpc_cpc_score: handle belongs to device %d, current device is %d", cpc->device, dev);
    const int tiles = (L + CPC_TT - 1) / CPC_TT;
    const size_t P = (size_t)N * tiles;
    TRY(cpc->part_loss.reserve(P * K * sizeof(double)));
    TRY(cpc->part_correct.reserve(P * K * sizeof(int)));
    CpcArgs a;
    a.z = z; a.c = c; a.W = cpc->W; a.bias = cpc->bias;
    a.utt_index = utt_index; a.seq_index = seq_index;
    a.scores = scores; a.correct = correct;
    a.part_loss = cpc->part_loss.as<double>(); a.part_correct = cpc->part_correct.as<int>();
    a.T = T; a.L = L; a.C = cpc->C; a.Spk = cpc->Spk; a.Utt = cpc->Utt; a.Neg = cpc->Neg; a.tiles = tiles;
    a.stream_id = stream_id; a.key0 = (unsigned)(seed & 0xFFFFFFFFu); a.key1 = (unsigned)(seed >> 32);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cpc_score_kernel, dim3(tiles, N, K), dim3(256), 0, s, a);
    hipLaunchKernelGGL(cpc_finish_kernel, dim3(1), dim3(256), 0, s, a.part_loss, a.part_correct, K, (int)P, N * L, loss, step_loss,
                       accuracy);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
