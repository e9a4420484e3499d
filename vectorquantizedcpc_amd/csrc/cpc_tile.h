// The forward of one CPC tile -- 16 anchors of one utterance at one prediction step -- shared by cpc.hip (scoring) and
// cpc_grad.hip (the same forward followed by the gradients): steps 1-3 of cpc_score_kernel as device functions, the finish
// kernel, and the handle.  Both files run THESE statements, so the loss, step losses and accuracies of vqcpc_cpc_grad have the
// bits of vqcpc_cpc_score.  What the gradient needs on top (the row a pair scored, the maximum and the sum of a position) leaves
// through optional LDS outputs; a null pointer (scoring) drops the store and nothing else.
#pragma once
#include "cpc_protocol.h"
#include "ar_shared.h"

namespace {

constexpr int CPC_TT = 16;           // anchors per workgroup
constexpr int CPC_D = 64;            // z_dim
constexpr int CPC_WCS = CPC_D + 4;   // LDS row stride of Wc: 16-byte reads of 16 different t fall on 16 different bank quads
constexpr int CPC_MAXJ = 65;         // 1 + Neg

struct CpcArgs {
    const float *z, *c, *W, *bias;             // W (n_steps, 64, C), bias (n_steps, 64): the handle's copies, or the caller's (grad)
    const int64_t *utt_index, *seq_index;      // both null: protocol mode
    float *scores;                             // (n_steps, N, 1 + Neg, L) or null
    uint8_t *correct;                          // (n_steps, N, L) or null
    double *part_loss;                         // (n_steps, N, tiles)
    int *part_correct;
    int T, L, C, Spk, Utt, Neg, tiles;
    unsigned stream_id, key0, key1;
};

// ---- 1. Wc tile: A = W_k rows (feature 16 wave + lane & 15), B = c rows (anchor lane & 15); component q of the fragment at
// column 16 s + 4 (lane >> 4) is the k-slot lane >> 4 of MFMA (s, q).  Anchors past L read row L - 1 and are masked below.
__device__ __forceinline__ void cpc_wc_tile(const CpcArgs &a, float (*wc)[CPC_WCS], int lane, int wave, int n, int k, int t0) {
    const int L = a.L, C = a.C;
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

// ---- 2. scores: pair p = (j = p >> 4, t = p & 15).  rows (LDS, [J][16]) takes the row of z each pair scored, u_out
// (n_steps, Utt, Neg) and s_out (n_steps, N, Neg, L) the negatives' two indices as int32; each may be null.
__device__ __forceinline__ void cpc_score_pairs(const CpcArgs &a, const float (*wc)[CPC_WCS], float (*sc)[CPC_TT], int tid, int tile, int n,
                                                int k, int (*rows)[CPC_TT], int *u_out, int *s_out) {
    const int t0 = tile * CPC_TT, N = a.Spk * a.Utt;
    const int spk = n / a.Utt, utt = n - spk * a.Utt;
    const int L = a.L;
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
            if (u_out && spk == 0 && tile == 0 && tl == 0) u_out[(size_t)(k - 1) * a.Utt * a.Neg + iu] = u;
            if (s_out && t0 + tl < L) s_out[(size_t)(k - 1) * N * a.Neg * L + is] = s;
        }
        if (rows) rows[j][tl] = (int)row;
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
}

// ---- 3. cross entropy against label 0 and first-maximum argmax, one thread per position (tid < 16); pos_m / pos_e (LDS, or
// null) take the maximum and the sum of exponentials of the position.
__device__ __forceinline__ void cpc_position(const CpcArgs &a, const float (*sc)[CPC_TT], float *pos_loss, int *pos_correct, int tid, int t0,
                                             int n, int k, float *pos_m, float *pos_e) {
    const int J = 1 + a.Neg, N = a.Spk * a.Utt, L = a.L;
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
    if (pos_m) { pos_m[tid] = m; pos_e[tid] = e; }
    if (a.correct && t0 + tid < L) a.correct[((size_t)(k - 1) * N + n) * L + t0 + tid] = (uint8_t)ok;
}

// the 16 positions of a tile, added in t order in double: one partial per workgroup (thread 0)
__device__ __forceinline__ void cpc_tile_partial(const CpcArgs &a, const float *pos_loss, const int *pos_correct, int tile, int n, int k) {
    const int t0 = tile * CPC_TT, N = a.Spk * a.Utt;
    double sum = 0.0;
    int cnt = 0;
    const int nv = min(CPC_TT, a.L - t0);
    for (int t = 0; t < nv; ++t) { sum += (double)pos_loss[t]; cnt += pos_correct[t]; }
    const size_t o = ((size_t)(k - 1) * N + n) * a.tiles + tile;
    a.part_loss[o] = sum;
    a.part_correct[o] = cnt;
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
    DevPtr<float> W, bias;           // the handle's copies of the first n_steps predictors, stacked
    DevBuf part_loss, part_correct;
    DevPtr<char> grad_work;          // vqcpc_cpc_grad's work space (cpc_grad.hip)
};

// What vqcpc_cpc_score and vqcpc_cpc_grad (`what`: the entry's name, for the messages) share before their launches: the
// checks of the shape, the draw counter, the index pair and the device, the two partial buffers (P partials per step), and
// the kernel argument -- reading the handle's predictors unless the caller gives W and bias; scores / correct left null.
static int cpc_begin(vqcpc_cpc *cpc, const char *what, const float *z, const float *c, int T, const float *W, const float *bias,
                     const int64_t *utt_index, const int64_t *seq_index, uint64_t seed, uint32_t stream_id, CpcArgs &a, size_t &P) {
    VQ_REQUIRE((utt_index == nullptr) == (seq_index == nullptr), "%s: give utt_index and seq_index together, or neither", what);
    const int K = cpc->n_steps;
    VQ_REQUIRE(T >= K + 2, "%s: T = %d, need at least n_steps + 2 = %d frames (model.py:259 draws from [1, T - n_steps))", what, T, K + 2);
    const int L = T - K, N = cpc->Spk * cpc->Utt;
    VQ_REQUIRE((long long)N * cpc->Neg * L < (1ll << 31), "%s: Spk * Utt * Neg * L = %lld does not fit the draw counter", what,
               (long long)N * cpc->Neg * L);
    TRY(vq_require_device(cpc->device, what));
    const int tiles = (L + CPC_TT - 1) / CPC_TT;
    P = (size_t)N * tiles;
    TRY(cpc->part_loss.reserve(P * K * sizeof(double)));
    TRY(cpc->part_correct.reserve(P * K * sizeof(int)));
    a.z = z; a.c = c; a.W = W ? W : cpc->W.as<float>(); a.bias = W ? bias : cpc->bias.as<float>();
    a.utt_index = utt_index; a.seq_index = seq_index;
    a.scores = nullptr; a.correct = nullptr;
    a.part_loss = cpc->part_loss.as<double>(); a.part_correct = cpc->part_correct.as<int>();
    a.T = T; a.L = L; a.C = cpc->C; a.Spk = cpc->Spk; a.Utt = cpc->Utt; a.Neg = cpc->Neg; a.tiles = tiles;
    a.stream_id = stream_id; a.key0 = (unsigned)(seed & 0xFFFFFFFFu); a.key1 = (unsigned)(seed >> 32);
    return VQCPC_OK;
}
