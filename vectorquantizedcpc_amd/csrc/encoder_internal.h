// What the encoder's kernels (encoder.hip), its handle (encoder_host.hip) and the exact-chain GEMM (gemm_chain.hip) share.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------
// im2col of Conv1d(k = 4, stride 2, padding 1) over mel (B, C, T) (model.py:43, :65): GEMM row m = b * To + tt, column kidx.
// mode 1 (VQCPC_CONV_IM2COL): kidx = 4 c + tap, the native layout of conv.weight; mode 2 (VQCPC_CONV_DIRECT): blocks of
// 16 channels, [block][tap][c in block], the k order of the reference's direct back end.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void im2col_ct(int mode, int kidx, int &c, int &tap) {
    if (mode == 1) { c = kidx >> 2; tap = kidx & 3; }
    else { const int rem = kidx & 63; tap = rem >> 4; c = (kidx >> 6) * 16 + (rem & 15); }
}
// Element (m, kidx) of the im2col matrix of N rows: zero in the padding and for rows m >= N.
__device__ __forceinline__ float im2col_at(const float *mel, int C, int T, int To, int N, int m, int kidx, int mode) {
    int c, tap;
    im2col_ct(mode, kidx, c, tap);
    const int b = m / To, tt = m - b * To, ti = 2 * tt + tap - 1;
    return (m < N && ti >= 0 && ti < T) ? mel[((size_t)b * C + c) * T + ti] : 0.f;
}

// The conv of the layered schedule: Y (M, N) = im2col(mel) (M, 4 C) x W (N, 4 C)^T in the k order `mode` W is arranged in, as an
// exact chain restarted every KC (gemm_chain.hip).
int vq_gemm_chain_im2col(const float *mel, int C, int T, int To, const float *W, float *Y, int M, int N, int KC, int mode, hipStream_t s);

// ------------------------------------------------------------------------------------------
// launches of encoder.hip
// ------------------------------------------------------------------------------------------
struct LnConst { float inv[16]; float sc[8]; };      // 1 / (j + 1); 64 / (64 (q + 1)): the weights of ATen's Welford cascade

// One front-end call of the fused / column-split schedules.  The handle fills the model's half once; a call sets mel, the
// shape, the conv order, the outputs and stage.
struct FusedP {
    const float *mel; int C, T, To, N;
    int conv_mode;                      // 1 im2col order (one chain), 2 direct order (chain restarted every 64 k)
    const float4 *conv_f;               // conv weight fragments in that order: [32 ct][K/16][64]
    const float *ln_g[5], *ln_b[5];
    const float4 *fc_f[4];              // [32 ct][32][64]
    const float4 *out_f; const float *out_b;   // [4 ct][32][64]
    const float4 *Ef; const float *E, *e2; int n_emb;
    float *z_pre; float *z_q; int64_t *idx;
    float *stage_out; int stage;        // stage dump (vqcpc_encoder_stage): -1 = none
    float eps; LnConst lnc;
};

// Y = LayerNorm(512)(X) (+ ReLU), M rows.  stat (M, 2), if given, receives every row's (mean, rstd) as the kernel computed them.
void launch_ln512(const float *X, const float *g, const float *b, float *Y, int M, float eps, int relu, const LnConst &k, hipStream_t s,
                  float *stat = nullptr);
// VQEmbeddingEMA.encode of N rows of 64: Ef codebook fragments (launch_vq_build_frag), e2 = |E|^2 (launch_rowsumsq64).
void launch_vq_encode(const float *X, int N, const float4 *Ef, const float *E, const float *e2, int n_emb, int64_t *idx, float *zq, hipStream_t s);
// The whole front end + VQ in one launch (p.stage < 0), or up to p.stage with that stage's rows in p.stage_out.
void launch_enc_fused(const FusedP &p, hipStream_t s);
// The same (p.stage < 0 only) in six column-split launches; a, b: two work buffers of N x 512 floats.
void launch_enc_split(const FusedP &p, float *a, float *b, hipStream_t s);
// Eval-branch statistics of VQEmbeddingEMA.forward; hist [n_emb] zeroed by the caller, part [nparts].
void launch_vq_stats(const float *x, const float *q, const int64_t *idx, int n_rows, float *zst, double *part, int nparts, unsigned *hist,
                     int n_emb, float *loss, float *ppl, hipStream_t s);
// Weight arrangement at create (default stream).
void launch_conv_weight_permute(const float *w, float *w1, float *w2, int O, int C, hipStream_t s = 0);   // conv.weight (O, C, 4) -> (O, 4 C) in the k order of mode 1, 2; also per call for a caller's weights, on its stream
void launch_rowsumsq64(const float *X, float *out, int n, hipStream_t s = 0);          // also after a codebook update, on its stream
void launch_vq_build_frag(const float *E, float4 *Ef, int n_emb, hipStream_t s = 0);
void launch_frag16_build(const float *W, int N, int K, float4 *Wf);                     // N % 16 == 0, K % 64 == 0: (N / 16) (K / 16) 64 float4

// ------------------------------------------------------------------------------------------
// launches of codebook.hip: the EMA update of VQEmbeddingEMA.forward in training mode (model.py:136-145)
// ------------------------------------------------------------------------------------------
// idx16 [n_rows] = idx narrowed; cnt [n_emb] = decay * ema_count + omd * hist (hist: what launch_vq_stats counted).
void launch_ema_prep(const int64_t *idx, int n_rows, const unsigned *hist, const float *ema_count, int n_emb, float decay, float omd,
                     uint16_t *idx16, float *cnt, hipStream_t s);
struct EmaP {
    const float *x; const uint16_t *idx16; int n_rows;        // rows (n_rows, 64) and their codes
    const float *cnt; int n_emb;                              // launch_ema_prep's counts
    float decay, omd, eps, meps;                              // (float)decay, (float)(1.0 - decay), (float)epsilon, (float)(n_emb * epsilon)
    float *ema_count, *ema_weight, *embedding;                // the module's buffers, updated in place
    float *codebook;                                          // the handle's copy of embedding
};
void launch_ema_update(const EmaP &p, hipStream_t s);

// ------------------------------------------------------------------------------------------
// front_grad.hip: the front end of a training step and its backward (include/vqcpc.h)
// ------------------------------------------------------------------------------------------
// The front end's weights as the kernels read them: the handle's copies (built once at create), or a caller's tensors.
struct FrontW {
    vqcpc_encoder_front_weights t;      // the seventeen tensors in the reference's layouts (t.conv_weight: also the layout of its gradient)
    const float *conv_w1, *conv_w2;     // conv.weight as a GEMM operand in the k order of conv mode 1, 2; null = build per call from t
};
using FrontG = vqcpc_encoder_front_grads;              // gradients wanted (null = not)
// The seventeen slots of either struct as one array in member order: conv, 5 LayerNorm weights, 5 LayerNorm biases, 4 fc, out
// weight, out bias -- the one way to walk them all.
constexpr int FRONT_SLOTS = 17;
static_assert(sizeof(vqcpc_encoder_front_weights) == FRONT_SLOTS * sizeof(void *) && sizeof(FrontG) == FRONT_SLOTS * sizeof(void *),
              "the front-end structs are seventeen pointers and nothing else");
inline const float *const (&front_slots(const vqcpc_encoder_front_weights &w))[FRONT_SLOTS] {
    return reinterpret_cast<const float *const (&)[FRONT_SLOTS]>(w);
}
inline float *const (&front_slots(const FrontG &g))[FRONT_SLOTS] { return reinterpret_cast<float *const (&)[FRONT_SLOTS]>(g); }

// Where a call of the layered schedule leaves its rows, per layer l = 0 .. 4: x[l] (N, 512) the rows entering LayerNorm l (the conv's
// or an FC's output), a[l] (N, 512) the rows leaving its ReLU, stat[l] (N, 2) that LayerNorm's (mean, rstd) or null = not kept;
// z_pre (N, 64), needed for stage 10 only.  Layers may share buffers wherever a row is dead before it is overwritten.
struct FrontDst { float *x[5], *a[5], *stat[5], *z_pre; };
// THE layered schedule (encoder_host.hip): conv as an im2col GEMM, then LayerNorm + ReLU and FC in turn, up to `stop_stage`
// (0 conv, 1 + 2l LN_l + ReLU, 2 + 2l FC_l, 10 z_pre), every GEMM an exact chain with fixed K blocks.  C = in_channels, conv_mode
// 1 or 2 (resolved), w.conv_w1 / conv_w2 given.  *stage_out = the buffer of `d` that holds the stop stage's rows.
int vq_front_chain(const FrontW &w, const LnConst &lnc, const float *mel, int B, int C, int T, int conv_mode, int stop_stage,
                   const FrontDst &d, const float **stage_out, hipStream_t s);
// The work space of both calls, grow-only, a member of the encoder handle.
struct FrontGradWork {
    DevBuf convw;                       // forward, caller's weights: conv.weight in the two k orders
    DevBuf wT;                          // backward: one layer's weight, transposed
    DevBuf d0, d1;                      // backward: two (R, 512) gradient buffers
    DevBuf part, colpart;               // backward: slab partials of a weight gradient; tile partials of dgamma, dbeta
    size_t bytes() const { return convw.cap + wT.cap + d0.cap + d1.cap + part.cap + colpart.cap; }
};
size_t vq_front_saved_bytes(int B, int To);
// C = in_channels, conv_mode 1 or 2 (resolved).  z_pre (R, 64) and `saved` as vqcpc.h says.
int vq_front_fwd(FrontGradWork &k, FrontW w, const LnConst &lnc, const float *mel, int B, int C, int T, int conv_mode, float *z_pre,
                 float *saved, hipStream_t s);
int vq_front_bwd(FrontGradWork &k, const FrontW &w, const float *mel, int B, int C, int T, const float *saved, const float *grad_z_pre,
                 const FrontG &g, hipStream_t s);
void launch_vq_bwd(const float *z_pre, const float *z_q, size_t n, float scale, const float *grad_z_st, const float *grad_loss,
                   float *grad_z_pre, hipStream_t s);
