// Gradients of the vocoder objective (vocoder.py:62-63: F.cross_entropy of the teacher-forced energies of audio[:, :-1] against
// audio[:, 1:]) through the sample-rate network rnnms.ar.* -- embedding, GRU, fc1, fc2 -- and with respect to the conditioning
// series: vqcpc_vocoder_ar_fwd / _bwd of include/vqcpc.h, and their *_cond forms, which
// take the conditioning series from the caller instead of running the prenet.  The prenet and the two tables in front of it are frozen
// here; their backward is prenet_grad.hip, fed by grad_cond.
// B utterances, Hr = size_h_rnn, Hf = n_cls = 256, de = size_i_embed_ar, C = dim_voc_latent, up = upsampling_t.  Utterance b scores
// the steps t < slen[b] = max(n_audio[b] - 1, 0): step t is fed x = audio[b, t], reads conditioning frame t / up and is scored against
// audio[b, t + 1].  Gate order r, z, n; h_t = n + z (h_{t-1} - n) (oracle/f64_ref.py:64-69).  loss = sum_b nll_sum[b] / N.
// Every sum has ONE order, fixed by the code and independent of the grid's timing: no floating-point read-modify-write that two
// workgroups share, no wait on another workgroup; launch boundaries order the steps and the passes.  Equal inputs give equal bits.
// Every operation below is one separately rounded fp32 operation (-ffp-contract=off); "chain" = fp32 fmas from 0.
//
// Forward (vqcpc_vocoder_ar_fwd): vq_tf_score of vocoder_host.hip, the function that IS vqcpc_vocoder_nll -- the same launch-per-step
//   scan and the same fused head -- with the caller's weights re-laid into the work space first (vq_vocoder_relayout) and h_t of every
//   scored step copied out of the chunk buffer after each chunk (tf_save_h_kernel): saved = (B, L - 1, Hr).
//
// Backward (vqcpc_vocoder_ar_bwd).  s = grad_loss * fl(1 / N).  The conditioning (frozen) runs again: cond and the frame table
//   Gc = cond W_ih[:, de:]^T + b_ih; Gemb = emb W_ih[:, :de]^T is the class table.  Every wanted output and the two table gradients
//   dGemb (n_cls, 3Hr), dGc (frames, 3Hr) are zero-filled, then the chunks of CH = tf_chunk_replays * steps_per_graph steps run in
//   REVERSE time order, each adding its sums to them: total' = total + (chunk's sum).  Rows of a chunk: r = b CH + (t - t0); a row is
//   live where t < slen[b]; a row that is not live enters every sum as exact zeros and nothing is read for it.
//   Per chunk:
//   1. voc_gather_h_kernel: H = h_t, Hp = h_{t-1} (zero at t = 0) of the chunk's rows from `saved`.
//   2. Gates again: gh = Hp W_hh^T + b_hh (vq_gemm_chain: bias + chain over k ascending); voc_gates_kernel: gi = Gemb[x] + Gc[frame],
//      r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n) (libm expf / tanhf).
//   3. Head: a = relu(H W1^T + b1), e = a W2^T + b2 (vq_gemm_chain); voc_softmax_kernel, one wave per row: m = max e (butterfly over
//      the lanes), q_k = expf(e_k - m), S = sum q (four per lane in k order, then the butterfly xor 32, 16, .., 1),
//      dlogit_k = (q_k / S - [k == target]) * s.  da = (dlogit W2) * [a > 0], dh_head = da W1: grad_rows_w_kernel of grad_slab.h (the
//      order: there), one 16 x 16 tile per workgroup, k over the four waves.
//   4. The serial part, voc_bwd_step_kernel, grid (Hr / 16, ceil(B / 16)), ONE launch per step, t descending.  Workgroup (rg, bt)
//      owns hidden units 16 rg .. + 15 of utterances 16 bt .. + 15:
//        dh_rec[b, u] = sum_k W_hh[k, u] dgh[t + 1][b, k], k < 3Hr: bptt_step_product of bptt_step.h (the order: there), NS = 3Hr / 64,
//          W_hh read in place; +0 without an MFMA at the last step of the call, and a column whose utterance has no step t + 1
//          enters as zeros.
//        dh = (dh_head + dh_rec) + carry        (carry = z_{t+1} dh_{t+1}; 0 at the utterance's last scored step)
//        gru_cell_bwd of bptt_step.h: dn = dh (1 - z)    dz = dh (h_{t-1} - n)
//        dgi_n = dn (1 - n n)    dgi_z = dz (z (1 - z))    dgi_r = (dgi_n gh_n) (r (1 - r))
//        dgh = (dgi_r, dgi_z, dgi_n r)          carry' = dh z
//      dgi (3Hr) and the n third of dgh (Hr) are stored for the chunk, with one more row per utterance that keeps step t0 + CH of
//      the chunk done before.
//   5. Weight sums of the chunk, grad_atb_kernel of grad_slab.h (A^T B over the chunk's rows in slabs of GRAD_SLAB rows, the slabs
//      added in slab order from 0; the order: there), and that sum is added to the total.
//        dW2 += dlogit^T a     dW1 += da^T H     dW_hh += dgh^T Hp     dGemb += onehot(x)^T dgi (the one-hot rows made on the fly)
//      Column sums, grad_colsum_kernel of grad_slab.h, added to the total:  db2 += sum dlogit    db1 += sum da    db_hh += sum dgh.
//      Frame sums, voc_frame_sum_kernel: dGc[frame] += (sum of dgi over the frame's live steps inside the chunk, t ascending from 0).
//   After the last chunk, from the two tables (the same two kernels, rows = classes or frames):
//      dW_ih[:, :de] = dGemb^T emb    dW_ih[:, de:] = dGc^T cond    db_ih = column sums of dGc
//      d emb = dGemb W_ih[:, :de]     grad_cond = dGc W_ih[:, de:]   (grad_rows_w_kernel, K = 3Hr)
//   Classes never fed and frames no scored step reads keep their zero rows: their products are sums of (+-0) from +0, i.e. +0.
//
// Work space (VocGradWork, beside what the forward scan uses), floats, M = B CH:
//   M (11 Hr + 2 Hf + n_cls) + 4 B Hr + B Hr + (n_cls + frames) 3Hr, plus for a caller's weights the scan's layouts of them.
//
// Padding and dirt: the utterance columns b >= B of the last tile are masked (their lanes load nothing and store nothing), rows that
// are not live likewise; the scan reads dgh[t + 1] and the carry only where step t + 1 of the same call wrote them.  Whatever an
// earlier call left in the work space never reaches a result.
#include "vocoder_internal.h"
#include "bptt_step.h"
#include "grad_slab.h"

namespace {

struct VocRows {                         // the chunk in flight
    const int *slen;                     // [B] scored steps
    const int64_t *audio;                // (B, L)
    int B, L, CH, t0, Hr;
};
__device__ __forceinline__ bool row_live(const VocRows &q, int r, int &b, int &t) {
    b = r / q.CH;
    t = q.t0 + r % q.CH;
    return b < q.B && t < q.slen[b];
}
__device__ __forceinline__ int clamp_class(long long x) { return x < 0 ? 0 : (x >= NLL_CLS ? NLL_CLS - 1 : (int)x); }

// grid (ceil(CH Hr / 4 / 256), B); Hp null: only the head's sums are wanted
__global__ void voc_gather_h_kernel(const float4 *__restrict__ saved, float4 *__restrict__ H, float4 *__restrict__ Hp,
                                    const int *__restrict__ slen, int CH, int t0, int H4, int Tsv) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= CH * H4) return;
    const int tt = i / H4, u = i % H4, t = t0 + tt;
    const bool live = t < slen[b];
    const size_t o = ((size_t)b * CH + tt) * H4 + u;
    const float4 *src = saved + ((size_t)b * Tsv + t) * H4 + u;
    float4 h = make_float4(0.f, 0.f, 0.f, 0.f), hp = h;
    if (live) h = src[0];
    if (live && t > 0) hp = src[-H4];
    H[o] = h;
    if (Hp) Hp[o] = hp;
}

// gh (M, 3Hr): in gh_r | gh_z | gh_n, out r | z | gh_n; nn (M, Hr) = n.  grid (ceil(CH Hr / 256), B)
__global__ void voc_gates_kernel(float *__restrict__ gh, float *__restrict__ nn, const float *__restrict__ Gemb, const float *__restrict__ Gc,
                                 const int *__restrict__ gbase, VocRows q, int up) {
    const int Hr = q.Hr, i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= q.CH * Hr) return;
    const int tt = i / Hr, u = i % Hr, t = q.t0 + tt;
    if (t >= q.slen[b]) return;
    const float *e = Gemb + (size_t)clamp_class(q.audio[(size_t)b * q.L + t]) * 3 * Hr + u;
    const float *c = Gc + ((size_t)gbase[b] + t / up) * 3 * Hr + u;
    float *g = gh + ((size_t)b * q.CH + tt) * 3 * Hr + u;
    const float r = sigmoidf_((e[0] + c[0]) + g[0]);
    const float z = sigmoidf_((e[Hr] + c[Hr]) + g[Hr]);
    const float n = tanhf((e[2 * Hr] + c[2 * Hr]) + r * g[2 * Hr]);
    g[0] = r; g[Hr] = z;
    nn[((size_t)b * q.CH + tt) * Hr + u] = n;
}

// e (M, 256) -> dlogit in place; one wave per row, 4 rows per workgroup.  grid (ceil(M / 4))
__global__ __launch_bounds__(256) void voc_softmax_kernel(float *__restrict__ e, VocRows q, const float *__restrict__ grad_loss, float inv_n) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= q.B * q.CH) return;
    int b, t;
    float4 *row = (float4 *)(e + (size_t)r * NLL_CLS) + lane;
    if (!row_live(q, r, b, t)) { *row = make_float4(0.f, 0.f, 0.f, 0.f); return; }
    const float s = grad_loss ? grad_loss[0] * inv_n : inv_n;
    const float4 v = *row;
    float m = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
    float4 p = make_float4(expf(v.x - m), expf(v.y - m), expf(v.z - m), expf(v.w - m));
    float S = ((p.x + p.y) + p.z) + p.w;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) S = S + __shfl_xor(S, d);
    const int k = clamp_class(q.audio[(size_t)b * q.L + t + 1]) - 4 * lane;
    p.x = (p.x / S - (k == 0 ? 1.f : 0.f)) * s;
    p.y = (p.y / S - (k == 1 ? 1.f : 0.f)) * s;
    p.z = (p.z / S - (k == 2 ? 1.f : 0.f)) * s;
    p.w = (p.w / S - (k == 3 ? 1.f : 0.f)) * s;
    *row = p;
}

// The row maps of grad_rows_w_kernel (grad_slab.h) that are not plain.  mask (R, N) or null: out = mask > 0 ? product : 0.  frames /
// gbase or null: out row (b, f) of (B, T2) reads A's row gbase[b] + f where f < frames[b] and is left alone elsewhere (the caller
// zero-filled it).
struct VocRowMap {
    const float *mask; int N;
    const int *frames, *gbase; int T2;
    __device__ long long src(int r) const {
        if (!frames) return r;
        const int b = r / T2, f = r % T2;
        return f < frames[b] ? (long long)gbase[b] + f : -1;
    }
    __device__ float value(int r, int c, float v) const { return mask && !(mask[(size_t)r * N + c] > 0.f) ? 0.f : v; }
};

struct VocStepP {
    const float *w_hh;                   // (3Hr, Hr)
    const float *gh, *nn, *hp, *dhh;     // (M, 3Hr) r | z | gh_n; (M, Hr) n; h_{t-1}; dh_head
    float *dgi, *dghn;                   // (B (CH + 1), 3Hr), (B (CH + 1), Hr)
    float *carry;                        // (B, Hr)
    VocRows q;
    int longest;
};

template <int NS>                        // 3Hr / 64
__global__ __launch_bounds__(256) void voc_bwd_step_kernel(VocStepP p, int t) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = blockIdx.x, bt = blockIdx.y, Hr = p.q.Hr, CH = p.q.CH, tt = t - p.q.t0;
    const int bg = bt * 16 + (tid >> 4), unit = 16 * rg + (tid & 15);
    const bool act = bg < p.q.B && t < p.q.slen[bg];
    const size_t row = (size_t)bg * CH + tt, drow = (size_t)bg * (CH + 1) + tt;
    float r = 0.f, z = 0.f, hn = 0.f, n = 0.f, hp = 0.f, dhh = 0.f, carry = 0.f;
    if (act) {                                       // requested first: they do not depend on the product
        const float *g = p.gh + row * (3 * Hr) + unit;
        r = g[0]; z = g[Hr]; hn = g[2 * Hr];
        n = p.nn[row * Hr + unit];
        hp = p.hp[row * Hr + unit];
        dhh = p.dhh[row * Hr + unit];
        if (t + 1 < p.q.slen[bg]) carry = p.carry[(size_t)bg * Hr + unit];
    }
    float dh_rec = 0.f;
    if (t + 1 < p.longest) {                         // uniform over the grid
        const int bcol = bt * 16 + (lane & 15);
        const bool live = bcol < p.q.B && t + 1 < p.q.slen[bcol];         // a masked column loads nothing
        const size_t nrow = (size_t)(live ? bcol : 0) * (CH + 1) + tt + 1;
        const int kq = lane >> 4;
        const float *wp = p.w_hh + ((size_t)wave * NS * 16 + 4 * kq) * Hr + unit - (tid & 15) + (lane & 15);    // W_hh in place; 16 * rg spelled so: profiles/ab_bptt_shared.txt, section 3
        dh_rec = bptt_step_product<NS, 2>(
            [&](int s) {
                const float *w = wp + (size_t)16 * s * Hr;
                return make_float4(w[0], w[Hr], w[2 * (size_t)Hr], w[3 * (size_t)Hr]);
            },
            [&](int s) {
                const int k = 16 * (wave * NS + s) + 4 * kq;                  // 2Hr is a multiple of 16: four k never straddle the two buffers
                if (!live) return make_float4(0.f, 0.f, 0.f, 0.f);
                return k < 2 * Hr ? *(const float4 *)(p.dgi + nrow * (3 * Hr) + k) : *(const float4 *)(p.dghn + nrow * Hr + (k - 2 * Hr));
            });
    }
    if (act) {
        const GruCellGrad c = gru_cell_bwd(r, z, hn, n, hp, (dhh + dh_rec) + carry);
        float *d = p.dgi + drow * (3 * Hr) + unit;
        d[0] = c.gr; d[Hr] = c.gz; d[2 * Hr] = c.gn;
        p.dghn[drow * Hr + unit] = c.gn_r;
        p.carry[(size_t)bg * Hr + unit] = c.carry;
    }
}

// Row t0 of every utterance -> its extra row CH, for the chunk in front.  grid (ceil(4 Hr / 256), B)
__global__ void voc_keep_first_kernel(float *__restrict__ dgi, float *__restrict__ dghn, int CH, int Hr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= 4 * Hr) return;
    const size_t r0 = (size_t)b * (CH + 1), r1 = r0 + CH;
    if (i < 3 * Hr) dgi[r1 * 3 * Hr + i] = dgi[r0 * 3 * Hr + i];
    else dghn[r1 * Hr + i - 3 * Hr] = dghn[r0 * Hr + i - 3 * Hr];
}

// The operands of the chunk's sums over rows that are not plain (grad_atb_kernel, grad_colsum_kernel of grad_slab.h); a row that is not
// live enters as zeros.  WHH: a = dgh of the chunk's rows (dgi's r and z thirds, dghn), b = Hp.  GEMB: a = onehot(x), b = dgi.
enum { ATB_WHH, ATB_GEMB };
template <int MODE> struct VocAtb {
    const float *dgi, *dghn, *hp;
    VocRows q;
    float *out; int ldo;                 // out[m * ldo + c] += sum
    int R;
    __device__ float a(int r, int m) const {
        int b, t;
        if (!row_live(q, r, b, t)) return 0.f;
        if (MODE == ATB_GEMB) return clamp_class(q.audio[(size_t)b * q.L + t]) == m ? 1.f : 0.f;
        const size_t dr = (size_t)b * (q.CH + 1) + (t - q.t0);
        return m < 2 * q.Hr ? dgi[dr * (3 * q.Hr) + m] : dghn[dr * q.Hr + m - 2 * q.Hr];
    }
    __device__ float b(int r, int c) const {
        if (MODE == ATB_WHH) return hp[(size_t)r * q.Hr + c];
        int b, t;
        if (!row_live(q, r, b, t)) return 0.f;
        return dgi[((size_t)b * (q.CH + 1) + (t - q.t0)) * (3 * q.Hr) + c];
    }
    __device__ void put(int m, int c, float v) const { float *o = out + (size_t)m * ldo + c; *o = *o + v; }
};

// dGc[gbase[b] + f] += sum of dgi over the live steps of frame f inside the chunk.  grid (B T2, ceil(3Hr / 256))
__global__ void voc_frame_sum_kernel(const float *__restrict__ dgi, float *__restrict__ dGc, const int *__restrict__ frames,
                                     const int *__restrict__ gbase, VocRows q, int T2, int up) {
    const int b = blockIdx.x / T2, f = blockIdx.x % T2, col = blockIdx.y * blockDim.x + threadIdx.x;
    if (col >= 3 * q.Hr || f >= frames[b]) return;
    const long long lo64 = (long long)f * up, hi64 = lo64 + up;
    int lo = lo64 < q.t0 ? q.t0 : (int)(lo64 < q.slen[b] ? lo64 : q.slen[b]);
    int hi = (int)(hi64 < q.slen[b] ? hi64 : q.slen[b]);
    hi = hi < q.t0 + q.CH ? hi : q.t0 + q.CH;
    if (lo >= hi) return;
    float sum = 0.f;
    for (int t = lo; t < hi; ++t) sum += dgi[((size_t)b * (q.CH + 1) + (t - q.t0)) * (3 * q.Hr) + col];
    float *o = dGc + ((size_t)gbase[b] + f) * (3 * q.Hr) + col;
    *o = *o + sum;
}

void launch_rows_w(const float *A, const float *W, int ldw, float *out, const VocRowMap &map, long long R, int K, hipStream_t s) {
    hipLaunchKernelGGL(grad_rows_w_kernel<VocRowMap>, dim3((unsigned)((R + 15) / 16), map.N / 16), dim3(256), 0, s, A, W, ldw, out, (int)R, K, map.N, map);
}

const float *const *members(const vqcpc_vocoder_ar_weights *w) { return &w->embedding; }     // nine pointers in a row
float *const *members(const vqcpc_vocoder_ar_grads *g) { return &g->embedding; }

// What both entries check before anything is enqueued.
int check_call(vqcpc_vocoder *v, const char *what, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
               const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const void *saved, std::vector<int> &slen, int *longest) {
    VQ_REQUIRE(v && audio && idx && speaker && saved, "%s: null argument", what);
    TRY(vq_require_device(v->device, what));
    TRY(vq_tf_check(v, B, Tc, L, n_codes, n_audio, slen, longest));
    VQ_REQUIRE((long long)B * (L > 1 ? L - 1 : 1) < (1ll << 31) / 4, "%s: B * (L - 1) = %lld rows do not fit the row index (< 2^29)", what,
               (long long)B * (L - 1));
    VQ_REQUIRE(B <= 65535, "%s: B = %d, at most 65535 utterances per call", what, B);
    VQ_REQUIRE(aligned16(saved), "%s: saved must be 16-byte aligned", what);
    if (w)
        for (int i = 0; i < 9; ++i) {
            VQ_REQUIRE(members(w)[i], "%s: all nine tensors of rnnms.ar are required in *w", what);
            VQ_REQUIRE(aligned16(members(w)[i]), "%s: the tensors of *w must be 16-byte aligned", what);
        }
    return VQCPC_OK;
}

int view_of(vqcpc_vocoder *v, const vqcpc_vocoder_ar_weights *w, bool scan, ArView *view, hipStream_t s) {
    if (!w) { *view = vq_vocoder_view(v); return VQCPC_OK; }
    return vq_vocoder_relayout(v, w->embedding, w->w_ih, w->w_hh, w->b_ih, w->b_hh, w->fc1_weight, w->fc1_bias, w->fc2_weight, w->fc2_bias, scan, view, s);
}

// the forward and the backward behind both forms of their entries; cond_in: the conditioning series given, or null = the prenet runs
int ar_fwd(const char *what, vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
           const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const float *cond_in, double *nll_sum,
           int64_t *n_scored, int64_t *n_correct, float *cond, void *saved, void *stream);
int ar_bwd(const char *what, vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
           const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const float *cond_in, const void *saved,
           const float *grad_loss, const vqcpc_vocoder_ar_grads *grads, float *grad_cond, void *stream);

}  // namespace

extern "C" int vqcpc_vocoder_ar_saved_bytes(vqcpc_vocoder *v, int B, int L, uint64_t *bytes) {
    VQ_REQUIRE(v && bytes, "vqcpc_vocoder_ar_saved_bytes: null argument");
    VQ_REQUIRE(B >= 1 && L >= 1, "vqcpc_vocoder_ar_saved_bytes: need B >= 1 and L >= 1 (got %d, %d)", B, L);
    VQ_REQUIRE(v->d.Hf == NLL_HF && v->d.n_cls == NLL_CLS, "vqcpc_vocoder_ar_saved_bytes: the scoring head is built for size_h_fc %d and %d "
               "classes, this model has %d and %d", NLL_HF, NLL_CLS, v->d.Hf, v->d.n_cls);
    *bytes = up256((uint64_t)B * (L > 1 ? L - 1 : 1) * v->d.Hr * sizeof(float));
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_ar_fwd(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
                                    const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, double *nll_sum,
                                    int64_t *n_scored, int64_t *n_correct, float *cond, void *saved, void *stream) {
    return ar_fwd("vqcpc_vocoder_ar_fwd", v, audio, idx, speaker, B, Tc, L, n_codes, n_audio, w, nullptr, nll_sum, n_scored, n_correct, cond, saved, stream);
}
extern "C" int vqcpc_vocoder_ar_fwd_cond(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
                                         const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const float *cond_in,
                                         double *nll_sum, int64_t *n_scored, int64_t *n_correct, float *cond, void *saved, void *stream) {
    VQ_REQUIRE(cond_in && aligned16(cond_in), "vqcpc_vocoder_ar_fwd_cond: cond_in must be given and 16-byte aligned");
    return ar_fwd("vqcpc_vocoder_ar_fwd_cond", v, audio, idx, speaker, B, Tc, L, n_codes, n_audio, w, cond_in, nll_sum, n_scored, n_correct, cond, saved, stream);
}
extern "C" int vqcpc_vocoder_ar_bwd(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
                                    const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const void *saved,
                                    const float *grad_loss, const vqcpc_vocoder_ar_grads *grads, float *grad_cond, void *stream) {
    return ar_bwd("vqcpc_vocoder_ar_bwd", v, audio, idx, speaker, B, Tc, L, n_codes, n_audio, w, nullptr, saved, grad_loss, grads, grad_cond, stream);
}
extern "C" int vqcpc_vocoder_ar_bwd_cond(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
                                         const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const float *cond_in,
                                         const void *saved, const float *grad_loss, const vqcpc_vocoder_ar_grads *grads, float *grad_cond,
                                         void *stream) {
    VQ_REQUIRE(cond_in && aligned16(cond_in), "vqcpc_vocoder_ar_bwd_cond: cond_in must be given and 16-byte aligned");
    return ar_bwd("vqcpc_vocoder_ar_bwd_cond", v, audio, idx, speaker, B, Tc, L, n_codes, n_audio, w, cond_in, saved, grad_loss, grads, grad_cond, stream);
}

namespace {

int ar_fwd(const char *what, vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
           const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const float *cond_in, double *nll_sum,
           int64_t *n_scored, int64_t *n_correct, float *cond, void *saved, void *stream) {
    VQ_REQUIRE(nll_sum && n_scored && n_correct, "%s: null argument", what);
    std::vector<int> slen;
    int longest = 0;
    TRY(check_call(v, what, audio, idx, speaker, B, Tc, L, n_codes, n_audio, w, saved, slen, &longest));
    VQ_REQUIRE(aligned16(cond), "%s: cond must be 16-byte aligned", what);
    hipStream_t s = (hipStream_t)stream;
    ArView view;
    TRY(view_of(v, w, true, &view, s));
    const int T2 = 2 * Tc, C = 2 * v->d.Hp;
    if (longest == 0 && cond) {                      // nothing to score: the scan's conditioning does not run, so it runs here
        UttLayout u;
        TRY(vq_tf_condition(v, idx, speaker, B, Tc, n_codes, slen, &view, u, s, cond_in));
    }
    TRY(vq_tf_score(v, audio, idx, speaker, B, Tc, L, n_codes, slen, longest, &view, nll_sum, n_scored, n_correct, nullptr, (float *)saved, s, cond_in));
    if (cond) vq_cond_rows(v->cond.as<float>(), cond, v->len.as<int>(), v->gbase.as<int>(), B, T2, C, true, s);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

int ar_bwd(const char *what, vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L,
           const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const float *cond_in, const void *saved,
           const float *grad_loss, const vqcpc_vocoder_ar_grads *grads, float *grad_cond, void *stream) {
    std::vector<int> slen;
    int longest = 0;
    TRY(check_call(v, what, audio, idx, speaker, B, Tc, L, n_codes, n_audio, w, saved, slen, &longest));
    const vqcpc_vocoder_ar_grads none{};
    const vqcpc_vocoder_ar_grads &g = grads ? *grads : none;
    bool any = grad_cond != nullptr;
    for (int i = 0; i < 9; ++i) {
        any = any || members(&g)[i];
        VQ_REQUIRE(aligned16(members(&g)[i]), "%s: the tensors of *grads must be 16-byte aligned", what);
    }
    VQ_REQUIRE(any, "%s: no wanted output (every member of *grads and grad_cond are NULL)", what);
    VQ_REQUIRE(aligned16(grad_cond) && ((uintptr_t)grad_loss & 3) == 0, "%s: grad_cond must be 16-byte aligned, grad_loss 4-byte", what);
    long long N = 0;
    for (int b = 0; b < B; ++b) N += slen[b];
    VQ_REQUIRE(N > 0, "%s: N = 0, no utterance has two samples: the mean over the scored samples does not exist", what);
    const float inv_n = (float)(1.0 / (double)N);

    hipStream_t s = (hipStream_t)stream;
    const auto &d = v->d;
    const int Hr = d.Hr, Hf = d.Hf, n_cls = d.n_cls, de = d.de, C = 2 * d.Hp, T2 = 2 * Tc, up = d.upsample_t, Tsv = L - 1;
    const int CH = v->tf_chunk_replays * v->steps_per_graph, nbt = (B + 15) / 16;
    const size_t M = (size_t)B * CH, F = sizeof(float);
    VQ_REQUIRE(M < ((size_t)1 << 26), "%s: B * chunk = %zu rows of one chunk do not fit the row index (< 2^26); lower tf_chunk_replays", what, M);
    const bool need_fc1 = g.fc1_weight || g.fc1_bias;
    const bool need_tabs = g.embedding || g.w_ih || g.b_ih || grad_cond, need_rnn = need_tabs || g.w_hh || g.b_hh;
    VocGradWork &k = v->gw;
    TRY(k.hcur.reserve(M * Hr * F));
    TRY(k.a1.reserve(M * Hf * F));
    TRY(k.dl.reserve(M * n_cls * F));
    if (need_fc1 || need_rnn) TRY(k.da.reserve(M * Hf * F));
    if (need_rnn) {
        TRY(k.hprev.reserve(M * Hr * F));
        TRY(k.gh.reserve(M * 3 * Hr * F));
        TRY(k.nn.reserve(M * Hr * F));
        TRY(k.dhh.reserve(M * Hr * F));
        TRY(k.dgi.reserve((size_t)B * (CH + 1) * 3 * Hr * F));
        TRY(k.dghn.reserve((size_t)B * (CH + 1) * Hr * F));
        TRY(k.carry.reserve(up256((size_t)B * Hr * F)));
    }
    ArView view;
    TRY(view_of(v, w, false, &view, s));
    UttLayout u;
    TRY(vq_tf_condition(v, idx, speaker, B, Tc, n_codes, slen, &view, u, s, cond_in));
    const size_t grows = (size_t)u.grows;            // > 0: some utterance scores a step, so it has a code
    if (need_tabs) {
        TRY(k.dGemb.reserve((size_t)n_cls * 3 * Hr * F));
        TRY(k.dGc.reserve(grows * 3 * Hr * F));
        HIP_TRY(hipMemsetAsync(k.dGemb.p, 0, (size_t)n_cls * 3 * Hr * F, s));
        HIP_TRY(hipMemsetAsync(k.dGc.p, 0, grows * 3 * Hr * F, s));
    }
    const size_t out_elems[9] = {(size_t)n_cls * de, (size_t)3 * Hr * (de + C), (size_t)3 * Hr * Hr, (size_t)3 * Hr, (size_t)3 * Hr,
                                 (size_t)Hf * Hr, (size_t)Hf, (size_t)n_cls * Hf, (size_t)n_cls};
    for (int i = 0; i < 9; ++i)
        if (members(&g)[i]) HIP_TRY(hipMemsetAsync(members(&g)[i], 0, out_elems[i] * F, s));
    if (grad_cond) HIP_TRY(hipMemsetAsync(grad_cond, 0, (size_t)B * T2 * C * F, s));

    // the plain tensors the products read: the caller's, or the handle's copies
    const float *w_hh = w ? w->w_hh : v->w_hh.as<float>(), *b_hh = w ? w->b_hh : v->b_hh.as<float>();
    const float *emb = w ? w->embedding : v->ar_emb.as<float>();
    const float *w_emb = w ? w->w_ih : v->w_emb.as<float>(), *w_cond = w ? w->w_ih + de : v->w_cond.as<float>();
    const int ld_emb = w ? de + C : de, ld_cond = w ? de + C : C;
    const int *slen_dev = v->nll_len.as<int>(), *frames = v->len.as<int>(), *gbase = v->gbase.as<int>();
    float *Hc = k.hcur.as<float>(), *Hp = k.hprev.as<float>(), *gh = k.gh.as<float>(), *nn = k.nn.as<float>(), *a1 = k.a1.as<float>();
    float *dl = k.dl.as<float>(), *da = k.da.as<float>(), *dhh = k.dhh.as<float>(), *dgi = k.dgi.as<float>(), *dghn = k.dghn.as<float>();

    const int nch = (longest + CH - 1) / CH;
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int t0 = ch * CH, n = longest - t0 < CH ? longest - t0 : CH;
        const VocRows q{slen_dev, audio, B, L, CH, t0, Hr};
        const dim3 gh4((unsigned)((CH * (Hr / 4) + 255) / 256), B), ghr((unsigned)((CH * Hr + 255) / 256), B);
        hipLaunchKernelGGL(voc_gather_h_kernel, gh4, dim3(256), 0, s, (const float4 *)saved, (float4 *)Hc, (float4 *)(need_rnn ? Hp : nullptr),
                           slen_dev, CH, t0, Hr / 4, Tsv);
        // head
        TRY(vq_gemm_chain_ex(Hc, Hr, view.w_fc1, view.b_fc1, a1, Hf, (int)M, Hf, Hr, Hr, 1, 0, 0, 0, 0, s));
        TRY(vq_gemm_chain(a1, Hf, view.w_fc2, view.b_fc2, dl, n_cls, (int)M, n_cls, Hf, Hf, s));
        hipLaunchKernelGGL(voc_softmax_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, dl, q, grad_loss, inv_n);
        const int R = (int)M;
        if (g.fc2_weight) vq_grad_atb(dl, n_cls, a1, Hf, g.fc2_weight, Hf, R, n_cls, Hf, s);
        if (g.fc2_bias) vq_grad_colsum(dl, n_cls, g.fc2_bias, R, n_cls, s);
        if (need_fc1 || need_rnn) launch_rows_w(dl, view.w_fc2, Hf, da, VocRowMap{a1, Hf, nullptr, nullptr, 1}, R, n_cls, s);
        if (g.fc1_weight) vq_grad_atb(da, Hf, Hc, Hr, g.fc1_weight, Hr, R, Hf, Hr, s);
        if (g.fc1_bias) vq_grad_colsum(da, Hf, g.fc1_bias, R, Hf, s);
        if (!need_rnn) continue;
        vq_grad_rows_w(da, view.w_fc1, Hr, dhh, R, Hf, Hr, s);
        // gates again
        TRY(vq_gemm_chain(Hp, Hr, w_hh, b_hh, gh, 3 * Hr, (int)M, 3 * Hr, Hr, Hr, s));
        hipLaunchKernelGGL(voc_gates_kernel, ghr, dim3(256), 0, s, gh, nn, view.Gemb, v->gcond.as<float>(), gbase, q, up);
        // the serial part
        VocStepP sp{w_hh, gh, nn, Hp, dhh, dgi, dghn, k.carry.as<float>(), q, longest};
        const dim3 grid(Hr / 16, nbt);
        for (int t = t0 + n - 1; t >= t0; --t) {
            if (Hr == 512) hipLaunchKernelGGL((voc_bwd_step_kernel<24>), grid, dim3(256), 0, s, sp, t);
            else if (Hr == 896) hipLaunchKernelGGL((voc_bwd_step_kernel<42>), grid, dim3(256), 0, s, sp, t);
            else hipLaunchKernelGGL((voc_bwd_step_kernel<48>), grid, dim3(256), 0, s, sp, t);
        }
        // the chunk's sums
        const dim3 blk(256);
        if (g.w_hh) hipLaunchKernelGGL(grad_atb_kernel<VocAtb<ATB_WHH>>, dim3(Hr / 16, 3 * Hr / 64), blk, 0, s, VocAtb<ATB_WHH>{dgi, dghn, Hp, q, g.w_hh, Hr, R});
        if (g.b_hh) hipLaunchKernelGGL(grad_colsum_kernel<VocAtb<ATB_WHH>>, dim3(3 * Hr / 64), blk, 0, s, VocAtb<ATB_WHH>{dgi, dghn, Hp, q, g.b_hh, 0, R});
        if (need_tabs) {
            hipLaunchKernelGGL(grad_atb_kernel<VocAtb<ATB_GEMB>>, dim3(3 * Hr / 16, n_cls / 64), blk, 0, s,
                               VocAtb<ATB_GEMB>{dgi, dghn, Hp, q, k.dGemb.as<float>(), 3 * Hr, R});
            hipLaunchKernelGGL(voc_frame_sum_kernel, dim3(B * T2, (3 * Hr + 255) / 256), dim3(256), 0, s, dgi, k.dGc.as<float>(), frames, gbase, q, T2, up);
        }
        if (ch > 0) hipLaunchKernelGGL(voc_keep_first_kernel, dim3((4 * Hr + 255) / 256, B), dim3(256), 0, s, dgi, dghn, CH, Hr);
    }
    if (need_tabs) {
        float *dGemb = k.dGemb.as<float>(), *dGc = k.dGc.as<float>();
        if (g.w_ih) {
            vq_grad_atb(dGemb, 3 * Hr, emb, de, g.w_ih, de + C, n_cls, 3 * Hr, de, s);
            vq_grad_atb(dGc, 3 * Hr, v->cond.as<float>(), C, g.w_ih + de, de + C, (int)grows, 3 * Hr, C, s);
        }
        if (g.b_ih) vq_grad_colsum(dGc, 3 * Hr, g.b_ih, (int)grows, 3 * Hr, s);
        if (g.embedding) vq_grad_rows_w(dGemb, w_emb, ld_emb, g.embedding, n_cls, 3 * Hr, de, s);
        if (grad_cond) launch_rows_w(dGc, w_cond, ld_cond, grad_cond, VocRowMap{nullptr, C, frames, gbase, T2}, (long long)B * T2, 3 * Hr, s);
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

}  // namespace
