// Gradients of the context LSTM, Encoder.rnn = nn.LSTM(z_dim, c_dim) (model.py:57, :69, :85): a forward that keeps what the
// backward reads again, and back-propagation through time -- what loss.backward() does to the LSTM in train_cpc.py:116-124.
// B utterances, T steps, D = z_dim, H = c_dim, rows r = b T + t, R = B T.  Gate order i, f, g, o (PyTorch).  a = pre-activations.
// Every sum has ONE order, fixed by the code and independent of the grid's timing: no floating-point read-modify-write on global
// memory, no wait on another workgroup; launch boundaries order the steps and the passes.  Equal inputs give equal bits.
// Every operation below is one separately rounded fp32 operation (-ffp-contract=off); "chain" = fp32 fmas from 0.
//
// Forward (vq_ctx_fwd): vq_lstm_project and vq_lstm_steps of scan.hip, the two functions that ARE vq_lstm_run's launch-per-step
//   path, over this work space's own scratch and with a SeqSave (seq_step_save_kernel) -> the same bits of c at every B (the
//   resident single-utterance scan is not used).  `saved` = gates (R, 4H) i | f | g | o after their non-linearities, cell state
//   (R, H), tanh(cell) (R, H).
//
// Backward scan: ctx_bwd_step_kernel<NS>, grid (H / 16, ceil(B / 16)), one launch per step t = T-1 .. 0.  Workgroup (rg, bt) owns
//   hidden units 16 rg .. + 15 of utterances 16 bt .. + 15.
//   dh_rec[b, u] = sum_k W_hh[k, u] dA[t+1][b, k], k < 4H: bptt_step_product of bptt_step.h (the order: there), NS = H / 16, with
//     W_hh^T in fragment order (build_wfrag_t_kernel).  At t = T-1 there is no MFMA: dh_rec = +0.
//   then per (b, u), with i f g o, tc = tanh(c_t), cp = c_{t-1} (0 at t = 0), gc = grad_c[b, t, u], carry (0 at t = T-1):
//     dh  = gc + dh_rec                     do_ = dh * tc
//     dct = (dh * o) * (1 - tc * tc) + carry
//     da_i = (dct * g) * (i * (1 - i))      da_f = (dct * cp) * (f * (1 - f))
//     da_g = (dct * i) * (1 - g * g)        da_o = do_ * (o * (1 - o))
//     carry' = dct * f
//   dA[t] goes to rows (R, 4H) of the work space, carry' to (B, H).
// After the scan (a pass whose products nobody asked for is not launched):
//   dW_ih = dA^T z and dW_hh = dA^T h_prev (h_prev of row (b, t) = c[b, t-1], zero at t = 0): ctx_grad_w_kernel, ONE kernel for
//     both, grid (column tiles of 16 over [z | h_prev], 4H / 64, slabs).  A slab is GRAD_SLAB = 1024 consecutive rows.  Inside a slab
//     MFMA (s, c) takes rows r0 + 16 s + 4 q + c, q = 0 .. 3 summed inside the instruction; c even goes to accumulator 0, c odd to
//     accumulator 1, s ascending, the two added once at the end.  ctx_grad_w_finish_kernel adds the slab partials in slab order.
//     (slab_mfma_tile of grad_slab.h, the statements cpc_grad_w_kernel runs with its own row maps.)
//   db (b_ih and b_hh receive the same values): ctx_grad_b_kernel, grid (slabs, 4H / 64), the same slabs: thread (column, row
//     group rg) adds rows r0 + rg + 4 i, i ascending, into four accumulators (i mod 4) combined (a0 + a1) + (a2 + a3); the four row
//     groups are combined the same way (slab_column_sum of grad_slab.h); the slab partials go through the finish kernel as a column
//     of their own.
//   dz = dA W_ih: vq_grad_rows_w (grad_rows.hip), one 16 x 16 tile per workgroup, k < 4H over the four waves in the order of dh_rec.
//
// Padding and dirt: the utterance columns b >= B of the last tile are MASKED -- their lanes load nothing (exact zeros enter the
// MFMA, an output column depends on its own input column only) and store nothing; rows r >= R likewise.  The scan reads dA[t+1] and
// the carry only after step t+1 of the same call wrote them for every b < B, and the slab partials of a column tile are read only
// where this call wrote them: whatever an earlier call left in the work space never reaches a result.  Nothing is zero-filled.
#include "seq_step.h"
#include "bptt_step.h"
#include "grad_slab.h"

namespace {

// W_hh^T in fragment order: WfT[((rg * 4 + w) * NS + s) * 64 + lane] (float4) = W_hh[16 S + 4 (lane >> 4) + 0 .. 3][16 rg + (lane & 15)],
// S = w NS + s, NS = K / 64 (the K gate rows of W_hh over four waves: K = 4H here, 3H for the prenet's GRU layers in prenet_grad.hip).
__global__ void build_wfrag_t_kernel(const float *__restrict__ w_hh, float4 *__restrict__ WfT, int H, int K) {
    const size_t total = (size_t)(H / 16) * (K / 16) * 64;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int lane = (int)(id & 63);
    const int S = (int)((id >> 6) % (size_t)(K / 16)), rg = (int)((id >> 6) / (size_t)(K / 16));
    const float *src = w_hh + (size_t)(16 * S + 4 * (lane >> 4)) * H + 16 * rg + (lane & 15);
    WfT[id] = make_float4(src[0], src[H], src[2 * (size_t)H], src[3 * (size_t)H]);
}

struct CtxBwdP {
    const float4 *WfT;
    const float *gates, *cell, *tanhc;   // saved
    const float *grad_c;                 // (R, H)
    float *dA;                           // (R, 4H)
    float *carry;                        // (B, H)
    int H, B, T;
};

template <int NS>
__global__ __launch_bounds__(256) void ctx_bwd_step_kernel(CtxBwdP p, int t) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = blockIdx.x, bt = blockIdx.y, H = p.H, T = p.T;
    const bool last = t + 1 >= T;
    // the element-wise operands of thread (utterance tid >> 4, unit tid & 15) are requested first: they do not depend on the product
    const int bg = bt * 16 + (tid >> 4), unit = 16 * rg + (tid & 15);
    const bool act = bg < p.B;
    const size_t row = (size_t)bg * T + t;
    float gc = 0.f, ig = 0.f, fg = 0.f, gg = 0.f, og = 0.f, tc = 0.f, cp = 0.f, carry = 0.f;
    if (act) {
        gc = p.grad_c[row * H + unit];
        const float *gs = p.gates + row * (4 * H) + unit;
        ig = gs[0]; fg = gs[H]; gg = gs[2 * H]; og = gs[3 * H];
        tc = p.tanhc[row * H + unit];
        if (t > 0) cp = p.cell[(row - 1) * H + unit];
        if (!last) carry = p.carry[(size_t)bg * H + unit];
    }
    float dh_rec = 0.f;
    if (!last) {                                     // uniform over the grid
        const int bcol = bt * 16 + (lane & 15);
        const bool live = bcol < p.B;                // a masked column loads nothing
        const float4 *dp = (const float4 *)(p.dA + ((size_t)(live ? bcol : 0) * T + t + 1) * (4 * H)) + (size_t)wave * NS * 4 + (lane >> 4);
        const float4 *wp = p.WfT + ((size_t)(rg * 4 + wave) * NS) * 64 + lane;
        dh_rec = bptt_step_product<NS, 4>([&](int s) { return wp[s * 64]; },
                                          [&](int s) { return live ? dp[4 * s] : make_float4(0.f, 0.f, 0.f, 0.f); });
    }
    if (act) {
        const float dh = gc + dh_rec;
        const float do_ = dh * tc;
        const float dct = (dh * og) * (1.0f - tc * tc) + carry;
        float *da = p.dA + row * (4 * H) + unit;
        da[0] = (dct * gg) * (ig * (1.0f - ig));
        da[H] = (dct * cp) * (fg * (1.0f - fg));
        da[2 * H] = (dct * ig) * (1.0f - gg * gg);
        da[3 * H] = do_ * (og * (1.0f - og));
        p.carry[(size_t)bg * H + unit] = dct * fg;
    }
}

// part (slabs, 4H, ld), ld = D + H + 16: columns [0, D) dW_ih, [D, D + H) dW_hh, column D + H the bias partial (the rest pads the row).
__global__ __launch_bounds__(256) void ctx_grad_w_kernel(const float *dA, const float *z, const float *c, float *part, int R, int T,
                                                         int D, int H, int ct0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, ks = lane >> 4;
    const int ct = ct0 + blockIdx.x, m0 = blockIdx.y * 64, slab = blockIdx.z;
    const int M = 4 * H, ld = D + H + 16, r0 = slab * GRAD_SLAB;      // R < 2^31 (the entry checks it)
    const bool from_z = ct * 16 < D;
    const int col = from_z ? ct * 16 + i : ct * 16 - D + i;           // of z, or of h_prev
    const auto a = [&](int r) { return dA[(size_t)r * M + m0 + wave * 16 + i]; };
    const f32x4 acc = from_z ? slab_mfma_tile(R, r0, ks, a, [&](int r) { return z[(size_t)r * D + col]; })
                             : slab_mfma_tile(R, r0, ks, a, [&](int r) { return r % T != 0 ? c[(size_t)(r - 1) * H + col] : 0.f; });   // h_prev: zero at t = 0
#pragma unroll
    for (int r = 0; r < 4; ++r)                          // row = gate row m0 + 16 wave + 4 ks + r, column = ct * 16 + i
        part[((size_t)slab * M + m0 + wave * 16 + ks * 4 + r) * ld + ct * 16 + i] = acc[r];
}

__global__ __launch_bounds__(256) void ctx_grad_b_kernel(const float *dA, float *part, int R, int D, int H) {
    __shared__ float red[4][64];
    const int d = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int slab = blockIdx.x, m = blockIdx.y * 64 + d, M = 4 * H, ld = D + H + 16;
    const float sum = slab_column_sum(dA + m, M, R, (long long)slab * GRAD_SLAB, rg, d, red);
    if (rg == 0) part[((size_t)slab * M + m) * ld + D + H] = sum;
}

__global__ __launch_bounds__(256) void ctx_grad_w_finish_kernel(const float *part, float *dW_ih, float *dW_hh, float *db, int S, int D, int H) {
    const int M = 4 * H, ld = D + H + 16, cols = D + H + 1;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;           // (m, col), col <= D + H
    if (e >= (size_t)M * cols) return;
    const int col = (int)(e % cols), m = (int)(e / cols);
    float *dst = col < D ? (dW_ih ? dW_ih + (size_t)m * D + col : nullptr)
               : col < D + H ? (dW_hh ? dW_hh + (size_t)m * H + col - D : nullptr) : (db ? db + m : nullptr);
    if (!dst) return;                                                  // not asked for: its partials were not written either
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += part[((size_t)s * M + m) * ld + col];
    *dst = sum;
}

}  // namespace

void vq_build_wfrag_t(const float *w_hh, float *WfT, int H, int K, hipStream_t s) {
    const size_t nfrag = (size_t)(H / 16) * (K / 16) * 64;
    hipLaunchKernelGGL(build_wfrag_t_kernel, dim3((unsigned)((nfrag + 255) / 256)), dim3(256), 0, s, w_hh, (float4 *)WfT, H, K);
}

size_t vq_ctx_saved_bytes(int B, int T, int H) { return (size_t)B * T * 6 * H * sizeof(float); }

static SeqSave saved_view(const float *saved, int B, int T, int H) {
    float *s = const_cast<float *>(saved);
    const size_t R = (size_t)B * T;
    return SeqSave{s, s + R * 4 * H, s + R * 5 * H};
}

int vq_ctx_fwd(CtxGradWork &k, LstmWeights w, bool own_weights, const float *b_ih, const float *b_hh, const float *z, int B, int T,
               float *c, float *saved, hipStream_t s) {
    const int H = w.H;
    if (own_weights) {                                   // what vq_lstm_plan_create builds, from the caller's tensors, in stream order
        TRY(k.bias.reserve((size_t)4 * H * sizeof(float)));
        vq_add_vec(b_ih, b_hh, k.bias.as<float>(), 4 * H, s);
        TRY(vq_build_wfrag(w.w_hh, H, H / 4, H, 4, 4, H, k.Wf, s));
        w.bias = k.bias.as<float>(); w.Wf = k.Wf.as<float>();
    }
    TRY(vq_lstm_project(k.fwd, w, z, B, T, s));
    const SeqSave sv = saved_view(saved, B, T, H);
    return vq_lstm_steps(k.fwd, w, B, T, c, &sv, s);
}

int vq_ctx_bwd(CtxGradWork &k, LstmWeights w, const float *z, int B, int T, const float *c, const float *saved, const float *grad_c,
               float *grad_z, float *grad_w_ih, float *grad_w_hh, float *grad_bias, hipStream_t s) {
    const int H = w.H, D = w.D, nbt = (B + 15) / 16, M = 4 * H;
    const long long R = (long long)B * T;
    const int slabs = (int)((R + GRAD_SLAB - 1) / GRAD_SLAB), ld = D + H + 16;
    const bool want_w = grad_w_ih || grad_w_hh || grad_bias;
    TRY(k.WfT.reserve((size_t)H * M * sizeof(float)));
    TRY(k.dA.reserve(up256((size_t)R * M * sizeof(float))));
    TRY(k.carry.reserve(up256((size_t)B * H * sizeof(float))));
    if (want_w) TRY(k.part.reserve(up256((size_t)slabs * M * ld * sizeof(float))));
    vq_build_wfrag_t(w.w_hh, k.WfT.as<float>(), H, M, s);
    const SeqSave sv = saved_view(saved, B, T, H);
    CtxBwdP p{};
    p.WfT = k.WfT.as<float4>(); p.gates = sv.gates; p.cell = sv.cell; p.tanhc = sv.tanhc; p.grad_c = grad_c;
    p.dA = k.dA.as<float>(); p.carry = k.carry.as<float>(); p.H = H; p.B = B; p.T = T;
    const dim3 blk(256), grid(H / 16, nbt);
    for (int t = T - 1; t >= 0; --t) {
        const bool built = vq_with_sw(H / 64, [&](auto sw) {
            hipLaunchKernelGGL((ctx_bwd_step_kernel<4 * decltype(sw)::value>), grid, blk, 0, s, p, t);
        });
        if (!built) { vq_set_error("context backward: hidden size %d unsupported", H); return VQCPC_ERR_INVALID; }
    }
    const float *dA = k.dA.as<float>();
    if (want_w) {
        float *part = k.part.as<float>();
        // the column tiles of [z | h_prev] somebody asked for: one launch when both are, else the one range
        const int ct_lo = grad_w_ih ? 0 : D / 16, ct_hi = grad_w_hh ? (D + H) / 16 : D / 16;
        if (ct_hi > ct_lo)
            hipLaunchKernelGGL(ctx_grad_w_kernel, dim3(ct_hi - ct_lo, M / 64, slabs), blk, 0, s, dA, z, c, part, (int)R, T, D, H, ct_lo);
        if (grad_bias) hipLaunchKernelGGL(ctx_grad_b_kernel, dim3(slabs, M / 64), blk, 0, s, dA, part, (int)R, D, H);
        const size_t outs = (size_t)M * (D + H + 1);
        hipLaunchKernelGGL(ctx_grad_w_finish_kernel, dim3((unsigned)((outs + 255) / 256)), blk, 0, s, part, grad_w_ih, grad_w_hh, grad_bias,
                           slabs, D, H);
    }
    if (grad_z) vq_grad_rows_w(dA, w.w_ih, D, grad_z, (int)R, M, D, s);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
