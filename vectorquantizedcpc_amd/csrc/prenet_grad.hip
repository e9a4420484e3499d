// Gradients of the vocoder's conditioning path (network_vocoder.py:73-77 and rnnms.prenet): code_embedding, speaker_embedding, the
// repeat of every code over two frames, and the two bidirectional GRU layers -- vqcpc_vocoder_cond_fwd / _bwd of
// include/vqcpc.h (K16).  B utterances, utterance b has len[b] = 2 n_codes[b] frames at rows row0[b] .. of every
// buffer below (run_condition's layout), R rows in all.  dz, ds: the embedding widths, F = dz + ds, Hp = dim_voc_latent / 2.
// Layer l reads X (R, I), I = F (l = 0, the glued series) or 2Hp (l = 1, layer 0's output), and writes Hout (R, 2Hp) = [forward |
// reverse].  Gate order r, z, n; h = (1 - z) n + z h_prev.  The forward direction's step s is frame s, the reverse direction's is
// frame len[b] - 1 - s (seq_step.h): h_prev of the reverse direction at frame t is h at t + 1.
// Every sum has ONE order, fixed by the code and independent of the grid's timing: no floating-point read-modify-write that two
// workgroups share, no wait on another workgroup; launch boundaries order the steps and the passes.  Equal inputs give equal bits.
// Every operation below is one separately rounded fp32 operation (-ffp-contract=off); "chain" = fp32 fmas from 0.
//
// Forward (vqcpc_vocoder_cond_fwd): vq_cond_run of vocoder_host.hip -- run_condition, the function that IS vqcpc_vocoder_condition and
//   the conditioning of every decode and scoring call: glue_kernel, vq_gemm_chain, vq_bigru_scan per layer -- writing the glued series
//   and both layers' outputs into `saved` = series (B T2, F) | out0 (B T2, 2Hp) | out1 (B T2, 2Hp), the first R rows of each used.
//   With a caller's weights the stacked w_ih / b_ih / b_hh (copies in stream order) and the W_hh fragments (vq_build_wfrag, the
//   kernel create uses) are made first, into the handle's work space.
//
// Backward (vqcpc_vocoder_cond_bwd), layer 1 then layer 0; dOut (R, 2Hp) = grad_cond's rows of the utterances' own frames (layer 1)
//   or layer 1's dX (layer 0).  Wanted weight outputs are zero-filled first.  Per layer:
//   1. pre_hprev_kernel: Hprev (R, 2Hp) from Hout: forward half h at t - 1 (zero at t = 0), reverse half h at t + 1 (zero at the
//      utterance's last frame).
//   2. Gates again, batched: gi = X W_ih^T + b_ih (both directions stacked, the forward's own product and bits), gh[d] = Hprev[d]
//      W_hh[d]^T + b_hh[d] (vq_gemm_chain: bias + chain over k ascending); pre_gates_kernel: r = sigmoid(gi_r + gh_r),
//      z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n) (libm expf / tanhf).  These are not the forward's bits (it adds
//      gi + (W_hh h + b) with the product in MFMA order); the float64 judge bounds the result.
//   3. The serial part, pre_bwd_step_kernel, grid (Hp / 16, 2 directions, ceil(B / 16)), ONE launch per step s = longest - 1 .. 0.
//      Workgroup (rg, d, bt) owns hidden units 16 rg .. + 15 of direction d of utterances 16 bt .. + 15.  Utterance b is live where
//      s < len[b], at frame f(s) = s (d = 0) or len[b] - 1 - s (d = 1).
//        dh_rec[b, u] = sum_k W_hh[d][k, u] dgh[f(s + 1)][b, d, k], k < 3Hp: bptt_step_product of bptt_step.h (the order: there),
//          NS = 3Hp / 64, with W_hh^T in fragment order (vq_build_wfrag_t).  No MFMA at s = longest - 1.  Where s + 1 >= len[b] -- the
//          utterance's first step of the backward -- dh_rec and the carry are exactly 0 by that mask, whatever the work space holds.
//        dh = (dOut + dh_rec) + carry
//        gru_cell_bwd of bptt_step.h: dn = dh (1 - z)    dz = dh (h_prev - n)
//        da_n = dn (1 - n n)    da_z = dz (z (1 - z))    da_r = (da_n gh_n) (r (1 - r))
//        dgi = (da_r, da_z, da_n)    dgh = (da_r, da_z, da_n r)    carry' = dh z
//      dgi and dgh go to rows (R, 6Hp) = [d][3Hp] of the work space, carry' to (2, B, Hp).
//   4. The layer's sums over all R rows, per direction d, by vq_grad_atb and vq_grad_colsum (grad_rows.hip; the orders:
//      grad_slab.h), each added to the zero-filled output:
//        dW_ih[d] = dgi[d]^T X    dW_hh[d] = dgh[d]^T Hprev[d]    db_ih[d] = sum dgi[d]    db_hh[d] = sum dgh[d].
//   5. dX = dgi W_ih over BOTH directions in one order (vq_grad_rows_w, K = 6Hp).  Launched only if something in front of it is
//      wanted: it is layer 0's dOut, and at layer 0 it is dseries (R, F).
//   The tables, from dseries: pre_keys_kernel writes every row's (clamped) code index and speaker id; grad_atb_kernel with PreTable's
//   operands, one 16 x 16 tile per wave: out[k, c] = sum over the rows r with key[r] = k of dseries[r, c], as onehot(key)^T dseries
//   in the slab order of 4 -- K15's dGemb form.  A row of codes or speakers the batch never names is a sum of (+-0) from +0, i.e. +0.
//
// Work space (CondGradWork, beside what the forward uses), floats: R (2Hp + 6Hp + 2Hp + 2Hp + 6Hp + 6Hp + 6Hp + F) + 2 B Hp + one
//   layer's W_hh^T fragments 6 Hp Hp + 2 R ints, plus for a caller's weights the stacked copies and fragments.
//
// Padding and dirt: the utterance columns b >= B of the last tile are masked (their lanes load nothing and store nothing), steps
// past an utterance's frames likewise; the scan reads dgh and the carry only where step s + 1 of the same call wrote them.  Whatever
// an earlier call left in the work space never reaches a result.
#include "vocoder_internal.h"
#include "bptt_step.h"
#include "grad_slab.h"

namespace {

// grid (B T2, ceil(2Hp / 256))
__global__ void pre_hprev_kernel(const float *__restrict__ Hout, float *__restrict__ Hprev, const int *__restrict__ len,
                                 const int *__restrict__ row0, int T2, int Hp) {
    const int j = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x / T2, f = blockIdx.x % T2;
    const int L = len[b];
    if (j >= 2 * Hp || f >= L) return;
    const size_t row = (size_t)row0[b] + f;
    float h = 0.f;
    if (j < Hp) { if (f > 0) h = Hout[(row - 1) * 2 * Hp + j]; }
    else if (f + 1 < L) h = Hout[(row + 1) * 2 * Hp + j];
    Hprev[row * 2 * Hp + j] = h;
}

// gh (R, 6Hp) = [d] gh_r | gh_z | gh_n in, [d] r | z | gh_n out; nn (R, 2Hp) = n.  grid (ceil(R 2Hp / 256))
__global__ void pre_gates_kernel(const float *__restrict__ gi, float *__restrict__ gh, float *__restrict__ nn, size_t R, int Hp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * 2 * Hp) return;
    const size_t row = i / (2 * Hp);
    const int j = (int)(i % (2 * Hp)), d = j / Hp, u = j % Hp;
    const size_t o = row * 6 * Hp + (size_t)d * 3 * Hp + u;
    const float r = sigmoidf_(gi[o] + gh[o]);
    const float z = sigmoidf_(gi[o + Hp] + gh[o + Hp]);
    const float n = tanhf(gi[o + 2 * Hp] + r * gh[o + 2 * Hp]);
    gh[o] = r; gh[o + Hp] = z;
    nn[i] = n;
}

struct PreStepP {
    const float4 *WfT;                   // [d][(Hp / 16) (3Hp / 16) 64]
    const float *gh, *nn, *hprev, *dout; // (R, 6Hp) r | z | gh_n; (R, 2Hp) n; h_prev; dOut
    float *dgi, *dgh;                    // (R, 6Hp)
    float *carry;                        // (2, B, Hp)
    const int *len, *row0;               // frames and first row per utterance
    int Hp, B, longest;
};

template <int NS>                        // 3Hp / 64
__global__ __launch_bounds__(256) void pre_bwd_step_kernel(PreStepP p, int s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = blockIdx.x, d = blockIdx.y, bt = blockIdx.z, Hp = p.Hp;
    // the element-wise operands of thread (utterance tid >> 4, unit tid & 15) are requested first: they do not depend on the product
    const int bg = bt * 16 + (tid >> 4), unit = 16 * rg + (tid & 15);
    const int L = bg < p.B ? p.len[bg] : 0;
    const bool act = s < L, rec = s + 1 < L;         // rec: step s + 1 of this utterance ran -- else its BPTT starts here, from 0
    const size_t row = act ? (size_t)p.row0[bg] + (d == 0 ? s : L - 1 - s) : 0;
    float r = 0.f, z = 0.f, hn = 0.f, n = 0.f, hp = 0.f, dout = 0.f, carry = 0.f;
    if (act) {
        const float *g = p.gh + row * (6 * Hp) + (size_t)d * 3 * Hp + unit;
        r = g[0]; z = g[Hp]; hn = g[2 * Hp];
        n = p.nn[row * (2 * Hp) + d * Hp + unit];
        hp = p.hprev[row * (2 * Hp) + d * Hp + unit];
        dout = p.dout[row * (2 * Hp) + d * Hp + unit];
        if (rec) carry = p.carry[((size_t)d * p.B + bg) * Hp + unit];
    }
    float dh_rec = 0.f;
    if (s + 1 < p.longest) {                         // uniform over the grid
        const int bcol = bt * 16 + (lane & 15);
        const int Lc = bcol < p.B ? p.len[bcol] : 0;
        const bool live = s + 1 < Lc;                // a masked column loads nothing
        const size_t nrow = live ? (size_t)p.row0[bcol] + (d == 0 ? s + 1 : Lc - 2 - s) : 0;
        const float4 *dp = (const float4 *)(p.dgh + nrow * (6 * Hp) + (size_t)d * 3 * Hp) + (size_t)wave * NS * 4 + (lane >> 4);
        const float4 *wp = p.WfT + ((size_t)d * (Hp / 16) * 4 + (size_t)(rg * 4 + wave)) * NS * 64 + lane;
        dh_rec = bptt_step_product<NS, 3>([&](int q) { return wp[q * 64]; },
                                          [&](int q) { return live ? dp[4 * q] : make_float4(0.f, 0.f, 0.f, 0.f); });
    }
    if (act) {
        if (!rec) dh_rec = 0.f;
        const GruCellGrad c = gru_cell_bwd(r, z, hn, n, hp, (dout + dh_rec) + carry);
        const size_t o = row * (6 * Hp) + (size_t)d * 3 * Hp + unit;
        p.dgi[o] = c.gr; p.dgi[o + Hp] = c.gz; p.dgi[o + 2 * Hp] = c.gn;
        p.dgh[o] = c.gr; p.dgh[o + Hp] = c.gz; p.dgh[o + 2 * Hp] = c.gn_r;
        p.carry[((size_t)d * p.B + bg) * Hp + unit] = c.carry;
    }
}

// keys[row] = the row's code index, keys[R + row] = its speaker id, both clamped as glue_kernel clamps them.  grid (B T2)
__global__ void pre_keys_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ spk, int *__restrict__ keys, const int *__restrict__ len,
                                const int *__restrict__ row0, int T2, int Tc, int n_codes, int n_spk, size_t R) {
    const int b = blockIdx.x / T2, f = blockIdx.x % T2;
    if (threadIdx.x != 0 || f >= len[b]) return;
    const size_t row = (size_t)row0[b] + f;
    long long z = idx[(size_t)b * Tc + f / 2], sp = spk[b];
    z = z < 0 ? 0 : (z >= n_codes ? n_codes - 1 : z);
    sp = sp < 0 ? 0 : (sp >= n_spk ? n_spk - 1 : sp);
    keys[row] = (int)z;
    keys[R + row] = (int)sp;
}

// out (Nk, ncol): out[k, c] = sum over the rows with key[r] == k of D[r, c0 + c], as onehot(key)^T D by grad_atb_kernel (grad_slab.h),
// grid (ceil(ncol / 16), ceil(Nk / 64)).
struct PreTable {
    const int *key; const float *D; int ld, c0, ncol;
    float *out; int Nk, R;
    __device__ float a(int r, int m) const { return key[r] == m ? 1.f : 0.f; }
    __device__ float b(int r, int c) const { return c < ncol ? D[(size_t)r * ld + c0 + c] : 0.f; }
    __device__ void put(int k, int c, float v) const { if (k < Nk && c < ncol) out[(size_t)k * ncol + c] = v; }
};

const float *const *members(const vqcpc_vocoder_cond_weights *w) { return &w->code_embedding; }     // eighteen pointers in a row
float *const *members(const vqcpc_vocoder_cond_grads *g) { return &g->code_embedding; }
constexpr int N_COND = 18;

// What both entries check before anything is enqueued; the layout of the call's utterances.
int check_call(vqcpc_vocoder *v, const char *what, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes,
               const vqcpc_vocoder_cond_weights *cw, const void *saved, const float *cond, CallPlan &cp) {
    VQ_REQUIRE(v && idx && speaker && saved && cond, "%s: null argument", what);
    TRY(vq_require_device(v->device, what));
    VQ_REQUIRE(B >= 1 && Tc >= 1, "%s: need B >= 1 and Tc >= 1 (got %d, %d)", what, B, Tc);
    VQ_REQUIRE(B <= 65535 && (long long)B * 2 * Tc < (1ll << 31) / 8, "%s: B = %d utterances of %d frames do not fit the row index "
               "(B <= 65535, B * 2 Tc < 2^28)", what, B, 2 * Tc);
    VQ_REQUIRE(aligned16(saved) && aligned16(cond), "%s: saved and the conditioning series must be 16-byte aligned", what);
    if (cw)
        for (int i = 0; i < N_COND; ++i) {
            VQ_REQUIRE(members(cw)[i], "%s: all eighteen tensors of the conditioning path are required in *cw", what);
            VQ_REQUIRE(aligned16(members(cw)[i]), "%s: the tensors of *cw must be 16-byte aligned", what);
        }
    return utt_layout(B, Tc, n_codes, v->d.upsample_t, 0, nullptr, cp);        // n_codes[b] in [0, Tc]
}

// The stacked layouts of CondView from a caller's tensors, enqueued on s into v->cg.  scan: also the W_hh fragments the scan reads.
int cond_relayout(vqcpc_vocoder *v, const vqcpc_vocoder_cond_weights *cw, bool scan, CondView *out, hipStream_t s) {
    const auto &d = v->d;
    const int Hp = d.Hp, F = d.dz + d.ds;
    const hipMemcpyKind D2D = hipMemcpyDeviceToDevice;
    CondGradWork &k = v->cg;
    CondView c{};
    c.code_emb = cw->code_embedding; c.spk_emb = cw->speaker_embedding;
    const size_t frag = (size_t)(Hp / 4) * (Hp / 16) * 64 * sizeof(float4);      // one direction's fragments
    for (int l = 0; l < 2; ++l) {
        const size_t I = l == 0 ? F : 2 * Hp, nw = (size_t)3 * Hp * I * sizeof(float), nb = (size_t)3 * Hp * sizeof(float);
        TRY(k.wih[l].reserve(2 * nw));
        TRY(k.bih[l].reserve(2 * nb));
        TRY(k.bhh[l].reserve(2 * nb));
        if (scan) TRY(k.wf[l].reserve(2 * frag));
        for (int dir = 0; dir < 2; ++dir) {
            HIP_TRY(hipMemcpyAsync((char *)k.wih[l].p + dir * nw, cw->prenet_w_ih[l][dir], nw, D2D, s));
            HIP_TRY(hipMemcpyAsync((char *)k.bih[l].p + dir * nb, cw->prenet_b_ih[l][dir], nb, D2D, s));
            HIP_TRY(hipMemcpyAsync((char *)k.bhh[l].p + dir * nb, cw->prenet_b_hh[l][dir], nb, D2D, s));
            if (scan) {
                TRY(vq_build_wfrag(cw->prenet_w_hh[l][dir], Hp, Hp / 4, Hp, 4, 3, Hp, k.frag, s));
                HIP_TRY(hipMemcpyAsync((char *)k.wf[l].p + dir * frag, k.frag.p, frag, D2D, s));
            }
            c.whh[l][dir] = cw->prenet_w_hh[l][dir];
        }
        c.wih[l] = k.wih[l].as<float>(); c.bih[l] = k.bih[l].as<float>(); c.bhh[l] = k.bhh[l].as<float>();
        c.wf[l] = scan ? k.wf[l].as<float>() : nullptr;
    }
    *out = c;
    return VQCPC_OK;
}

struct SavedView { float *series, *out0, *out1; };
SavedView saved_view(const vqcpc_vocoder *v, const void *saved, int B, int Tc) {
    const size_t rows = (size_t)B * 2 * Tc;
    float *p = (float *)const_cast<void *>(saved);
    return SavedView{p, p + rows * (v->d.dz + v->d.ds), p + rows * (v->d.dz + v->d.ds + 2 * v->d.Hp)};
}

}  // namespace

extern "C" int vqcpc_vocoder_cond_saved_bytes(vqcpc_vocoder *v, int B, int Tc, uint64_t *bytes) {
    VQ_REQUIRE(v && bytes, "vqcpc_vocoder_cond_saved_bytes: null argument");
    VQ_REQUIRE(B >= 1 && Tc >= 1, "vqcpc_vocoder_cond_saved_bytes: need B >= 1 and Tc >= 1 (got %d, %d)", B, Tc);
    *bytes = up256((uint64_t)B * 2 * Tc * (v->d.dz + v->d.ds + 4 * v->d.Hp) * sizeof(float));
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_cond_fwd(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes,
                                      const vqcpc_vocoder_cond_weights *cw, float *cond, void *saved, void *stream) {
    const char *what = "vqcpc_vocoder_cond_fwd";
    CallPlan cp;                                     // no decode loop: the layout alone sizes the staging arena
    TRY(check_call(v, what, idx, speaker, B, Tc, n_codes, cw, saved, cond, cp));
    hipStream_t s = (hipStream_t)stream;
    TRY(begin_call(v, cp, B));
    CondView view = vq_cond_view(v);
    if (cw) TRY(cond_relayout(v, cw, true, &view, s));
    const SavedView sv = saved_view(v, saved, B, Tc);
    TRY(vq_cond_run(v, cp, view, idx, speaker, B, Tc, v->gbase, sv.series, sv.out0, sv.out1, s));
    vq_cond_rows(sv.out1, cond, v->len.as<int>(), v->gbase.as<int>(), B, 2 * Tc, 2 * v->d.Hp, true, s);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_cond_bwd(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes,
                                      const vqcpc_vocoder_cond_weights *cw, const void *saved, const float *grad_cond,
                                      const vqcpc_vocoder_cond_grads *grads, void *stream) {
    const char *what = "vqcpc_vocoder_cond_bwd";
    CallPlan cp;
    TRY(check_call(v, what, idx, speaker, B, Tc, n_codes, cw, saved, grad_cond, cp));
    VQ_REQUIRE(grads, "%s: null argument", what);
    const vqcpc_vocoder_cond_grads &g = *grads;
    bool any = false;
    for (int i = 0; i < N_COND; ++i) {
        any = any || members(&g)[i];
        VQ_REQUIRE(aligned16(members(&g)[i]), "%s: the tensors of *grads must be 16-byte aligned", what);
    }
    VQ_REQUIRE(any, "%s: no wanted output (every member of *grads is NULL)", what);

    hipStream_t s = (hipStream_t)stream;
    const auto &d = v->d;
    const int Hp = d.Hp, dl = 2 * Hp, dz = d.dz, ds = d.ds, F = dz + ds, T2 = 2 * Tc, nbt = (B + 15) / 16;
    const size_t R = (size_t)cp.grows, FL = sizeof(float);
    int longest = 0;
    for (int b = 0; b < B; ++b) longest = cp.lens[b] > longest ? cp.lens[b] : longest;
    const bool want_tab = g.code_embedding || g.speaker_embedding;
    bool want_l[2] = {false, false};
    for (int l = 0; l < 2; ++l)
        for (int dir = 0; dir < 2; ++dir)
            want_l[l] = want_l[l] || g.prenet_w_ih[l][dir] || g.prenet_w_hh[l][dir] || g.prenet_b_ih[l][dir] || g.prenet_b_hh[l][dir];
    const bool run_l0 = want_l[0] || want_tab;

    // every wanted weight gradient starts from +0: the sums add to it, and a batch without a frame leaves it there
    for (int l = 0; l < 2; ++l)
        for (int dir = 0; dir < 2; ++dir) {
            const size_t I = l == 0 ? F : dl;
            if (g.prenet_w_ih[l][dir]) HIP_TRY(hipMemsetAsync(g.prenet_w_ih[l][dir], 0, (size_t)3 * Hp * I * FL, s));
            if (g.prenet_w_hh[l][dir]) HIP_TRY(hipMemsetAsync(g.prenet_w_hh[l][dir], 0, (size_t)3 * Hp * Hp * FL, s));
            if (g.prenet_b_ih[l][dir]) HIP_TRY(hipMemsetAsync(g.prenet_b_ih[l][dir], 0, (size_t)3 * Hp * FL, s));
            if (g.prenet_b_hh[l][dir]) HIP_TRY(hipMemsetAsync(g.prenet_b_hh[l][dir], 0, (size_t)3 * Hp * FL, s));
        }
    if (R == 0) {                                    // no utterance has a code: every gradient is +0
        if (g.code_embedding) HIP_TRY(hipMemsetAsync(g.code_embedding, 0, (size_t)d.n_codes * dz * FL, s));
        if (g.speaker_embedding) HIP_TRY(hipMemsetAsync(g.speaker_embedding, 0, (size_t)d.n_speakers * ds * FL, s));
        return VQCPC_OK;
    }

    CondGradWork &k = v->cg;
    TRY(v->gi.reserve(R * 6 * Hp * FL));
    TRY(k.hprev.reserve(R * dl * FL));
    TRY(k.gh.reserve(R * 6 * Hp * FL));
    TRY(k.nn.reserve(R * dl * FL));
    TRY(k.dout.reserve(R * dl * FL));
    TRY(k.dgi.reserve(R * 6 * Hp * FL));
    TRY(k.dgh.reserve(R * 6 * Hp * FL));
    TRY(k.carry.reserve(up256((size_t)2 * B * Hp * FL)));
    const size_t fragT = (size_t)(Hp / 16) * (3 * Hp / 16) * 64 * 4;             // floats of one direction's W_hh^T fragments
    TRY(k.wft.reserve(2 * fragT * FL));
    if (want_tab) {
        TRY(k.dx0.reserve(R * F * FL));
        TRY(k.keys.reserve(2 * R * sizeof(int)));
    }
    TRY(begin_call(v, cp, B));
    TRY(vq_upload_layout(v, cp, v->gbase, s));
    CondView view = vq_cond_view(v);
    if (cw) TRY(cond_relayout(v, cw, false, &view, s));
    const int *len = v->len.as<int>(), *row0 = v->gbase.as<int>();
    const SavedView sv = saved_view(v, saved, B, Tc);
    float *gi = v->gi.as<float>(), *hprev = k.hprev.as<float>(), *gh = k.gh.as<float>(), *nn = k.nn.as<float>(), *dout = k.dout.as<float>();
    float *dgi = k.dgi.as<float>(), *dgh = k.dgh.as<float>(), *wft = k.wft.as<float>();

    vq_cond_rows(grad_cond, dout, len, row0, B, T2, dl, false, s);
    for (int l = 1; l >= (run_l0 ? 0 : 1); --l) {
        const float *X = l == 0 ? sv.series : sv.out0, *Hout = l == 0 ? sv.out0 : sv.out1;
        const int I = l == 0 ? F : dl;
        hipLaunchKernelGGL(pre_hprev_kernel, dim3(B * T2, (dl + 255) / 256), dim3(256), 0, s, Hout, hprev, len, row0, T2, Hp);
        // gates again
        TRY(vq_gemm_chain(X, I, view.wih[l], view.bih[l], gi, 6 * Hp, (int)R, 6 * Hp, I, I, s));
        for (int dir = 0; dir < 2; ++dir) {
            TRY(vq_gemm_chain(hprev + dir * Hp, dl, view.whh[l][dir], view.bhh[l] + dir * 3 * Hp, gh + dir * 3 * Hp, 6 * Hp, (int)R, 3 * Hp, Hp, Hp, s));
            vq_build_wfrag_t(view.whh[l][dir], wft + dir * fragT, Hp, 3 * Hp, s);
        }
        hipLaunchKernelGGL(pre_gates_kernel, dim3((unsigned)((R * dl + 255) / 256)), dim3(256), 0, s, gi, gh, nn, R, Hp);
        // the serial part
        const PreStepP sp{(const float4 *)wft, gh, nn, hprev, dout, dgi, dgh, k.carry.as<float>(), len, row0, Hp, B, longest};
        const dim3 grid(Hp / 16, 2, nbt);
        for (int t = longest - 1; t >= 0; --t) {
            const bool built = vq_with_sw(Hp / 64, [&](auto sw) {
                hipLaunchKernelGGL((pre_bwd_step_kernel<3 * decltype(sw)::value>), grid, dim3(256), 0, s, sp, t);
            });
            if (!built) { vq_set_error("%s: dim_voc_latent / 2 = %d unsupported (64, 128, 256 and 512 are built)", what, Hp); return VQCPC_ERR_INVALID; }
        }
        // the layer's sums
        for (int dir = 0; dir < 2; ++dir) {
            const float *a_gi = dgi + dir * 3 * Hp, *a_gh = dgh + dir * 3 * Hp;
            if (g.prenet_w_ih[l][dir]) vq_grad_atb(a_gi, 6 * Hp, X, I, g.prenet_w_ih[l][dir], I, (int)R, 3 * Hp, I, s);
            if (g.prenet_w_hh[l][dir]) vq_grad_atb(a_gh, 6 * Hp, hprev + dir * Hp, dl, g.prenet_w_hh[l][dir], Hp, (int)R, 3 * Hp, Hp, s);
            if (g.prenet_b_ih[l][dir]) vq_grad_colsum(a_gi, 6 * Hp, g.prenet_b_ih[l][dir], (int)R, 3 * Hp, s);
            if (g.prenet_b_hh[l][dir]) vq_grad_colsum(a_gh, 6 * Hp, g.prenet_b_hh[l][dir], (int)R, 3 * Hp, s);
        }
        // dX: layer 0's dOut, or dseries
        if (l == 1 && run_l0) vq_grad_rows_w(dgi, view.wih[1], dl, dout, (int)R, 6 * Hp, dl, s);
        if (l == 0 && want_tab) vq_grad_rows_w(dgi, view.wih[0], F, k.dx0.as<float>(), (int)R, 6 * Hp, F, s);
    }
    if (want_tab) {
        int *keys = k.keys.as<int>();
        const float *dx0 = k.dx0.as<float>();
        hipLaunchKernelGGL(pre_keys_kernel, dim3(B * T2), dim3(64), 0, s, idx, speaker, keys, len, row0, T2, Tc, d.n_codes, d.n_speakers, R);
        if (g.code_embedding)
            hipLaunchKernelGGL(grad_atb_kernel<PreTable>, dim3((dz + 15) / 16, (d.n_codes + 63) / 64), dim3(256), 0, s,
                               PreTable{keys, dx0, F, 0, dz, g.code_embedding, d.n_codes, (int)R});
        if (g.speaker_embedding)
            hipLaunchKernelGGL(grad_atb_kernel<PreTable>, dim3((ds + 15) / 16, (d.n_speakers + 63) / 64), dim3(256), 0, s,
                               PreTable{keys + R, dx0, F, dz, ds, g.speaker_embedding, d.n_speakers, (int)R});
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
