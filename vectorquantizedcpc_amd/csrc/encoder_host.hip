// encoder_host.hip -- the encoder handle (struct vqcpc_encoder), the choice among the three schedules of its front end
// (layered kernels, one fused launch, six column-split launches: encoder.hip) and every vqcpc_encoder_* entry point.
#include "encoder_internal.h"
#include <string.h>

struct vqcpc_encoder {
    int in_channels, channels, n_emb, z_dim, c_dim;
    DevPtr<float> conv_w1, conv_w2;      // conv.weight as a GEMM operand in the k order of conv mode 1, 2
    DevPtr<float> ln_g[5], ln_b[5];
    DevPtr<float> fc_w[4];
    DevPtr<float> out_w, out_b;
    DevPtr<float> codebook, e2;
    DevPtr<float4> cbfrag;
    LstmPlan *lstm = nullptr;
    int dbg_drop = -1, dbg_timeout_ms = 1000;      // tests of the resident scan's abort path
    LnConst lnc;
    DevPtr<float> bufA, bufB, zpre;
    DevPtr<char> stats;
    DevPtr<char> adapt;                  // work space of vqcpc_encoder_vq_adapt, grown on demand: q, idx, 16-bit idx, counts
    CtxGradWork ctx;                     // work space of vqcpc_encoder_context_fwd / _bwd (context_grad.hip)
    FrontGradWork front;                 // work space of vqcpc_encoder_front_fwd / _bwd (front_grad.hip)
    DevPtr<float> conv_w;                // conv.weight as given (the layout of its gradient)
    FrontW fw{};                         // the front-end weights above as the layered schedule and the gradients read them
    int device = 0;                      // the device the handle was created on
    // fused and column-split schedules: weights in 16x16x4 fragment order (only when 4 * in_channels <= 512, the width of
    // their activation tile), and the model's half of their kernel argument
    DevPtr<float4> conv_f[2], fc_f[4], out_f;
    FusedP fp{};
    int fused = -1;                      // -1 auto (split below split_max_tiles row tiles, else fused), 0 layered kernels,
                                         // 1 one-launch fused kernel, 2 six-launch column-split kernels
    int split_max_tiles = 80;            // auto: calls of up to this many 16-row tiles take the column-split launches
    int last_schedule = -1;              // vqcpc_encoder_last_schedule: what the last front end ran (0 / 1 / 2 as `fused`), -1 none yet
    ~vqcpc_encoder() { if (lstm) vq_lstm_plan_destroy(lstm); }
};

extern "C" void vqcpc_encoder_destroy(vqcpc_encoder *e) { delete e; }

static int build_frag16(const float *W, int N, int K, DevPtr<float4> &out) {
    VQ_REQUIRE(N % 16 == 0 && K % 64 == 0, "build_frag16: unsupported shape (%d, %d)", N, K);
    TRY(out.reserve((size_t)(N / 16) * (K / 16) * 64 * sizeof(float4)));
    launch_frag16_build(W, N, K, out);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

static int encoder_create_impl(const vqcpc_encoder_weights *w, vqcpc_encoder *e) {
    const int C = w->in_channels, CH = w->channels;
    e->in_channels = C; e->channels = CH; e->n_emb = w->n_embeddings; e->z_dim = w->z_dim; e->c_dim = w->c_dim;
    HIP_TRY(hipGetDevice(&e->device));
    for (int j = 0; j < 16; ++j) e->lnc.inv[j] = 1.0f / (float)(j + 1);
    for (int q = 0; q < 8; ++q) e->lnc.sc[q] = (float)64 / (float)(64 * (q + 1));
    const size_t nconv = (size_t)CH * C * 4;
    TRY(e->conv_w1.reserve(nconv * sizeof(float)));
    TRY(e->conv_w2.reserve(nconv * sizeof(float)));
    launch_conv_weight_permute(w->conv_weight, e->conv_w1, e->conv_w2, CH, C);
    TRY(dev_copy(e->conv_w, w->conv_weight, nconv * sizeof(float), hipMemcpyDeviceToDevice));
    HIP_TRY(hipGetLastError());
    const hipMemcpyKind D2D = hipMemcpyDeviceToDevice;
    for (int i = 0; i < 5; ++i) {
        TRY(dev_copy(e->ln_g[i], w->ln_weight[i], CH * sizeof(float), D2D));
        TRY(dev_copy(e->ln_b[i], w->ln_bias[i], CH * sizeof(float), D2D));
    }
    for (int i = 0; i < 4; ++i) TRY(dev_copy(e->fc_w[i], w->fc_weight[i], (size_t)CH * CH * sizeof(float), D2D));
    TRY(dev_copy(e->out_w, w->out_weight, (size_t)w->z_dim * CH * sizeof(float), D2D));
    TRY(dev_copy(e->out_b, w->out_bias, w->z_dim * sizeof(float), D2D));
    TRY(dev_copy(e->codebook, w->codebook, (size_t)w->n_embeddings * w->z_dim * sizeof(float), D2D));
    TRY(e->e2.reserve(w->n_embeddings * sizeof(float)));
    launch_rowsumsq64(e->codebook, e->e2, w->n_embeddings);
    TRY(e->cbfrag.reserve((size_t)w->n_embeddings * 64 * sizeof(float)));
    launch_vq_build_frag(e->codebook, e->cbfrag, w->n_embeddings);
    HIP_TRY(hipGetLastError());
    TRY(vq_lstm_plan_create(w->rnn_w_ih, w->rnn_w_hh, w->rnn_b_ih, w->rnn_b_hh, w->z_dim, w->c_dim, &e->lstm));

    // fragment-ordered copies for the fused front end (the activation tile is 512 wide: 4 C <= 512)
    if (4 * C <= 512) {
        TRY(build_frag16(e->conv_w1, CH, 4 * C, e->conv_f[0]));
        TRY(build_frag16(e->conv_w2, CH, 4 * C, e->conv_f[1]));
        for (int i = 0; i < 4; ++i) TRY(build_frag16(e->fc_w[i], CH, CH, e->fc_f[i]));
        TRY(build_frag16(e->out_w, w->z_dim, CH, e->out_f));
    }
    FrontW &f = e->fw;
    f.t.conv_weight = e->conv_w; f.conv_w1 = e->conv_w1; f.conv_w2 = e->conv_w2;
    for (int i = 0; i < 5; ++i) { f.t.ln_weight[i] = e->ln_g[i]; f.t.ln_bias[i] = e->ln_b[i]; }
    for (int i = 0; i < 4; ++i) f.t.fc_weight[i] = e->fc_w[i];
    f.t.out_weight = e->out_w; f.t.out_bias = e->out_b;
    FusedP &p = e->fp;
    p.C = C;
    for (int i = 0; i < 5; ++i) { p.ln_g[i] = e->ln_g[i]; p.ln_b[i] = e->ln_b[i]; }
    for (int i = 0; i < 4; ++i) p.fc_f[i] = e->fc_f[i];
    p.out_f = e->out_f; p.out_b = e->out_b;
    p.Ef = e->cbfrag; p.E = e->codebook; p.e2 = e->e2; p.n_emb = e->n_emb;
    p.eps = 1e-5f; p.lnc = e->lnc;
    HIP_TRY(hipDeviceSynchronize());
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_create(const vqcpc_encoder_weights *w, vqcpc_encoder **out) {
    VQ_REQUIRE(w && out, "vqcpc_encoder_create: null argument");
    *out = nullptr;
    TRY(vq_require_gfx950());
    VQ_REQUIRE(w->channels == 512 && w->z_dim == 64, "encoder: channels must be 512 and z_dim 64 (got %d, %d)",
               w->channels, w->z_dim);
    VQ_REQUIRE(w->in_channels % 16 == 0 && w->in_channels > 0 && w->in_channels <= 256,
               "encoder: in_channels must be a multiple of 16 in (0, 256] (got %d)", w->in_channels);
    VQ_REQUIRE(w->n_embeddings % 64 == 0 && w->n_embeddings > 0 && w->n_embeddings <= 4096,
               "encoder: n_embeddings must be a multiple of 64 in (0, 4096] (got %d)", w->n_embeddings);
    VQ_REQUIRE(w->c_dim % 64 == 0 && w->c_dim > 0 && w->c_dim <= 1024, "encoder: c_dim must be a multiple of 64 (got %d)", w->c_dim);
    vqcpc_encoder *e = new vqcpc_encoder();
    int rc = encoder_create_impl(w, e);
    if (rc != VQCPC_OK) { vqcpc_encoder_destroy(e); return rc; }
    *out = e;
    return VQCPC_OK;
}

// Output frames of a T-frame utterance: Conv1d(k = 4, stride 2, padding 1) (model.py:43).
static int frames_of(int T) { return (T - 2) / 2 + 1; }

// VQCPC_CONV_AUTO: the order the reference's back end would pick for this call.
static int resolve_conv_mode(const vqcpc_encoder *e, int conv_mode, int B, int T) {
    if (conv_mode != VQCPC_CONV_AUTO) return conv_mode;
    return (B > 1 || (long)B * e->in_channels * T > 20480) ? VQCPC_CONV_DIRECT : VQCPC_CONV_IM2COL;
}

// The layered schedule (encoder_internal.h): conv + seg-FC stack up to `stop_stage`.  The one place that spells the sequence; the
// inference path below and the state-keeping forward of front_grad.hip differ only in `d`.
int vq_front_chain(const FrontW &w, const LnConst &lnc, const float *mel, int B, int C, int T, int conv_mode, int stop_stage,
                   const FrontDst &d, const float **stage_out, hipStream_t s) {
    const int CH = 512, To = frames_of(T), N = B * To;
    // conv (model.py:65) as an im2col GEMM in the reference back-end's summation order
    const bool one_chain = conv_mode == VQCPC_CONV_IM2COL;
    TRY(vq_gemm_chain_im2col(mel, C, T, To, one_chain ? w.conv_w1 : w.conv_w2, d.x[0], N, CH, one_chain ? 4 * C : 64, conv_mode, s));
    *stage_out = d.x[0];
    // seg-FC stack (model.py:46-55, :67): stage 1 + 2l = LN_l + ReLU, 2 + 2l = FC_l, 10 = the out layer
    for (int st = 1; st <= stop_stage; ++st) {
        const int l = (st - 1) / 2;
        if (st & 1) {
            launch_ln512(d.x[l], w.t.ln_weight[l], w.t.ln_bias[l], d.a[l], N, 1e-5f, 1, lnc, s, d.stat[l]);
            *stage_out = d.a[l];
        } else if (st < 10) {
            TRY(vq_gemm_chain(d.a[l], CH, w.t.fc_weight[l], nullptr, d.x[l + 1], CH, N, CH, CH, 256, s));
            *stage_out = d.x[l + 1];
        } else {
            TRY(vq_gemm_chain(d.a[4], CH, w.t.out_weight, w.t.out_bias, d.z_pre, 64, N, 64, CH, 256, s));
            *stage_out = d.z_pre;
            HIP_TRY(hipGetLastError());
        }
    }
    return VQCPC_OK;
}

// Inference: the chain over the handle's copies and its two ping-pong buffers, no statistics kept.
// Returns the device buffer holding the stop stage's rows in *stage_out.
static int encoder_front(vqcpc_encoder *e, const float *mel, int B, int T, int conv_mode, int stop_stage,
                         float *zp, const float **stage_out, hipStream_t s) {
    const size_t bytes = (size_t)B * frames_of(T) * e->channels * sizeof(float);
    TRY(e->bufA.reserve(bytes));
    TRY(e->bufB.reserve(bytes));
    e->last_schedule = 0;
    FrontDst d{};
    for (int l = 0; l < 5; ++l) { d.x[l] = e->bufA; d.a[l] = e->bufB; }
    d.z_pre = zp;
    return vq_front_chain(e->fw, e->lnc, mel, B, e->in_channels, T, resolve_conv_mode(e, conv_mode, B, T), stop_stage, d, stage_out, s);
}

static bool use_fused(const vqcpc_encoder *e) { return e->fused != 0 && e->conv_f[0] != nullptr; }

// The whole front end + VQ in one launch (stage < 0), or up to `stage` with that stage's rows in stage_out.
static int encoder_fused(vqcpc_encoder *e, const float *mel, int B, int T, int conv_mode, float *z_pre, float *z_q,
                         int64_t *idx, int stage, float *stage_out, hipStream_t s) {
    FusedP p = e->fp;
    p.mel = mel; p.T = T; p.To = frames_of(T); p.N = B * p.To;
    p.conv_mode = resolve_conv_mode(e, conv_mode, B, T);
    p.conv_f = e->conv_f[p.conv_mode == VQCPC_CONV_IM2COL ? 0 : 1];
    p.z_pre = z_pre; p.z_q = z_q; p.idx = idx; p.stage_out = stage_out; p.stage = stage;
    const int ntiles = (p.N + 15) / 16;
    const bool split = stage < 0 && (e->fused == 2 || (e->fused != 1 && ntiles <= e->split_max_tiles));
    e->last_schedule = split ? 2 : 1;
    if (split) {                                          // small call: six column-split launches (enc_split_*_kernel)
        TRY(e->bufA.reserve((size_t)p.N * 512 * sizeof(float)));
        TRY(e->bufB.reserve((size_t)p.N * 512 * sizeof(float)));
        launch_enc_split(p, e->bufA, e->bufB, s);
    } else {
        launch_enc_fused(p, s);
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_set_option(vqcpc_encoder *e, const char *name, int value) {
    VQ_REQUIRE(e && name, "vqcpc_encoder_set_option: null argument");
    if (!strcmp(name, "fused")) {
        VQ_REQUIRE(value >= -1 && value <= 2, "fused must be -1 (auto), 0, 1 or 2");
        VQ_REQUIRE(value < 1 || e->conv_f[0], "fused front end needs 4 * in_channels <= 512");
        e->fused = value;
        return VQCPC_OK;
    }
    if (!strcmp(name, "split_max_tiles")) {
        VQ_REQUIRE(value >= 0, "split_max_tiles must be >= 0");
        e->split_max_tiles = value;
        return VQCPC_OK;
    }
    if (!strcmp(name, "persistent_context")) return vq_lstm_set_persistent(e->lstm, value == 2 ? 2 : (value != 0 ? -1 : 0));
    if (!strcmp(name, "context_debug_drop_step")) { e->dbg_drop = value; return vq_lstm_set_debug(e->lstm, e->dbg_drop, e->dbg_timeout_ms); }
    if (!strcmp(name, "context_timeout_ms")) {
        VQ_REQUIRE(value >= 1 && value <= 10000, "context_timeout_ms must be in [1, 10000]");
        e->dbg_timeout_ms = value;
        return vq_lstm_set_debug(e->lstm, e->dbg_drop, e->dbg_timeout_ms);
    }
    vq_set_error("unknown option %s", name);
    return VQCPC_ERR_INVALID;
}

extern "C" int vqcpc_encoder_last_schedule(vqcpc_encoder *e) { return e ? e->last_schedule : -1; }

extern "C" int vqcpc_encoder_encode(vqcpc_encoder *e, const float *mel, int B, int T, int conv_mode,
                                    float *z_q, float *c, int64_t *idx, float *z_pre, void *stream) {
    VQ_REQUIRE(e && mel && z_q && idx, "vqcpc_encoder_encode: null argument");
    VQ_REQUIRE(B > 0 && T >= 2, "encoder.encode: need B > 0 and T >= 2 (got B=%d T=%d)", B, T);
    VQ_REQUIRE(conv_mode >= 0 && conv_mode <= 2, "encoder.encode: conv_mode must be 0, 1 or 2");
    hipStream_t s = (hipStream_t)stream;
    const int To = frames_of(T), N = B * To;
    float *zp = z_pre;
    if (!zp && !use_fused(e)) { TRY(e->zpre.reserve((size_t)N * 64 * sizeof(float))); zp = e->zpre; }
    VQ_REQUIRE(aligned16(zp, z_q), "encoder.encode: outputs must be 16-byte aligned");
    if (use_fused(e)) {
        TRY(encoder_fused(e, mel, B, T, conv_mode, z_pre, z_q, idx, -1, nullptr, s));     // z_pre only if asked for
    } else {
        const float *unused = nullptr;
        TRY(encoder_front(e, mel, B, T, conv_mode, 10, zp, &unused, s));
        launch_vq_encode(zp, N, e->cbfrag, e->codebook, e->e2, e->n_emb, idx, z_q, s);    // VQ (model.py:103-115)
        HIP_TRY(hipGetLastError());
    }
    if (c) TRY(vq_lstm_run(e->lstm, z_q, B, To, c, s));
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_check(vqcpc_encoder *e) {
    VQ_REQUIRE(e, "vqcpc_encoder_check: null argument");
    return vq_lstm_check(e->lstm);
}

extern "C" int vqcpc_encoder_vq_encode(vqcpc_encoder *e, const float *x, int n_rows, float *z_q, int64_t *idx,
                                       void *stream) {
    VQ_REQUIRE(e && x && z_q && idx && n_rows > 0, "vqcpc_encoder_vq_encode: bad argument");
    VQ_REQUIRE(aligned16(x, z_q), "vqcpc_encoder_vq_encode: rows must be 16-byte aligned");
    launch_vq_encode(x, n_rows, e->cbfrag, e->codebook, e->e2, e->n_emb, idx, z_q, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_stage(vqcpc_encoder *e, const float *mel, int B, int T, int conv_mode, int stage,
                                   float *out, void *stream) {
    VQ_REQUIRE(e && mel && out, "vqcpc_encoder_stage: null argument");
    VQ_REQUIRE(B > 0 && T >= 2 && stage >= 0 && stage <= 10, "vqcpc_encoder_stage: bad shape or stage");
    hipStream_t s = (hipStream_t)stream;
    if (use_fused(e))                                    // the fused kernel stops after `stage` and dumps its tile
        return encoder_fused(e, mel, B, T, conv_mode, stage == 10 ? out : nullptr, nullptr, nullptr, stage,
                             stage == 10 ? nullptr : out, s);
    const float *src = nullptr;
    float *zp = nullptr;
    if (stage == 10) {
        VQ_REQUIRE(aligned16(out), "vqcpc_encoder_stage: out must be 16-byte aligned");
        zp = out;
    }
    TRY(encoder_front(e, mel, B, T, conv_mode, stage, zp, &src, s));
    if (stage != 10)
        HIP_TRY(hipMemcpyAsync(out, src, (size_t)B * frames_of(T) * e->channels * sizeof(float), hipMemcpyDeviceToDevice, s));
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_context(vqcpc_encoder *e, const float *z, int B, int Tz, float *c, void *stream) {
    VQ_REQUIRE(e && z && c && B > 0 && Tz > 0, "vqcpc_encoder_context: bad argument");
    return vq_lstm_run(e->lstm, z, B, Tz, c, (hipStream_t)stream);
}

// The checks vqcpc_encoder_context_fwd / _bwd share; nothing is enqueued before they pass.
static int context_grad_begin(vqcpc_encoder *e, const char *what, int B, int Tz, const float *w_ih, const float *w_hh, const float *b_ih,
                              const float *b_hh, bool need_bias, LstmWeights &w, bool &own) {
    VQ_REQUIRE(B >= 1 && Tz >= 1, "%s: need B >= 1 and Tz >= 1 (got B=%d Tz=%d)", what, B, Tz);
    const int given = (w_ih != nullptr) + (w_hh != nullptr) + (need_bias ? (b_ih != nullptr) + (b_hh != nullptr) : 0);
    own = given != 0;
    VQ_REQUIRE(given == 0 || given == (need_bias ? 4 : 2), "%s: give all of the LSTM's weight tensors, or none of them (the handle's copies)", what);
    VQ_REQUIRE((long long)B * Tz <= 65535ll * 1024 && B <= 65535 * 16, "%s: B * Tz = %lld rows, more than 65535 slabs of 1024", what,
               (long long)B * Tz);
    TRY(vq_require_device(e->device, what));
    w = vq_lstm_plan_weights(e->lstm);
    if (own) { w.w_ih = w_ih; w.w_hh = w_hh; w.bias = nullptr; w.Wf = nullptr; }
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_context_saved_bytes(vqcpc_encoder *e, int B, int Tz, uint64_t *bytes) {
    VQ_REQUIRE(e && bytes, "vqcpc_encoder_context_saved_bytes: null argument");
    VQ_REQUIRE(B >= 1 && Tz >= 1, "vqcpc_encoder_context_saved_bytes: need B >= 1 and Tz >= 1 (got B=%d Tz=%d)", B, Tz);
    *bytes = (uint64_t)vq_ctx_saved_bytes(B, Tz, e->c_dim);
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_context_fwd(vqcpc_encoder *e, const float *z, int B, int Tz, const float *w_ih, const float *w_hh,
                                         const float *b_ih, const float *b_hh, float *c, void *saved, void *stream) {
    VQ_REQUIRE(e && z && c && saved, "vqcpc_encoder_context_fwd: null argument");
    LstmWeights w;
    bool own = false;
    TRY(context_grad_begin(e, "vqcpc_encoder_context_fwd", B, Tz, w_ih, w_hh, b_ih, b_hh, true, w, own));
    VQ_REQUIRE(aligned16(z, c, saved, w.w_ih, w.w_hh),
               "vqcpc_encoder_context_fwd: z, c, saved and the weights must be 16-byte aligned");
    return vq_ctx_fwd(e->ctx, w, own, b_ih, b_hh, z, B, Tz, c, (float *)saved, (hipStream_t)stream);
}

extern "C" int vqcpc_encoder_context_bwd(vqcpc_encoder *e, const float *z, int B, int Tz, const float *w_ih, const float *w_hh,
                                         const float *c, const void *saved, const float *grad_c, float *grad_z, float *grad_w_ih,
                                         float *grad_w_hh, float *grad_bias, void *stream) {
    VQ_REQUIRE(e && z && c && saved && grad_c, "vqcpc_encoder_context_bwd: null argument");
    LstmWeights w;
    bool own = false;
    TRY(context_grad_begin(e, "vqcpc_encoder_context_bwd", B, Tz, w_ih, w_hh, nullptr, nullptr, false, w, own));
    VQ_REQUIRE(aligned16(z, c, saved, grad_c, w.w_ih, w.w_hh, grad_z, grad_w_ih, grad_w_hh, grad_bias),
               "vqcpc_encoder_context_bwd: z, c, saved, the weights and the gradients must be 16-byte aligned");
    return vq_ctx_bwd(e->ctx, w, z, B, Tz, c, (const float *)saved, grad_c, grad_z, grad_w_ih, grad_w_hh, grad_bias, (hipStream_t)stream);
}

// ---- include/vqcpc.h: the front end of a training step, its backward and the VQ step's backward (front_grad.hip)
// The checks vqcpc_encoder_front_fwd / _bwd share; nothing is enqueued before they pass.
static int front_grad_begin(vqcpc_encoder *e, const char *what, const float *mel, int B, int T, int conv_mode,
                            const vqcpc_encoder_front_weights *w, FrontW &fw) {
    VQ_REQUIRE(e && mel, "%s: null argument", what);
    VQ_REQUIRE(B >= 1 && T >= 2, "%s: need B >= 1 and T >= 2 (got B=%d T=%d)", what, B, T);
    VQ_REQUIRE(conv_mode >= 0 && conv_mode <= 2, "%s: conv_mode must be 0, 1 or 2", what);
    VQ_REQUIRE((long long)B * frames_of(T) <= (1ll << 22), "%s: B * (T / 2) = %lld rows, more than 2^22", what, (long long)B * frames_of(T));
    VQ_REQUIRE((long long)B * e->in_channels * T < (1ll << 31), "%s: mel of %lld elements, 2^31 or more", what, (long long)B * e->in_channels * T);
    TRY(vq_require_device(e->device, what));
    bool ok = aligned16(mel);
    if (w) {
        fw = FrontW{*w, nullptr, nullptr};
        bool all = true;
        for (const float *p : front_slots(*w)) { all = all && p; ok = ok && aligned16(p); }
        VQ_REQUIRE(all, "%s: a weights struct must give every front-end tensor (NULL struct = the handle's copies)", what);
    } else {
        fw = e->fw;
    }
    VQ_REQUIRE(ok, "%s: mel and the weights must be 16-byte aligned", what);
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_front_saved_bytes(vqcpc_encoder *e, int B, int T, uint64_t *bytes) {
    VQ_REQUIRE(e && bytes, "vqcpc_encoder_front_saved_bytes: null argument");
    VQ_REQUIRE(B >= 1 && T >= 2, "vqcpc_encoder_front_saved_bytes: need B >= 1 and T >= 2 (got B=%d T=%d)", B, T);
    *bytes = (uint64_t)vq_front_saved_bytes(B, frames_of(T));
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_front_fwd(vqcpc_encoder *e, const float *mel, int B, int T, int conv_mode,
                                       const vqcpc_encoder_front_weights *w, float *z_pre, void *saved, void *stream) {
    VQ_REQUIRE(z_pre && saved, "vqcpc_encoder_front_fwd: null argument");
    FrontW fw;
    TRY(front_grad_begin(e, "vqcpc_encoder_front_fwd", mel, B, T, conv_mode, w, fw));
    VQ_REQUIRE(aligned16(z_pre, saved), "vqcpc_encoder_front_fwd: z_pre and saved must be 16-byte aligned");
    return vq_front_fwd(e->front, fw, e->lnc, mel, B, e->in_channels, T, resolve_conv_mode(e, conv_mode, B, T), z_pre, (float *)saved,
                        (hipStream_t)stream);
}

extern "C" int vqcpc_encoder_front_bwd(vqcpc_encoder *e, const float *mel, int B, int T, int conv_mode,
                                       const vqcpc_encoder_front_weights *w, const void *saved, const float *grad_z_pre,
                                       const vqcpc_encoder_front_grads *grads, void *stream) {
    VQ_REQUIRE(saved && grad_z_pre && grads, "vqcpc_encoder_front_bwd: null argument");
    FrontW fw;
    TRY(front_grad_begin(e, "vqcpc_encoder_front_bwd", mel, B, T, conv_mode, w, fw));
    bool any = false, ok = aligned16(saved, grad_z_pre);
    for (float *p : front_slots(*grads)) { any = any || p; ok = ok && aligned16(p); }
    VQ_REQUIRE(any, "vqcpc_encoder_front_bwd: no gradient asked for");
    VQ_REQUIRE(ok, "vqcpc_encoder_front_bwd: saved, grad_z_pre and the gradients must be 16-byte aligned");
    return vq_front_bwd(e->front, fw, mel, B, e->in_channels, T, (const float *)saved, grad_z_pre, *grads, (hipStream_t)stream);
}

extern "C" int vqcpc_encoder_vq_bwd(vqcpc_encoder *e, const float *z_pre, const float *z_q, int n_rows, const float *grad_z_st,
                                    const float *grad_loss, float *grad_z_pre, void *stream) {
    VQ_REQUIRE(e && z_pre && z_q && grad_z_pre, "vqcpc_encoder_vq_bwd: null argument");
    VQ_REQUIRE(grad_z_st || grad_loss, "vqcpc_encoder_vq_bwd: give grad_z_st, grad_loss or both");
    VQ_REQUIRE(n_rows >= 1, "vqcpc_encoder_vq_bwd: n_rows must be at least 1 (got %d)", n_rows);
    VQ_REQUIRE(aligned16(z_pre, z_q, grad_z_pre, grad_z_st),
               "vqcpc_encoder_vq_bwd: the rows must be 16-byte aligned");
    TRY(vq_require_device(e->device, "vqcpc_encoder_vq_bwd"));
    const float scale = (float)(0.5 / ((double)n_rows * (double)e->z_dim));
    launch_vq_bwd(z_pre, z_q, (size_t)n_rows * e->z_dim, scale, grad_z_st, grad_loss, grad_z_pre, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_forward_stats(vqcpc_encoder *e, const float *z_pre, const float *z_q,
                                           const int64_t *idx, int n_rows, float *z_st, float *loss,
                                           float *perplexity, void *stream) {
    VQ_REQUIRE(e && z_pre && z_q && idx && loss && perplexity && n_rows > 0, "vqcpc_encoder_forward_stats: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int nblk = 64;
    const size_t hist_bytes = (size_t)e->n_emb * sizeof(unsigned);
    TRY(e->stats.reserve(hist_bytes + nblk * sizeof(double) + 64));
    unsigned *hist = e->stats.as<unsigned>();
    double *part = (double *)(e->stats + ((hist_bytes + 15) / 16) * 16);
    HIP_TRY(hipMemsetAsync(hist, 0, hist_bytes, s));
    launch_vq_stats(z_pre, z_q, idx, n_rows, z_st, part, nblk, hist, e->n_emb, loss, perplexity, s);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

// Bytes of the adapt work space for n_rows rows: quantised rows, int64 indices (when the caller keeps none), 16-bit indices,
// counts -- each part 16-byte aligned.
static size_t adapt_offsets(int n_rows, int n_emb, size_t (&off)[4]) {
    const size_t sz[4] = {(size_t)n_rows * 64 * sizeof(float), (size_t)n_rows * sizeof(int64_t), (size_t)n_rows * sizeof(uint16_t),
                          (size_t)n_emb * sizeof(float)};
    size_t at = 0;
    for (int i = 0; i < 4; ++i) { off[i] = at; at += (sz[i] + 15) / 16 * 16; }
    return at;
}

extern "C" int vqcpc_encoder_vq_adapt(vqcpc_encoder *e, const float *x, int n_rows, double decay, double epsilon,
                                      float *embedding, float *ema_count, float *ema_weight,
                                      float *z_st, int64_t *idx, float *loss, float *perplexity, void *stream) {
    VQ_REQUIRE(e && x && embedding && ema_count && ema_weight && loss && perplexity, "vqcpc_encoder_vq_adapt: null argument");
    VQ_REQUIRE(n_rows >= 1 && n_rows <= (1 << 24), "vqcpc_encoder_vq_adapt: n_rows must be in [1, 2^24] (got %d)", n_rows);
    VQ_REQUIRE(decay > 0.0 && decay < 1.0, "vqcpc_encoder_vq_adapt: decay must be in (0, 1) (got %g)", decay);
    VQ_REQUIRE(epsilon > 0.0, "vqcpc_encoder_vq_adapt: epsilon must be > 0 (got %g)", epsilon);
    VQ_REQUIRE(aligned16(x), "vqcpc_encoder_vq_adapt: rows must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    size_t off[4];
    TRY(e->adapt.reserve(adapt_offsets(n_rows, e->n_emb, off)));
    float *q = (float *)(e->adapt + off[0]);
    int64_t *ix = idx ? idx : (int64_t *)(e->adapt + off[1]);
    uint16_t *idx16 = (uint16_t *)(e->adapt + off[2]);
    float *cnt = (float *)(e->adapt + off[3]);

    // the eval forward from the OLD codebook (model.py:126-134, :147-153); its integer histogram stays in e->stats
    launch_vq_encode(x, n_rows, e->cbfrag, e->codebook, e->e2, e->n_emb, ix, q, s);
    HIP_TRY(hipGetLastError());
    TRY(vqcpc_encoder_forward_stats(e, x, q, ix, n_rows, z_st, loss, perplexity, stream));

    // the update (model.py:136-145)
    EmaP p{};
    p.x = x; p.idx16 = idx16; p.n_rows = n_rows; p.cnt = cnt; p.n_emb = e->n_emb;
    p.decay = (float)decay; p.omd = (float)(1.0 - decay);              // 1 - decay in double, as Python forms it
    p.eps = (float)epsilon; p.meps = (float)((double)e->n_emb * epsilon);
    p.ema_count = ema_count; p.ema_weight = ema_weight; p.embedding = embedding; p.codebook = e->codebook;
    launch_ema_prep(ix, n_rows, e->stats.as<unsigned>(), ema_count, e->n_emb, p.decay, p.omd, idx16, cnt, s);
    launch_ema_update(p, s);
    // the handle follows: |e|^2 and the search fragments as create builds them
    launch_rowsumsq64(e->codebook, e->e2, e->n_emb, s);
    launch_vq_build_frag(e->codebook, e->cbfrag, e->n_emb, s);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_encoder_workspace_bytes(vqcpc_encoder *e, uint64_t *bytes) {
    VQ_REQUIRE(e && bytes, "vqcpc_encoder_workspace_bytes: null argument");
    *bytes = (uint64_t)(e->bufA.cap + e->bufB.cap + e->zpre.cap + e->stats.cap + e->adapt.cap + e->ctx.bytes() + e->front.bytes());
    return VQCPC_OK;
}
