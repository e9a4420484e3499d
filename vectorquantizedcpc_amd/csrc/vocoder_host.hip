// vocoder_host.hip -- the vocoder handle (vqcpc_vocoder_*): create / destroy, options and the status-word policy, the conditioning
// (glue -> bi-GRU prenet in scan.hip -> Gcond rows), and the dispatch of a planned call (vocoder_plan.hip) onto the per-XCD
// resident decoders (ar_xcd.hip / ar_xcm.hip) or the launch-per-step kernels (vocoder.hip, through ar_step.h).
#include "vocoder_internal.h"
#include <math.h>
#include <stdio.h>
#include <limits.h>


// [rows][3][H] -> unit quads [rows][H/4][4] float4 (r, z, n, 0)
__global__ void quads_build_kernel(const float *__restrict__ src, float4 *__restrict__ dst, int rows, int H) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)rows * H) return;
    const int unit = (int)(id % H);
    const size_t row = id / H;
    const float *s = src + row * 3 * H + unit;
    dst[row * H + unit] = make_float4(s[0], s[H], s[2 * H], 0.f);
}

// Vocoder glue (network_vocoder.py:73-77): series[b, t2, :dz] = code_emb[idx[b, t2/2]], [dz:] = spk_emb[spk[b]]
// An index outside its table (nn.Embedding raises IndexError, network_vocoder.py:73,75) is clamped for the read and reported through
// the handle's host-mapped status word (STATUS_BAD_INDEX; vqcpc_vocoder_check): no read-back of the indices on the host, no synchronisation.
__global__ void glue_kernel(const int64_t *__restrict__ idx, const int64_t *__restrict__ spk,
                            const float *__restrict__ ce, const float *__restrict__ se, float *__restrict__ out,
                            int B, int Tc, int dz, int ds, int n_codes, int n_spk, unsigned *status, unsigned status_tag,
                            const int *__restrict__ frames, const int *__restrict__ row0) {
    const int F = dz + ds;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * 2 * Tc * F) return;
    const int f = (int)(i % F);
    const size_t r = i / F;
    const int t2 = (int)(r % (2 * Tc)), b = (int)(r / (2 * Tc));
    if (row0) {                                         // ragged rows: an utterance's own frames only, at its row base
        if (t2 >= frames[b]) return;
        i = ((size_t)row0[b] + t2) * F + f;
    }
    if (f < dz) {
        long long z = idx[(size_t)b * Tc + t2 / 2];
        if ((z < 0 || z >= n_codes) && f == 0 && status) __hip_atomic_fetch_or(status, status_tag | STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        z = z < 0 ? 0 : (z >= n_codes ? n_codes - 1 : z);
        out[i] = ce[(size_t)z * dz + f];
    } else {
        long long sp = spk[b];
        if ((sp < 0 || sp >= n_spk) && f == dz && t2 == 0 && status) __hip_atomic_fetch_or(status, status_tag | STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        sp = sp < 0 ? 0 : (sp >= n_spk ? n_spk - 1 : sp);
        out[i] = se[(size_t)sp * ds + (f - dz)];
    }
}

__global__ void copy_submatrix_kernel(const float *__restrict__ src, int ld, int col0, float *__restrict__ dst,
                                      int rows, int cols) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * cols) return;
    const int r = (int)(i / cols), cidx = (int)(i % cols);
    dst[i] = src[(size_t)r * ld + col0 + cidx];
}
static ArStep step_of(vqcpc_vocoder *v) { return ArStep{v->d.Hr, v->d.Hf, v->d.n_cls, v->big_min_tiles, &v->big_attr_set}; }

static void clear_graphs(vqcpc_vocoder::Group &G) {
    for (auto &kv : G.graphs) (void)hipGraphExecDestroy(kv.second);
    G.graphs.clear();
}
static void clear_graphs(vqcpc_vocoder *v) {
    for (auto &G : v->grp) clear_graphs(G);
}

// The grow-only work buffers, which vqcpc_vocoder_workspace_bytes sums (the weights and call records made at create are not
// counted).  Nothing is freed through this list: every buffer is an owning member.
static std::vector<const DevBuf *> work_buffers(const vqcpc_vocoder *v) {
    std::vector<const DevBuf *> b = {&v->series, &v->gi, &v->out0, &v->cond, &v->gcond, &v->gbase, &v->hseq, &v->len, &v->hall, &v->a1c, &v->nll_part,
                                     &v->nll_len, &v->xd_x, &v->xd_segs};
    for (auto &G : v->grp) b.insert(b.end(), {&G.har, &G.a1, &G.cand_s, &G.cand_k, &G.slot_tab, &G.cur, &G.gcur, &G.candg});
    for (const DevBuf *g : v->gw.all()) b.push_back(g);
    for (const DevBuf *g : v->cg.all()) b.push_back(g);
    return b;
}

// The members free their memory; what is not memory goes here, before they die.
vqcpc_vocoder::~vqcpc_vocoder() {
    clear_graphs(this);
    stage.drain();
    for (hipStream_t st : {side_stream, cap_stream}) if (st) (void)hipStreamDestroy(st);
    for (hipEvent_t e : {ev_fork, ev_join, ev0, ev1}) if (e) (void)hipEventDestroy(e);
}

extern "C" void vqcpc_vocoder_destroy(vqcpc_vocoder *v) { delete v; }

static int vocoder_create_impl(const vqcpc_vocoder_weights *w, vqcpc_vocoder *v) {
    v->d = *w;
    HIP_TRY(hipGetDevice(&v->device));
    const int F = w->dz + w->ds, Hp = w->Hp, dl = 2 * Hp, Hr = w->Hr, de = w->de;
    const hipMemcpyKind D2D = hipMemcpyDeviceToDevice;
    DevPtr<float> &w_emb = v->w_emb, &emb = v->ar_emb;     // the Gemb table's two factors (kept: its gradients need them)
    TRY(dev_copy(v->code_emb, w->code_embedding, (size_t)w->n_codes * w->dz * sizeof(float), D2D));
    TRY(dev_copy(v->spk_emb, w->speaker_embedding, (size_t)w->n_speakers * w->ds * sizeof(float), D2D));
    for (int l = 0; l < 2; ++l) {
        const int I = l == 0 ? F : dl;
        TRY(v->p_wih[l].reserve((size_t)6 * Hp * I * sizeof(float)));
        TRY(v->p_bih[l].reserve((size_t)6 * Hp * sizeof(float)));
        TRY(v->p_bhh[l].reserve((size_t)6 * Hp * sizeof(float)));
        TRY(v->p_wf[l].reserve((size_t)2 * (Hp / 4) * (Hp / 16) * 64 * sizeof(float4)));
        TRY(v->p_whh[l].reserve((size_t)6 * Hp * Hp * sizeof(float)));
        for (int d = 0; d < 2; ++d) {
            HIP_TRY(hipMemcpy(v->p_wih[l] + (size_t)d * 3 * Hp * I, w->prenet_w_ih[l][d], (size_t)3 * Hp * I * sizeof(float), D2D));
            HIP_TRY(hipMemcpy(v->p_bih[l] + (size_t)d * 3 * Hp, w->prenet_b_ih[l][d], (size_t)3 * Hp * sizeof(float), D2D));
            HIP_TRY(hipMemcpy(v->p_bhh[l] + (size_t)d * 3 * Hp, w->prenet_b_hh[l][d], (size_t)3 * Hp * sizeof(float), D2D));
            HIP_TRY(hipMemcpy(v->p_whh[l] + (size_t)d * 3 * Hp * Hp, w->prenet_w_hh[l][d], (size_t)3 * Hp * Hp * sizeof(float), D2D));
            DevBuf frag;                 // one direction's W_hh in fragment order
            TRY(vq_build_wfrag(w->prenet_w_hh[l][d], Hp, Hp / 4, Hp, 4, 3, Hp, frag));
            HIP_TRY(hipMemcpy((char *)v->p_wf[l].p + d * frag.cap, frag.p, frag.cap, D2D));
        }
    }
    // AR input weights split: [:, :de] feeds the sample embedding (-> lookup table Gemb), [:, de:] the conditioning
    TRY(w_emb.reserve((size_t)3 * Hr * de * sizeof(float)));
    TRY(v->w_cond.reserve((size_t)3 * Hr * dl * sizeof(float)));
    hipLaunchKernelGGL(copy_submatrix_kernel, dim3((unsigned)(((size_t)3 * Hr * de + 255) / 256)), dim3(256), 0, 0,
                       w->ar_w_ih, de + dl, 0, w_emb.as<float>(), 3 * Hr, de);
    hipLaunchKernelGGL(copy_submatrix_kernel, dim3((unsigned)(((size_t)3 * Hr * dl + 255) / 256)), dim3(256), 0, 0,
                       w->ar_w_ih, de + dl, de, v->w_cond.as<float>(), 3 * Hr, dl);
    HIP_TRY(hipGetLastError());
    TRY(dev_copy(v->b_ih, w->ar_b_ih, (size_t)3 * Hr * sizeof(float), D2D));
    TRY(dev_copy(v->b_hh, w->ar_b_hh, (size_t)3 * Hr * sizeof(float), D2D));
    TRY(v->Gemb.reserve((size_t)w->n_cls * 3 * Hr * sizeof(float)));
    TRY(dev_copy(emb, w->ar_embedding, (size_t)w->n_cls * de * sizeof(float), D2D));
    TRY(vq_gemm_chain(emb.as<float>(), de, w_emb.as<float>(), nullptr, v->Gemb, 3 * Hr, w->n_cls, 3 * Hr, de, de, 0));
    TRY(v->Gemb4.reserve((size_t)w->n_cls * Hr * sizeof(float4)));
    TRY(v->bh4.reserve((size_t)Hr * sizeof(float4)));
    hipLaunchKernelGGL(quads_build_kernel, dim3((unsigned)(((size_t)w->n_cls * Hr + 255) / 256)), dim3(256), 0, 0, v->Gemb.as<float>(), v->Gemb4.as<float4>(), w->n_cls, Hr);
    hipLaunchKernelGGL(quads_build_kernel, dim3((unsigned)((Hr + 255) / 256)), dim3(256), 0, 0, v->b_hh.as<float>(), v->bh4.as<float4>(), 1, Hr);
    HIP_TRY(hipGetLastError());
    TRY(build_wfrag12(w->ar_w_hh, Hr, Hr / 4, Hr, Hr, v->Wf_hh12));
    if (Hr % 16 == 0) TRY(vq_build_wfrag(w->ar_w_hh, Hr, 3 * (Hr / 16), Hr, 4, 16, Hr, v->Wf_hh16));
    TRY(vq_build_wfrag(w->fc1_weight, Hr, w->Hf / 16, Hr, 4, 0, 0, v->Wf_fc1));
    TRY(vq_build_wfrag(w->fc1_weight, Hr, w->Hf / 8, Hr, 4, 8, 0, v->Wf_fc1h));
    TRY(vq_build_wfrag(w->fc2_weight, w->Hf, w->n_cls / 16, w->Hf, 1, 0, 0, v->Wf_fc2));
    TRY(dev_copy(v->w_hh, w->ar_w_hh, (size_t)3 * Hr * Hr * sizeof(float), D2D));
    TRY(dev_copy(v->w_fc1, w->fc1_weight, (size_t)w->Hf * Hr * sizeof(float), D2D));
    TRY(dev_copy(v->w_fc2, w->fc2_weight, (size_t)w->n_cls * w->Hf * sizeof(float), D2D));
    TRY(dev_copy(v->b_fc1, w->fc1_bias, w->Hf * sizeof(float), D2D));
    TRY(dev_copy(v->b_fc2, w->fc2_bias, w->n_cls * sizeof(float), D2D));
    // mu-law decode table (preprocess.py:30-35, evaluated in float64 like the reference's numpy)
    std::vector<float> tab(w->n_cls);
    const double mu = (double)((1 << w->bits_mu_law) - 1);
    for (int s = 0; s < w->n_cls; ++s) {
        const double y = 2.0 * (double)s / mu - 1.0, sg = (y > 0) - (y < 0);
        tab[s] = (float)(sg / mu * (pow(1.0 + mu, fabs(y)) - 1.0));
    }
    TRY(dev_copy(v->mulaw_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    for (auto &g : v->grp) TRY(g.call.reserve(sizeof(ArCall)));
    if (w->Hf == NLL_HF && w->n_cls == NLL_CLS) TRY(vq_tf_nll_prepare());      // the scoring head's LDS attribute, once per handle
    TRY(v->status.create());
    HIP_TRY(hipStreamCreateWithFlags(&v->side_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&v->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&v->ev_join, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&v->cap_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&v->ev0));
    HIP_TRY(hipEventCreate(&v->ev1));
    HIP_TRY(hipDeviceSynchronize());
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_create(const vqcpc_vocoder_weights *w, vqcpc_vocoder **out) {
    VQ_REQUIRE(w && out, "vqcpc_vocoder_create: null argument");
    *out = nullptr;
    TRY(vq_require_gfx950());
    VQ_REQUIRE(w->bits_mu_law >= 8 && w->bits_mu_law <= 10 && w->n_cls == (1 << w->bits_mu_law),
               "vocoder: bits_mu_law must be 8 (config.py:15), 9 or 10 with n_cls = 2^bits (got %d, %d)", w->bits_mu_law, w->n_cls);
    VQ_REQUIRE(w->Hf >= 256 && w->Hf <= 1024 && w->Hf % 256 == 0, "vocoder: size_h_fc must be 256 (config.py:77), 512, 768 or 1024 (got %d)", w->Hf);
    VQ_REQUIRE((w->dz + w->ds) % 32 == 0 && w->Hp % 64 == 0 && w->Hp <= 1024, "vocoder: dz+ds %% 32 and Hp %% 64 required");
    VQ_REQUIRE(w->de % 32 == 0, "vocoder: size_i_embed_ar %% 32 required (got %d)", w->de);
    VQ_REQUIRE(w->Hr == 512 || w->Hr == 896 || w->Hr == 1024, "vocoder: size_h_rnn %d: the per-sample kernels are built for 512, 896 "
               "(config.py:76) and 1024", w->Hr);
    VQ_REQUIRE(w->Hp == 64 || w->Hp == 128 || w->Hp == 256 || w->Hp == 512, "vocoder: dim_voc_latent / 2 = %d: the prenet scan is built "
               "for 64, 128 (config.py:68), 256 and 512", w->Hp);
    VQ_REQUIRE(w->upsample_t > 0, "vocoder: upsample_t must be positive");
    vqcpc_vocoder *v = new vqcpc_vocoder();
    int rc = vocoder_create_impl(w, v);
    if (rc != VQCPC_OK) { vqcpc_vocoder_destroy(v); return rc; }
    *out = v;
    return VQCPC_OK;
}

// set_option: name, member, accepted range, and flags -- OPT_BOOL stores value != 0 (any value is accepted), OPT_GRAPHS drops the
// captured graphs when the value changes (they bake it), OPT_EVEN takes even values only.
enum { OPT_BOOL = 1, OPT_GRAPHS = 2, OPT_EVEN = 4 };
struct OptSpec { const char *name; int vqcpc_vocoder::*field; int lo, hi, flags; };
static const OptSpec k_options[] = {
    {"use_graph", &vqcpc_vocoder::use_graph, 0, 1, OPT_BOOL},
    {"steps_per_graph", &vqcpc_vocoder::steps_per_graph, 2, 4096, OPT_GRAPHS | OPT_EVEN},
    {"big_min_tiles", &vqcpc_vocoder::big_min_tiles, 0, INT_MAX, OPT_GRAPHS},
    {"two_groups", &vqcpc_vocoder::two_groups, 0, 1, OPT_BOOL},
    {"fuse_fc2", &vqcpc_vocoder::fuse_fc2, 0, 1, OPT_BOOL | OPT_GRAPHS},
    {"handoff_timeout_ms", &vqcpc_vocoder::handoff_timeout_ms, 1, 10000, OPT_GRAPHS},
    {"handoff_debug_drop_step", &vqcpc_vocoder::handoff_debug_drop_step, INT_MIN, INT_MAX, OPT_GRAPHS},
    {"xcd", &vqcpc_vocoder::xcd, -1, 1, 0},
    {"xcd_slots", &vqcpc_vocoder::xcd_slots, 1, 8 * XD_MAX_BX, 0},
    {"xcd_agent_stores", &vqcpc_vocoder::xcd_agent_stores, 0, 1, OPT_BOOL},
    {"xcm", &vqcpc_vocoder::xcm, -1, 1, 0},
    {"xcm_min", &vqcpc_vocoder::xcm_min, 0, 65536, 0},
    {"xcm_max", &vqcpc_vocoder::xcm_max, 0, 1 << 20, 0},
    {"xcm_slots", &vqcpc_vocoder::xcm_slots, 1, 8 * XM_BX, 0},
    {"xcd_timeout_ms", &vqcpc_vocoder::xcd_timeout_ms, 1, 10000, 0},
    {"xcd_debug_drop_step", &vqcpc_vocoder::xcd_debug_drop_step, INT_MIN, INT_MAX, 0},
    {"xcd_debug_misplace", &vqcpc_vocoder::xcd_debug_misplace, 0, 1, OPT_BOOL},
    {"tf_chunk_replays", &vqcpc_vocoder::tf_chunk_replays, 1, 64, 0},
    {"slots", &vqcpc_vocoder::n_slots, 0, 65536, 0},
};

extern "C" int vqcpc_vocoder_set_option(vqcpc_vocoder *v, const char *name, int value) {
    VQ_REQUIRE(v && name, "vqcpc_vocoder_set_option: null argument");
    for (const OptSpec &o : k_options) {
        if (strcmp(name, o.name)) continue;
        if (o.flags & OPT_BOOL) value = value != 0;
        VQ_REQUIRE(value >= o.lo && value <= o.hi && !((o.flags & OPT_EVEN) && value % 2), "%s must be %sin [%d, %d]", name,
                   (o.flags & OPT_EVEN) ? "even and " : "", o.lo, o.hi);
        if ((o.flags & OPT_GRAPHS) && value != v->*o.field) clear_graphs(v);
        v->*o.field = value;
        if (o.field == &vqcpc_vocoder::xcd) { v->fell_back = false; v->placement_misses = 0; }   // a choice of its own re-arms the fallback
        return VQCPC_OK;
    }
    vq_set_error("unknown option %s", name);
    return VQCPC_ERR_INVALID;
}

// Did an in-kernel hand-off of an earlier call give up?  The status word is host-mapped (no HIP call).  `synced`: the caller has
// synchronised the stream that carried the calls (vqcpc_vocoder_check's contract), so a zero word clears every call in flight;
// without it (the start of the next call) only a word that is already set is acted on -- nothing is cleared before a sync.
constexpr int REARM_CLEAN = 16;
static void fall_back(vqcpc_vocoder *v) {          // resident decoders off; what to re-arm is saved at the first fall-back
    if (!v->fell_back) { v->saved_xcd = v->xcd; v->saved_fuse_fc2 = v->fuse_fc2; }
    v->fell_back = true; v->clean_calls = 0; v->xcd = 0;
}
static int status_check(vqcpc_vocoder *v, bool synced) {
    if (!v->status_pending) return VQCPC_OK;
    const unsigned flag = *(volatile unsigned *)v->status.host;        // written by the kernel; no HIP call
    if (flag == 0) {
        if (synced) {
            v->status_pending = false;
            v->placement_misses = 0;
            if (v->fell_back && ++v->clean_calls >= REARM_CLEAN) {     // re-arm: the cause (a co-tenant kernel, a hung peer) is probably gone
                v->fell_back = false;
                v->xcd = v->saved_xcd;
                if (v->saved_fuse_fc2 && !v->fuse_fc2) { v->fuse_fc2 = 1; clear_graphs(v); }
            }
        }
        return VQCPC_OK;
    }
    *(volatile unsigned *)v->status.host = 0u;
    v->status_pending = false;
    const unsigned code = flag & 0xffu, ep = flag >> 8;
    char which[64];
    if (ep) snprintf(which, sizeof which, "call #%u of this handle", ep);
    else snprintf(which, sizeof which, "an earlier call of this handle");
    if (code & STATUS_BAD_INDEX) {
        vq_set_error("index out of range in self (%s): a code index or speaker id outside its embedding table (network_vocoder.py:73,75), "
                     "or a sample class outside [0, n_cls) in a scored position of vqcpc_vocoder_nll", which);
        return VQCPC_ERR_INVALID;
    }
    if (code & STATUS_MISPLACED) {
        v->placement_misses += 1;
        if (v->placement_misses >= 2) {
            fall_back(v);
            vq_set_error("decode not run (%s): the resident decoders' workgroups were not dealt 32 to each XCD, twice in a row (no output was "
                         "written; the GPU is probably shared) -- this handle now uses one launch per kernel and step; repeat the call", which);
        } else {
            vq_set_error("decode not run (%s): the resident decoders' workgroups were not dealt 32 to each XCD (no output was written; "
                         "another kernel held compute units) -- repeat the call", which);
        }
        return VQCPC_ERR_HIP;
    }
    fall_back(v);
    if (code & STATUS_RANGE) {         // as a timeout, but the launch path's own hand-offs are not in doubt: the fused fc2 launch stays
        vq_set_error("decode aborted (%s): a non-finite or out-of-range hidden state (NaN, inf or |h| >= 2 -- from the weights, the conditioning "
                     "or a resumed state) cannot travel in the resident decoders' exchange words (outputs of that call are incomplete); this handle "
                     "now uses one launch per kernel and step, and re-arms after %d clean calls or set_option xcd -- repeat the call",
                     which, REARM_CLEAN);
        return VQCPC_ERR_HIP;
    }
    if (v->fuse_fc2) { v->fuse_fc2 = 0; clear_graphs(v); }
    vq_set_error("decode aborted (%s): an in-kernel exchange timed out (outputs of that call are incomplete); this handle now uses one launch "
                 "per kernel and step, and re-arms after %d clean calls or set_option xcd / fuse_fc2 -- repeat the call", which, REARM_CLEAN);
    return VQCPC_ERR_HIP;
}

extern "C" int vqcpc_vocoder_last_path(vqcpc_vocoder *v) {
    return v ? v->last_path : -1;
}

extern "C" int vqcpc_vocoder_check(vqcpc_vocoder *v) {
    VQ_REQUIRE(v, "vqcpc_vocoder_check: null argument");
    return status_check(v, true);
}

extern "C" int vqcpc_vocoder_last_slots(vqcpc_vocoder *v) {
    return v ? v->last_slots : -1;
}

extern "C" int vqcpc_vocoder_workspace_bytes(vqcpc_vocoder *v, uint64_t *bytes) {
    VQ_REQUIRE(v && bytes, "vqcpc_vocoder_workspace_bytes: null argument");
    uint64_t n = 0;
    for (const DevBuf *b : work_buffers(v)) n += b->cap;
    *bytes = n;
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_last_timing(vqcpc_vocoder *v, float *loop_ms, int *n_steps) {
    VQ_REQUIRE(v && loop_ms && n_steps, "vqcpc_vocoder_last_timing: null argument");
    TRY(status_check(v, true));
    HIP_TRY(hipEventElapsedTime(loop_ms, v->ev0, v->ev1));
    *n_steps = v->last_steps;
    return VQCPC_OK;
}

// conditioning: glue -> 2-layer bi-GRU prenet -> cond.  Dense (frames_dev == row0_dev == nullptr): cond (B, 2Tc, 2Hp), every
// utterance 2 Tc frames.  Ragged: frames_dev[b] valid frames per utterance, row0_dev[b] its first row, n_rows = their sum -- every
// buffer of the prenet (series, hoisted gate inputs, both layers' outputs) holds the utterances' OWN frames only, utterance b at
// rows row0[b] ..: on a manifest of 1 - 10 s utterances (mean 3.4 s) two thirds of B x T_max would be padding.
// cv: the weights it reads; series_out, out0_out: where the glued series and layer 0's output go, null = the handle's work space.
static int run_condition(vqcpc_vocoder *v, const CondView &cv, const int64_t *idx, const int64_t *spk, int B, int Tc,
                         const int *frames_dev, const int *row0_dev, size_t n_rows, float *series_out, float *out0_out, float *cond_out,
                         hipStream_t s) {
    const auto &d = v->d;
    const int F = d.dz + d.ds, Hp = d.Hp, dl = 2 * Hp, T2 = 2 * Tc, nbt = (B + 15) / 16;
    const size_t rows = row0_dev ? (n_rows ? n_rows : 1) : (size_t)B * T2;
    if (!series_out) { TRY(v->series.reserve(rows * F * sizeof(float))); series_out = v->series.as<float>(); }
    TRY(v->gi.reserve(rows * 6 * Hp * sizeof(float)));
    if (!out0_out) { TRY(v->out0.reserve(rows * dl * sizeof(float))); out0_out = v->out0.as<float>(); }
    const size_t hsz = (size_t)2 * nbt * Hp * 16 * sizeof(float);
    TRY(v->hseq.reserve(2 * hsz));
    const size_t ng = (size_t)B * T2 * F;
    hipLaunchKernelGGL(glue_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, idx, spk, cv.code_emb,
                       cv.spk_emb, series_out, B, Tc, d.dz, d.ds, d.n_codes, d.n_speakers, v->status.dev, v->epoch << 8,
                       frames_dev, row0_dev);
    v->status_pending = true;            // an index outside its table is reported through the status word
    for (int l = 0; l < 2; ++l) {
        const float *xin = l == 0 ? series_out : out0_out;
        const int I = l == 0 ? F : dl;
        float *xout = l == 0 ? out0_out : cond_out;
        TRY(vq_gemm_chain(xin, I, cv.wih[l], cv.bih[l], v->gi.as<float>(), 6 * Hp, (int)rows, 6 * Hp, I, I, s));
        if (frames_dev && !row0_dev) HIP_TRY(hipMemsetAsync(xout, 0, rows * dl * sizeof(float), s));      // dense rows past an utterance's end
        TRY(vq_bigru_scan(cv.wf[l], cv.bhh[l], v->gi.as<float>(), v->hseq.as<float>(), xout, frames_dev, row0_dev, Hp, B, T2, s));
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

// Teacher-forced scan, after chunk `chunk` (steps [chunk*CH, (chunk+1)*CH)) has left its h_t in v->hall:
// a = relu(W1 h + b1) for all B*CH rows, logits = W2 a + b2 stored at (b, chunk*CH + tt) for tt < Ts - chunk*CH.
static int tf_chunk_gemms(vqcpc_vocoder *v, int B, int Ts, int CH, int chunk, float *logits, hipStream_t s) {
    const auto &d = v->d;
    const int M = B * CH;
    TRY(vq_gemm_chain_ex(v->hall.as<float>(), d.Hr, v->w_fc1, v->b_fc1, v->a1c.as<float>(), d.Hf, M, d.Hf, d.Hr, d.Hr,
                         1, 0, 0, 0, 0, s));
    TRY(vq_gemm_chain_ex(v->a1c.as<float>(), d.Hf, v->w_fc2, v->b_fc2, logits, d.n_cls, M, d.n_cls, d.Hf, d.Hf,
                         0, CH, Ts, chunk * CH, Ts, s));
    return VQCPC_OK;
}

// What a scoring call (vqcpc_vocoder_nll) hands the teacher-forced scan: its chunks end in the fused head of nll.hip instead of
// the two GEMMs, and nothing of size (B, Ts, n_cls) exists.
struct NllCall {
    const int64_t *audio;                // DEVICE (B, L): step t reads audio[b, t], its target is audio[b, t + 1]
    int L;
    std::vector<int> slen;               // scored steps per utterance: n_audio[b] - 1, at least 0
    float *nll;                          // DEVICE (B, L - 1) or null
    double *nll_sum; int64_t *n_scored, *n_correct;   // DEVICE (B)
    ArView w;                            // the weights the scan and the head read
    float *hsave;                        // DEVICE (B, L - 1, Hr) or null: h_t of every scored step (the gradients' forward)
    const float *cond_in;                // DEVICE (B, 2Tc, 2Hp) or null: the conditioning series given (run_conditioning)
};

CondView vq_cond_view(const vqcpc_vocoder *v) {
    CondView c{};
    c.code_emb = v->code_emb; c.spk_emb = v->spk_emb;
    const size_t whh = (size_t)3 * v->d.Hp * v->d.Hp;
    for (int l = 0; l < 2; ++l) {
        c.wih[l] = v->p_wih[l]; c.bih[l] = v->p_bih[l]; c.bhh[l] = v->p_bhh[l]; c.wf[l] = v->p_wf[l];
        c.whh[l][0] = v->p_whh[l]; c.whh[l][1] = v->p_whh[l] + whh;
    }
    return c;
}

// grid (B T2, ceil(C / 256))
__global__ void cond_rows_kernel(const float *__restrict__ src, float *__restrict__ dst, const int *__restrict__ frames,
                                 const int *__restrict__ gbase, int T2, int C, int to_dense) {
    const int c = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x / T2, f = blockIdx.x % T2;
    if (c >= C) return;
    const bool own = f < frames[b];
    const size_t dense = (size_t)blockIdx.x * C + c, ragged = ((size_t)gbase[b] + f) * C + c;
    if (to_dense) dst[dense] = own ? src[ragged] : 0.f;
    else if (own) dst[ragged] = src[dense];
}
void vq_cond_rows(const float *src, float *dst, const int *frames, const int *gbase, int B, int T2, int C, bool to_dense, hipStream_t s) {
    hipLaunchKernelGGL(cond_rows_kernel, dim3(B * T2, (C + 255) / 256), dim3(256), 0, s, src, dst, frames, gbase, T2, C, to_dense ? 1 : 0);
}

ArView vq_vocoder_view(const vqcpc_vocoder *v) {
    return ArView{v->w_cond, v->b_ih, v->Gemb, v->Gemb4, v->bh4, v->Wf_hh12, v->Wf_hh16, v->w_fc1, v->b_fc1, v->w_fc2, v->b_fc2, 0};
}

// h_t of the chunk's scored steps, from hall [B][CH][Hr] to the caller's (B, Tsv, Hr): grid (ceil(CH Hr / 4 / 256), B).  Rows at or
// past an utterance's scored length are left alone: the backward does not read them.
__global__ void tf_save_h_kernel(const float4 *__restrict__ hall, float4 *__restrict__ saved, const int *__restrict__ slen, int CH,
                                 int t0, int Tsv, int H4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    if (i >= CH * H4) return;
    const int tt = i / H4, u = i % H4, t = t0 + tt;
    if (t >= slen[b] || t >= Tsv) return;
    saved[((size_t)b * Tsv + t) * H4 + u] = hall[((size_t)b * CH + tt) * H4 + u];
}

static int tf_chunk_nll(vqcpc_vocoder *v, int B, int CH, int chunk, const NllCall &nc, hipStream_t s) {
    NllHead h{};
    h.hall = v->hall.as<float>(); h.w1 = nc.w.w_fc1; h.b1 = nc.w.b_fc1; h.w2 = nc.w.w_fc2; h.b2 = nc.w.b_fc2;
    h.audio = nc.audio; h.slen = v->nll_len.as<int>(); h.nll = nc.nll; h.part = v->nll_part.as<NllPart>();
    h.status = v->status.dev; h.status_tag = v->epoch << 8;
    h.B = B; h.L = nc.L; h.CH = CH; h.t0 = chunk * CH; h.Hr = v->d.Hr;
    TRY(vq_tf_nll_chunk(h, nc.nll_sum, nc.n_scored, nc.n_correct, s));
    if (nc.hsave) {
        const int H4 = v->d.Hr / 4;
        hipLaunchKernelGGL(tf_save_h_kernel, dim3((unsigned)((CH * H4 + 255) / 256), B), dim3(256), 0, s, (const float4 *)v->hall.as<float>(),
                           (float4 *)nc.hsave, v->nll_len.as<int>(), CH, chunk * CH, nc.L - 1, H4);
    }
    return VQCPC_OK;
}
// One resident, weight-stationary decoder per XCD (ar_xcd.hip, or its matrix-core form ar_xcm.hip): slot q runs the utterances
// of cp.dp.lists[q] back to back (no replay boundaries here).
int run_resident(vqcpc_vocoder *v, const CallPlan &cp, int T2, unsigned long long seed, float *wav, int64_t *mulaw, hipStream_t s, const Resume *rs) {
    VQ_REQUIRE(!rs || cp.dp.path == 2, "vocoder stream: chunks do not run on the matrix-core decoders");
    const auto &d = v->d;
    const DecodePlan &pl = cp.dp;
    const int B = (int)cp.utt.size();
    size_t max_seg = 1;
    for (auto &l : pl.lists) max_seg = l.size() + 1 > max_seg ? l.size() + 1 : max_seg;
    std::vector<XdSeg> tab((size_t)8 * pl.bxt * max_seg, XdSeg{-1, 0, 0, 0u});
    XdParams xp{};
    for (int q = 0; q < pl.xs; ++q) {
        for (size_t i = 0; i < pl.lists[q].size(); ++i) tab[(size_t)q * max_seg + i] = pl.lists[q][i];
        const int x = q % 8;
        if (pl.xend[q] + 1 > xp.n_steps[x]) xp.n_steps[x] = (int)pl.xend[q] + 1;
    }
    // behind the table: first Gcond row of every utterance (the kernels find it from the table's own address)
    const size_t tab_bytes = tab.size() * sizeof(XdSeg);
    TRY(v->xd_segs.reserve(tab_bytes + (size_t)B * sizeof(int)));
    TRY(v->stage.upload((char *)v->xd_segs.p + tab_bytes, cp.gbase.data(), (size_t)B * sizeof(int), s));
    TRY(v->xd_x.reserve(pl.path == 3 ? xm_exchange_bytes() : xd_exchange_bytes(pl.bxt)));
    TRY(v->stage.upload(v->xd_segs.p, tab.data(), tab_bytes, s));
    xp.w_hh = v->w_hh; xp.w_fc1 = v->w_fc1; xp.b_fc1 = v->b_fc1; xp.w_fc2 = v->w_fc2; xp.b_fc2 = v->b_fc2;
    xp.Gemb = v->Gemb; xp.b_hh = v->b_hh; xp.Gcond = v->gcond.as<float>(); xp.mulaw_tab = v->mulaw_tab;
    xp.segs = v->xd_segs.as<XdSeg>(); xp.xg = v->xd_x.as<unsigned long long>(); xp.status = v->status.dev;
    xp.status_tag = v->epoch << 8;
    xp.wav = wav; xp.mulaw = mulaw; xp.seed = seed; xp.max_seg = (int)max_seg; xp.n_slots = pl.xs; xp.bxt = pl.bxt;
    xp.Lout = d.upsample_t * T2; xp.F = T2; xp.upsample = d.upsample_t; xp.agent_stores = v->xcd_agent_stores;
    xp.timeout_ticks = (unsigned)v->xcd_timeout_ms * 100000u; xp.dbg_drop_step = v->xcd_debug_drop_step;
    xp.dbg_misplace = v->xcd_debug_misplace;
    if (rs) { xp.Lout = rs->Lout; xp.Gcond = rs->Gcond; }
    v->xcd_debug_misplace = 0;                     // one shot: the repeated call finds the workgroups where they are
    HIP_TRY(hipEventRecord(v->ev0, s));
    TRY(pl.path == 3 ? xm_launch(xp, s) : xd_launch(xp, s, rs ? &rs->x : nullptr));
    HIP_TRY(hipEventRecord(v->ev1, s));
    v->last_steps = (int)pl.longest;
    v->last_slots = pl.xs;
    v->last_path = pl.path;
    v->status_pending = true;
    return VQCPC_OK;
}

// The cached graph of one replay of group g (captured on first use).  A graph bakes its ArModel's buffer pointers: when a
// workspace of the group moved, the group's cached graphs are dropped first.
static int group_graph(vqcpc_vocoder *v, int g, const ArModel &m, int nbt, bool tf, int alt, hipGraphExec_t *out) {
    auto &G = v->grp[g];
    const void *now[8] = {G.har.p, G.a1.p, G.cand_s.p, G.cand_k.p, G.cur.p, G.gcur.p, G.candg.p, nullptr};
    if (memcmp(G.baked, now, sizeof now) != 0) {
        clear_graphs(G);
        memcpy(G.baked, now, sizeof now);
    }
    // what the capture bakes; alt: the model reads a caller's weights from the gradient work space (fixed addresses of their own)
    const int gkey = ((((nbt * 17 + m.live_last) * 2 + m.lead6) * 2 + (tf ? 1 : 0)) * 3 + m.fused) * 2 + alt;
    auto it = G.graphs.find(gkey);
    if (it == G.graphs.end()) {
        hipGraph_t gr = nullptr;
        hipGraphExec_t ge = nullptr;
        HIP_TRY(hipStreamBeginCapture(v->cap_stream, hipStreamCaptureModeThreadLocal));
        int rc = launch_ar_steps(step_of(v), m, G.call, nbt, v->steps_per_graph, tf, v->cap_stream);
        hipError_t e = hipStreamEndCapture(v->cap_stream, &gr);     // always end the capture, also on failure
        if (rc != VQCPC_OK || e != hipSuccess) {
            if (gr) (void)hipGraphDestroy(gr);
            if (rc != VQCPC_OK) return rc;
            HIP_TRY(e);
        }
        e = hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0);
        (void)hipGraphDestroy(gr);
        HIP_TRY(e);
        it = G.graphs.emplace(gkey, ge).first;
    }
    *out = it->second;
    return VQCPC_OK;
}

// The launch-per-step kernels: per tile group its state buffers, call record (ArCall) and model (ArModel), then the replays of
// steps_per_graph steps each -- captured graphs, or plain launches with use_graph = 0.
int run_launch_path(vqcpc_vocoder *v, const CallPlan &cp, const int64_t *inputs, int T2, int Ts, unsigned long long seed,
                    float *wav, int64_t *mulaw, float *logits, hipStream_t s, const Resume *rs, const NllCall *nc) {
    const auto &d = v->d;
    const int Hr = d.Hr, S = v->steps_per_graph, B = (int)cp.utt.size(), n_slots = cp.dp.xs, max_t = (int)cp.dp.longest;
    const bool tf = inputs != nullptr;     // teacher-forced scan: one group, GRU steps only, chunked GEMMs for fc1 / fc2
    ArCall calls[2];
    ArModel models[2];
    for (int g = 0; g < cp.n_grp; ++g) {
        auto &G = v->grp[g];
        const int nb = cp.tiles[g], Spg = nb * 16, slot0 = g * cp.tiles[0] * 16;
        // a scoring call uploads the table's first row only (ArCall::one_row): its work space does not depend on the call's length
        const size_t tab_n = nc ? (size_t)Spg : cp.table[g].size();
        TRY(G.slot_tab.reserve(tab_n * sizeof(XdSeg)));
        TRY(G.cur.reserve((size_t)Spg * sizeof(XdSeg)));
        TRY(v->stage.upload(G.slot_tab.p, cp.table[g].data(), tab_n * sizeof(XdSeg), s));
        TRY(v->stage.upload(G.cur.p, cp.table[g].data(), (size_t)Spg * sizeof(XdSeg), s));
        const size_t hsz = (size_t)nb * Hr * 16 * sizeof(float);
        TRY(G.har.reserve(2 * hsz));
        TRY(G.a1.reserve((size_t)nb * d.Hf * 16 * sizeof(float)));
        const size_t nrg = (size_t)d.n_cls / 16;
        TRY(G.cand_s.reserve((size_t)Spg * nrg * sizeof(float)));
        TRY(G.cand_k.reserve((size_t)Spg * nrg * sizeof(int)));
        TRY(G.gcur.reserve((size_t)Spg * Hr * sizeof(float4)));
        HIP_TRY(hipMemsetAsync(G.har.p, 0, 2 * hsz, s));
        HIP_TRY(hipMemsetAsync(G.cand_s.p, 0, (size_t)Spg * nrg * sizeof(float), s));
        HIP_TRY(hipMemsetAsync(G.cand_k.p, 0, (size_t)Spg * nrg * sizeof(int), s));
        const size_t cg_bytes = (size_t)nb * nrg * 16 * sizeof(u64);          // granules, then one 64-byte block for the abort word
        TRY(G.candg.reserve(cg_bytes + 64));
        HIP_TRY(hipMemsetAsync(G.candg.p, 0, cg_bytes + 64, s));
        ArCall &c = calls[g];
        c = ArCall{};
        c.Gcond = v->gcond.as<float>(); c.gbase = v->gbase.as<int>(); c.inputs = inputs; c.wav = wav; c.mulaw = mulaw; c.logits = logits;
        c.slots = G.slot_tab.as<XdSeg>(); c.S = S; c.Sp = Spg; c.n_rep = cp.rep[g] > 0 ? cp.rep[g] : 1;
        c.F = T2; c.Ts = Ts; c.Lout = d.upsample_t * T2; c.max_t = cp.gmax[g]; c.nbt = nb; c.seed = seed; c.t_base = 0;
        if (rs) {
            // sample s0 + j of a row goes to column 1 + j: the step kernels index with the absolute sample from a base s0 - 1 columns back
            c.Gcond = rs->Gcond; c.gbase = rs->gbase; c.Lout = rs->Lout;
            c.wav = wav ? (float *)((uintptr_t)wav - (uintptr_t)(rs->x.s0 - 1) * sizeof(float)) : nullptr;
            c.mulaw = mulaw ? (int64_t *)((uintptr_t)mulaw - (uintptr_t)(rs->x.s0 - 1) * sizeof(int64_t)) : nullptr;
            c.h_in = rs->x.s0 > 0 ? rs->x.h_in : nullptr; c.x_in = rs->x.x_in; c.h_out = rs->x.h_out; c.s0 = rs->x.s0;
        }
        if (tf) {
            c.CH = v->tf_chunk_replays * S;
            TRY(v->hall.reserve((size_t)B * c.CH * Hr * sizeof(float)));
            if (nc) {                                 // scoring: the chunk ends in the fused head; audio rows are L apart
                c.Ts = nc->L; c.one_row = 1;
                TRY(v->nll_part.reserve((size_t)B * vq_tf_nll_tiles(c.CH) * sizeof(NllPart)));
            } else TRY(v->a1c.reserve((size_t)B * c.CH * d.Hf * sizeof(float)));
            c.hall = v->hall.as<float>(); c.hall_t0 = 0;
            c.logits = nullptr;                       // written by the chunk GEMMs, not by ar_fc2_kernel
        }
        TRY(v->stage.upload(G.call.p, &c, sizeof c, s));
        ArModel &m = models[g];
        m = ArModel{};
        m.Wf_hh12 = v->Wf_hh12; m.Wf_hh16 = v->Wf_hh16; m.bh4 = v->bh4; m.Gemb4 = v->Gemb4; m.Gemb = v->Gemb; m.Wf_fc1 = v->Wf_fc1; m.Wf_fc1h = v->Wf_fc1h; m.b_fc1 = v->b_fc1;
        if (nc) {                                     // a scoring call's GRU steps read the call's view (the handle's, or a caller's weights)
            m.Wf_hh12 = nc->w.Wf_hh12; m.Wf_hh16 = nc->w.Wf_hh16; m.bh4 = nc->w.bh4; m.Gemb4 = nc->w.Gemb4; m.Gemb = nc->w.Gemb;
        }
        m.Wf_fc2 = v->Wf_fc2; m.b_fc2 = v->b_fc2; m.mulaw_tab = v->mulaw_tab;
        m.hbuf = G.har.as<float>(); m.a1 = G.a1.as<float>(); m.cand_s = G.cand_s.as<float>(); m.cand_k = G.cand_k.as<int>(); m.cur = G.cur.as<XdSeg>(); m.gcur4 = G.gcur.as<float4>();
        m.gc_replay = d.upsample_t % S == 0;
        const int live = (n_slots - slot0 < Spg ? n_slots - slot0 : Spg) - (nb - 1) * 16;
        m.live_last = live < 1 ? 1 : (live > 16 ? 16 : live);
        m.lead6 = cp.n_grp == 2 && nb <= 2;
        m.candg = G.candg.as<u64>();
        m.abort_dev = (unsigned *)((char *)G.candg.p + cg_bytes);
        m.abort_host = v->status.dev;
        m.timeout_ticks = (unsigned)v->handoff_timeout_ms * 100000u;
        m.dbg_drop_t = v->handoff_debug_drop_step;
        m.fused = (v->fuse_fc2 && !tf && cp.gmax[g] < (1 << CAND_TAG_BITS)) ? 1 : 0;
        m.Hr = Hr; m.Hf = d.Hf; m.n_cls = d.n_cls; m.upsample = d.upsample_t;
    }
    for (int g = 0; g < cp.n_grp; ++g)    // replay 0's slot row and Gcond rows
        launch_next_row(models[g], v->grp[g].call, cp.tiles[g], s);

    HIP_TRY(hipEventRecord(v->ev0, s));
    if (v->use_graph) {
        hipGraphExec_t exec[2] = {nullptr, nullptr};
        for (int g = 0; g < cp.n_grp; ++g) TRY(group_graph(v, g, models[g], cp.tiles[g], tf, nc ? nc->w.alt : 0, &exec[g]));
        if (cp.n_grp == 2) {              // group 1 runs on the side stream.  (Round 1 started it a fixed 12 000 cycles late "to
            HIP_TRY(hipEventRecord(v->ev_fork, s));                     // de-phase the groups": measured with and without, and with
            HIP_TRY(hipStreamWaitEvent(v->side_stream, v->ev_fork, 0));  // 40 000 -- the same 23.4 / 40.6 us per step at 256 / 512
        }                                                               // utterances; the streams drift over 200 replays anyway.)
        const int nr = cp.rep[0] > cp.rep[1] ? cp.rep[0] : cp.rep[1];
        for (int r = 0; r < nr; ++r) {
            if (r < cp.rep[0]) HIP_TRY(hipGraphLaunch(exec[0], s));
            if (cp.n_grp == 2 && r < cp.rep[1]) HIP_TRY(hipGraphLaunch(exec[1], v->side_stream));
            if (tf && ((r + 1) % v->tf_chunk_replays == 0 || r + 1 == nr))
                TRY(nc ? tf_chunk_nll(v, B, calls[0].CH, r / v->tf_chunk_replays, *nc, s)
                       : tf_chunk_gemms(v, B, Ts, calls[0].CH, r / v->tf_chunk_replays, logits, s));
        }
        if (cp.n_grp == 2) {
            HIP_TRY(hipEventRecord(v->ev_join, v->side_stream));
            HIP_TRY(hipStreamWaitEvent(s, v->ev_join, 0));
        }
    } else {
        for (int t0 = 0, r = 0; t0 < max_t; t0 += S, ++r) {
            TRY(launch_ar_steps(step_of(v), models[0], v->grp[0].call, cp.tiles[0], S, tf, s));
            if (tf && ((r + 1) % v->tf_chunk_replays == 0 || t0 + S >= max_t))
                TRY(nc ? tf_chunk_nll(v, B, calls[0].CH, r / v->tf_chunk_replays, *nc, s)
                       : tf_chunk_gemms(v, B, Ts, calls[0].CH, r / v->tf_chunk_replays, logits, s));
        }
    }
    HIP_TRY(hipEventRecord(v->ev1, s));
    v->last_steps = max_t;
    v->last_slots = n_slots;
    v->last_call = calls[0]; v->last_model = models[0]; v->last_path = 0;
    if (models[0].fused) v->status_pending = true;      // an in-kernel candidate wait may report a timeout
    return VQCPC_OK;
}

PlanOpts plan_opts(const vqcpc_vocoder *v) {
    const auto &d = v->d;
    return PlanOpts{v->xcd, v->xcm, v->xcm_min, v->xcm_max, v->xcd_slots, v->xcm_slots, v->n_slots, xd_supported(d.Hr, d.Hf, d.n_cls),
                    d.upsample_t, v->steps_per_graph, v->fuse_fc2, v->big_min_tiles, v->two_groups, v->use_graph};
}

// The next call's epoch: the kernels tag the status word with it (24 bits, never 0).
static void next_epoch(vqcpc_vocoder *v) { v->epoch = (v->epoch + 1u) & 0xffffffu ? (v->epoch + 1u) & 0xffffffu : 1u; }

// Everything a call may upload through the pinned arena (no synchronisation of the caller's stream): the layout's lengths, row
// bases and scored lengths; then either both groups' slot tables, first rows and call records (launch path) or the resident
// decoders' segment table (at most B + 1 segments in each of 8 * XM_BX slots) and row bases; 256 bytes for the 16-byte alignment.
static size_t stage_bytes(const CallPlan &cp, int B) {
    return cp.lens.size() * sizeof(int) + (cp.table[0].size() + cp.table[1].size()) * sizeof(XdSeg) +
           (size_t)(cp.tiles[0] + cp.tiles[1]) * 16 * sizeof(XdSeg) + 2 * sizeof(ArCall) + 256 +
           (size_t)8 * XM_BX * (B + 1) * sizeof(XdSeg) + (size_t)3 * (B + 16) * sizeof(int);
}

int begin_call(vqcpc_vocoder *v, const CallPlan &cp, int B) {
    TRY(status_check(v, false));          // has an earlier call's hand-off reported already?  (nothing is cleared without a sync)
    next_epoch(v);
    return v->stage.begin(stage_bytes(cp, B));
}

int vq_upload_layout(vqcpc_vocoder *v, const UttLayout &u, DevBuf &gbase, hipStream_t s) {
    TRY(v->len.reserve(u.lens.size() * sizeof(int)));
    TRY(v->stage.upload(v->len.p, u.lens.data(), u.lens.size() * sizeof(int), s));
    TRY(gbase.reserve(u.gbase.size() * sizeof(int)));
    return v->stage.upload(gbase.p, u.gbase.data(), u.gbase.size() * sizeof(int), s);
}

int vq_cond_run(vqcpc_vocoder *v, const UttLayout &u, const CondView &cv, const int64_t *idx, const int64_t *spk, int B, int Tc, DevBuf &gbase,
                float *series, float *out0, float *cond, hipStream_t s) {
    TRY(vq_upload_layout(v, u, gbase, s));
    return run_condition(v, cv, idx, spk, B, Tc, v->len.as<int>(), gbase.as<int>(), (size_t)u.grows, series, out0, cond, s);
}

int run_conditioning(vqcpc_vocoder *v, const UttLayout &u, const int64_t *idx, const int64_t *spk, int B, int Tc,
                     DevBuf &cond, DevBuf &gcond, DevBuf &gbase, hipStream_t s, const float *w_cond, const float *b_ih, const float *cond_in) {
    const int Hr = v->d.Hr, dl = 2 * v->d.Hp;
    const size_t crows = u.grows > 0 ? (size_t)u.grows : 1;
    TRY(cond.reserve(crows * dl * sizeof(float)));
    if (cond_in) {
        TRY(vq_upload_layout(v, u, gbase, s));
        vq_cond_rows(cond_in, cond.as<float>(), v->len.as<int>(), gbase.as<int>(), B, 2 * Tc, dl, false, s);
        HIP_TRY(hipGetLastError());
    } else TRY(vq_cond_run(v, u, vq_cond_view(v), idx, spk, B, Tc, gbase, nullptr, nullptr, cond.as<float>(), s));
    TRY(gcond.reserve(crows * 3 * Hr * sizeof(float)));
    if (u.grows > 0)
        TRY(vq_gemm_chain(cond.as<float>(), dl, w_cond ? w_cond : v->w_cond.as<float>(), b_ih ? b_ih : v->b_ih.as<float>(), gcond.as<float>(),
                          3 * Hr, (int)u.grows, 3 * Hr, dl, dl, s));
    return VQCPC_OK;
}

int vq_vocoder_relayout(vqcpc_vocoder *v, const float *embedding, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        const float *fc1_weight, const float *fc1_bias, const float *fc2_weight, const float *fc2_bias, bool scan, ArView *out, hipStream_t s) {
    // what vocoder_create_impl builds for the scan, from the caller's tensors, in stream order
    const auto &d = v->d;
    const int Hr = d.Hr, de = d.de, dl = 2 * d.Hp;
    VocGradWork &g = v->gw;
    TRY(g.w_emb.reserve((size_t)3 * Hr * de * sizeof(float)));
    TRY(g.w_cond.reserve((size_t)3 * Hr * dl * sizeof(float)));
    TRY(g.Gemb.reserve((size_t)d.n_cls * 3 * Hr * sizeof(float)));
    hipLaunchKernelGGL(copy_submatrix_kernel, dim3((unsigned)(((size_t)3 * Hr * de + 255) / 256)), dim3(256), 0, s, w_ih, de + dl, 0, g.w_emb.as<float>(), 3 * Hr, de);
    hipLaunchKernelGGL(copy_submatrix_kernel, dim3((unsigned)(((size_t)3 * Hr * dl + 255) / 256)), dim3(256), 0, s, w_ih, de + dl, de, g.w_cond.as<float>(), 3 * Hr, dl);
    TRY(vq_gemm_chain(embedding, de, g.w_emb.as<float>(), nullptr, g.Gemb.as<float>(), 3 * Hr, d.n_cls, 3 * Hr, de, de, s));
    if (scan) {
        TRY(g.Gemb4.reserve((size_t)d.n_cls * Hr * sizeof(float4)));
        TRY(g.bh4.reserve((size_t)Hr * sizeof(float4)));
        hipLaunchKernelGGL(quads_build_kernel, dim3((unsigned)(((size_t)d.n_cls * Hr + 255) / 256)), dim3(256), 0, s, g.Gemb.as<float>(), g.Gemb4.as<float4>(), d.n_cls, Hr);
        hipLaunchKernelGGL(quads_build_kernel, dim3((unsigned)((Hr + 255) / 256)), dim3(256), 0, s, b_hh, g.bh4.as<float4>(), 1, Hr);
        TRY(build_wfrag12(w_hh, Hr, Hr / 4, Hr, Hr, g.Wf12, s));
        if (Hr % 16 == 0) TRY(vq_build_wfrag(w_hh, Hr, 3 * (Hr / 16), Hr, 4, 16, Hr, g.Wf16, s));
    }
    HIP_TRY(hipGetLastError());
    *out = ArView{g.w_cond.as<float>(), b_ih, g.Gemb.as<float>(), g.Gemb4.as<float4>(), g.bh4.as<float4>(), g.Wf12.as<float>(), g.Wf16.as<float>(),
                  fc1_weight, fc1_bias, fc2_weight, fc2_bias, 1};
    return VQCPC_OK;
}

// Shared driver of generate() and logits(): validate and plan on the host, upload the tables and run the conditioning, then
// the decode loop the plan chose.
static int run_ar(vqcpc_vocoder *v, const int64_t *idx, const int64_t *spk, int B, int Tc, const int *n_codes_host,
                  const int64_t *inputs, int Ts, unsigned long long seed, unsigned utt_base,
                  const uint32_t *utt_ids_host, float *wav,
                  int64_t *mulaw, float *logits, int max_steps, hipStream_t s, const NllCall *nc = nullptr) {
    const int Lout = v->d.upsample_t * 2 * Tc;
    CallPlan cp;
    TRY(plan_call(plan_opts(v), B, Tc, n_codes_host, inputs != nullptr, Ts, max_steps, utt_base, utt_ids_host, cp, nc ? nc->slen.data() : nullptr));
    TRY(begin_call(v, cp, B));
    TRY(run_conditioning(v, cp, idx, spk, B, Tc, v->cond, v->gcond, v->gbase, s, nc ? nc->w.w_cond : nullptr, nc ? nc->w.b_ih : nullptr,
                         nc ? nc->cond_in : nullptr));
    if (wav) HIP_TRY(hipMemsetAsync(wav, 0, (size_t)B * Lout * sizeof(float), s));
    if (mulaw) HIP_TRY(hipMemsetAsync(mulaw, 0, (size_t)B * Lout * sizeof(int64_t), s));
    if (v->last_path != 0) v->last_path = 1;      // a call that fails from here on ran no decode loop
    VQ_REQUIRE(!nc || cp.dp.path == 0, "vocoder.nll: a scoring call must take the launch path (planned path %d)", cp.dp.path);
    if (cp.dp.path != 0) return run_resident(v, cp, 2 * Tc, seed, wav, mulaw, s);
    if (nc) {
        TRY(v->nll_len.reserve((size_t)B * sizeof(int)));
        TRY(v->stage.upload(v->nll_len.p, nc->slen.data(), (size_t)B * sizeof(int), s));
    }
    return run_launch_path(v, cp, inputs, 2 * Tc, Ts, seed, wav, mulaw, logits, s, nullptr, nc);
}

extern "C" int vqcpc_vocoder_generate(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                                      const int *n_codes, uint64_t seed, uint32_t utt_base, const uint32_t *utt_ids,
                                      float *wav, int64_t *mulaw, int max_steps, void *stream) {
    VQ_REQUIRE(v && idx && speaker && wav, "vqcpc_vocoder_generate: null argument");
    VQ_REQUIRE(B > 0 && Tc > 0, "vocoder.generate: need B > 0 and Tc > 0 (got %d, %d)", B, Tc);
    return run_ar(v, idx, speaker, B, Tc, n_codes, nullptr, 0, seed, utt_base, utt_ids, wav, mulaw, nullptr, max_steps,
                  (hipStream_t)stream);
}

extern "C" int vqcpc_vocoder_logits(vqcpc_vocoder *v, const int64_t *x, const int64_t *idx, const int64_t *speaker,
                                    int B, int Tc, int Ts, float *logits, void *stream) {
    VQ_REQUIRE(v && x && idx && speaker && logits, "vqcpc_vocoder_logits: null argument");
    VQ_REQUIRE(B > 0 && Tc > 0 && Ts > 0 && Ts <= 2 * v->d.upsample_t * Tc,
               "vocoder.forward: Ts=%d must be in (0, %d]", Ts, 2 * v->d.upsample_t * Tc);
    VQ_REQUIRE(((uintptr_t)logits & 15) == 0, "vocoder.forward: logits must be 16-byte aligned");
    return run_ar(v, idx, speaker, B, Tc, nullptr, x, Ts, 0, 0, nullptr, nullptr, nullptr, logits, 0, (hipStream_t)stream);
}

extern "C" int vqcpc_vocoder_nll(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                                 int L, const int *n_codes, const int *n_audio, double *nll_sum, int64_t *n_scored,
                                 int64_t *n_correct, float *nll, void *stream) {
    VQ_REQUIRE(v && audio && idx && speaker && nll_sum && n_scored && n_correct, "vqcpc_vocoder_nll: null argument");
    std::vector<int> slen;
    int longest = 0;
    TRY(vq_tf_check(v, B, Tc, L, n_codes, n_audio, slen, &longest));
    return vq_tf_score(v, audio, idx, speaker, B, Tc, L, n_codes, slen, longest, nullptr, nll_sum, n_scored, n_correct, nll, nullptr,
                       (hipStream_t)stream);
}

int vq_tf_check(const vqcpc_vocoder *v, int B, int Tc, int L, const int *n_codes, const int *n_audio, std::vector<int> &slen, int *longest) {
    VQ_REQUIRE(B > 0 && Tc > 0 && L > 0, "vocoder.nll: need B > 0, Tc > 0 and L > 0 (got %d, %d, %d)", B, Tc, L);
    const auto &d = v->d;
    VQ_REQUIRE(d.Hf == NLL_HF && d.n_cls == NLL_CLS, "vocoder.nll: the scoring head is built for size_h_fc %d and %d classes "
               "(config.py:69,77), this model has %d and %d", NLL_HF, NLL_CLS, d.Hf, d.n_cls);
    slen.assign(B, 0);
    *longest = 0;
    for (int b = 0; b < B; ++b) {
        const int na = n_audio ? n_audio[b] : L, ncd = n_codes ? n_codes[b] : Tc;
        VQ_REQUIRE(na >= 0 && na <= L, "vocoder.nll: n_audio[%d] = %d outside [0, %d]", b, na, L);
        VQ_REQUIRE(ncd >= 0 && ncd <= Tc, "vocoder: n_codes[%d] = %d outside [0, %d]", b, ncd, Tc);
        VQ_REQUIRE((long)na - 1 <= (long)2 * d.upsample_t * ncd, "vocoder.nll: utterance %d has %d samples to score but its %d codes "
                   "cover %ld (n_audio - 1 <= 2 * upsample_t * n_codes)", b, na - 1, ncd, (long)2 * d.upsample_t * ncd);
        slen[b] = na >= 2 ? na - 1 : 0;
        *longest = slen[b] > *longest ? slen[b] : *longest;
    }
    return VQCPC_OK;
}

int vq_tf_score(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L, const int *n_codes,
                const std::vector<int> &slen, int longest, const ArView *w, double *nll_sum, int64_t *n_scored, int64_t *n_correct, float *nll,
                float *hsave, hipStream_t s, const float *cond_in) {
    NllCall nc{audio, L, slen, nll, nll_sum, n_scored, n_correct, w ? *w : vq_vocoder_view(v), hsave, cond_in};
    HIP_TRY(hipMemsetAsync(nll_sum, 0, (size_t)B * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(n_scored, 0, (size_t)B * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(n_correct, 0, (size_t)B * sizeof(int64_t), s));
    if (nll && L > 1) HIP_TRY(hipMemsetAsync(nll, 0, (size_t)B * (L - 1) * sizeof(float), s));
    if (longest == 0) return VQCPC_OK;         // no row has two samples: nothing to score
    return run_ar(v, idx, speaker, B, Tc, n_codes, audio, longest, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, s, &nc);
}

int vq_tf_condition(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes, const std::vector<int> &slen,
                    const ArView *w, UttLayout &u, hipStream_t s, const float *cond_in) {
    CallPlan cp;                               // no decode loop: the layout alone sizes the staging arena
    TRY(utt_layout(B, Tc, n_codes, v->d.upsample_t, 0, nullptr, cp));
    TRY(begin_call(v, cp, B));
    TRY(run_conditioning(v, cp, idx, speaker, B, Tc, v->cond, v->gcond, v->gbase, s, w ? w->w_cond : nullptr, w ? w->b_ih : nullptr, cond_in));
    TRY(v->nll_len.reserve((size_t)B * sizeof(int)));
    TRY(v->stage.upload(v->nll_len.p, slen.data(), (size_t)B * sizeof(int), s));
    u = cp;
    return VQCPC_OK;
}

// Average wall time of `reps` back-to-back launches of each per-sample kernel (HIP events on
// `stream`), on the state the last generate()/logits() call left behind.  Includes the ~1.5 us
// dependent-launch boundary of this chip.  out_us = {ar_gru, ar_fc1, ar_fc2}.
// A fused launch is timed on successive odd local steps (same state-buffer parity, a NEW step number each time), so
// that its gate waves really wait for the candidates its own fc2 workgroups produce -- relaunching one step would find
// the previous repetition's granules already tagged with it and time the launch without its hand-off.
extern "C" int vqcpc_vocoder_kernel_times(vqcpc_vocoder *v, int reps, float *out_us, void *stream) {
    VQ_REQUIRE(v && out_us && reps > 0, "vqcpc_vocoder_kernel_times: bad argument");
    VQ_REQUIRE(v->last_path == 0, "vqcpc_vocoder_kernel_times: call generate() or logits() first");
    hipStream_t s = (hipStream_t)stream;
    ArCall c = v->last_call;
    c.t_base = 1;                        // a mid-utterance step (t = 1: candidates are merged, Gemb gathered)
    c.wav = nullptr; c.mulaw = nullptr; c.logits = nullptr;
    ArCall *call = v->grp[0].call;
    const ArStep a = step_of(v);
    HIP_TRY(hipMemcpyAsync(call, &c, sizeof c, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    const ArModel m = v->last_model;
    const bool tbig = use_big(a, c.nbt);
    const int nf = tbig ? (v->d.n_cls / 16) * c.nbt / 4 : (v->d.n_cls / 16) * c.nbt;   // fused launch: fc2 blocks of step t-1 in front of the GRU blocks of step t
    int fresh = 0;                       // fused launches so far
    for (int which = 0; which < 3; ++which) {
        for (int pass = 0; pass < 2; ++pass) {          // pass 0 = warm-up
            if (pass == 1) HIP_TRY(hipEventRecord(v->ev0, s));
            const int n = pass == 0 ? 20 : reps;
            for (int i = 0; i < n; ++i) {
                if (which == 2) { launch_fc2_step(a, m, call, 0, c.nbt, s); continue; }
                if (which == 1) { TRY(launch_fc1_step(a, m, call, 0, c.nbt, s)); continue; }
                const int period = c.max_t > 5 ? (c.max_t - 3) / 2 : 1;              // keep t = t_base + tl inside the call (reps beyond
                const int tl = m.fused ? 1 + 2 * (fresh++ % period) : 0;             // that reuse steps, i.e. find their tags in place)
                TRY(launch_gru_step(a, m, call, tl, c.nbt, m.fused ? nf : 0, s));
            }
        }
        HIP_TRY(hipEventRecord(v->ev1, s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, v->ev0, v->ev1));
        out_us[which] = ms * 1e3f / (float)reps;
    }
    out_us[3] = (float)(c.nbt * 16);       // decode slots one launch of the timed configuration covers
    out_us[4] = m.fused ? (tbig ? 5.f : 4.f) : (c.nbt == 1 ? 0.f : (tbig ? 2.f : 1.f));    // which GRU-step kernel that configuration runs
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_glue(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc, float *series,
                                  void *stream) {
    VQ_REQUIRE(v && idx && speaker && series && B > 0 && Tc > 0, "vqcpc_vocoder_glue: bad argument");
    const auto &d = v->d;
    const size_t ng = (size_t)B * 2 * Tc * (d.dz + d.ds);
    hipLaunchKernelGGL(glue_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx, speaker, v->code_emb,
                       v->spk_emb, series, B, Tc, d.dz, d.ds, d.n_codes, d.n_speakers, v->status.dev, v->epoch << 8, nullptr, nullptr);
    v->status_pending = true;
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_condition(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                                       float *cond, void *stream) {
    VQ_REQUIRE(v && idx && speaker && cond && B > 0 && Tc > 0, "vqcpc_vocoder_condition: bad argument");
    return run_condition(v, vq_cond_view(v), idx, speaker, B, Tc, nullptr, nullptr, 0, nullptr, nullptr, cond, (hipStream_t)stream);
}
