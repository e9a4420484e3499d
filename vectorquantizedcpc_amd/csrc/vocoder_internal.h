// The vocoder handle (struct vqcpc_vocoder), its decode plan types and what vocoder_host.hip, vocoder_plan.hip and
// vocoder_stream.hip share.  Nothing here is a kernel source: the step kernels' side of the interface is ar_step.h.
#pragma once
#include "common.h"
#include "ar_shared.h"
#include "ar_xcd.h"
#include "ar_step.h"
#include "nll.h"
#include <string.h>
#include <map>
#include <vector>

// Pinned staging arena for host-built tables (lengths, decode-slot schedule, call records): the tables are copied in
// and uploaded from there with hipMemcpyAsync, so a decode call never synchronises the caller's stream ("no
// hidden sync").  The arena is reused by the next call only after the event recorded behind this call's uploads.
struct HostStage {
    HostBuf mem;
    size_t used = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    ~HostStage() {
        drain();
        if (ev) (void)hipEventDestroy(ev);
    }
    void drain() {                       // wait for the uploads still reading the arena
        if (pending && ev) (void)hipEventSynchronize(ev);
        pending = false;
    }
    int begin(size_t need) {
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (pending) { HIP_TRY(hipEventSynchronize(ev)); pending = false; }       // the PREVIOUS call's uploads only
        if (need > mem.cap) TRY(mem.reserve(need + need / 2 + 4096));
        used = 0;
        return VQCPC_OK;
    }
    int upload(void *dst, const void *src, size_t n, hipStream_t s) {
        const size_t at = (used + 15) & ~(size_t)15;
        VQ_REQUIRE(at + n <= mem.cap, "host staging arena too small (%zu + %zu > %zu)", at, n, mem.cap);
        char *p = (char *)mem.p;
        memcpy(p + at, src, n);
        used = at + n;
        HIP_TRY(hipMemcpyAsync(dst, p + at, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(ev, s));
        pending = true;
        return VQCPC_OK;
    }
};

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
// Defaults of the decode-loop options: the handle starts with them, and vqcpc_vocoder_plan takes them for -1 / 0.
constexpr int XCM_MIN_DEFAULT = 68, XCM_MAX_DEFAULT = 512, XCD_SLOTS_DEFAULT = 8 * XD_MAX_BX, XCM_SLOTS_DEFAULT = 8 * XM_BX;

// The sample-rate network's weights as the teacher-forced scan, its head and the conditioning's last product read them: the
// handle's copies (alt 0), or the layouts a gradient entry made from a caller's tensors for one call (alt 1; the captured step
// graphs bake these pointers, so the two sets have graphs of their own).
struct ArView {
    const float *w_cond, *b_ih;          // W_ih[:, de:] as a contiguous (3Hr, C); (3Hr)
    const float *Gemb;                   // [n_cls][3Hr]
    const float4 *Gemb4, *bh4;
    const float *Wf_hh12, *Wf_hh16;
    const float *w_fc1, *b_fc1, *w_fc2, *b_fc2;      // plain
    int alt;
};

// Work space of the vocoder gradients (vocoder_grad.hip), grow-only, counted by vqcpc_vocoder_workspace_bytes.
struct VocGradWork {
    DevBuf w_emb, w_cond, Gemb, Gemb4, bh4, Wf12, Wf16;       // a caller's weights, re-laid per call
    DevBuf hcur, hprev, gh, nn, a1, dl, da, dhh, dgi, dghn, carry, dGemb, dGc;     // backward: one chunk's rows, the carry, the two table gradients
    std::vector<const DevBuf *> all() const {
        return {&w_emb, &w_cond, &Gemb, &Gemb4, &bh4, &Wf12, &Wf16, &hcur, &hprev, &gh, &nn, &a1, &dl, &da, &dhh, &dgi, &dghn, &carry, &dGemb, &dGc};
    }
};

// The conditioning path's weights as glue_kernel, the hoisted projections and the bi-GRU scan read them, per layer with both
// directions stacked: the handle's copies, or the layouts a gradient entry made from a caller's tensors for one call.
struct CondView {
    const float *code_emb, *spk_emb;
    const float *wih[2], *bih[2], *bhh[2];           // (2, 3Hp, I), (2, 3Hp), (2, 3Hp)
    const float *wf[2];                  // W_hh fragments of both directions (vq_build_wfrag, rowmode 3), null where no scan runs
    const float *whh[2][2];              // plain (3Hp, Hp) per layer and direction (the backward's products)
};

// Work space of the conditioning path's gradients (prenet_grad.hip), grow-only, counted by vqcpc_vocoder_workspace_bytes.
struct CondGradWork {
    DevBuf wih[2], bih[2], bhh[2], wf[2], frag;      // a caller's weights, re-laid per call (frag: one direction's fragments on their way)
    DevBuf wft;                          // backward: one layer's W_hh^T fragments, both directions
    DevBuf hprev, gh, nn, dout, dgi, dgh, carry, dx0, keys;  // backward: one layer's rows, the carry, dseries, the rows' table indices
    std::vector<const DevBuf *> all() const {
        return {&wih[0], &wih[1], &bih[0], &bih[1], &bhh[0], &bhh[1], &wf[0], &wf[1], &frag, &wft, &hprev, &gh, &nn, &dout, &dgi,
                &dgh, &carry, &dx0, &keys};
    }
};

struct vqcpc_vocoder {
    ~vqcpc_vocoder();                    // what is not memory: graphs, the arena's pending uploads, streams, events (vocoder_host.hip)
    vqcpc_vocoder_weights d;             // dims only (the weights below are owned copies)
    int device = 0;                      // the device the handle was created on
    DevPtr<float> code_emb, spk_emb;
    DevPtr<float> p_wih[2], p_bih[2], p_bhh[2], p_wf[2];   // per layer, both directions stacked
    DevPtr<float> p_whh[2];              // plain (2, 3Hp, Hp) copies of the prenet's W_hh (the gradients of the conditioning path)
    DevPtr<float> w_cond, b_ih, Gemb;
    DevPtr<float> ar_emb, w_emb;         // plain copies of the sample embedding and of W_ih[:, :de] (the gradients of the Gemb table)
    VocGradWork gw;
    CondGradWork cg;
    DevPtr<float4> Gemb4, bh4;
    DevPtr<float> Wf_hh12, Wf_hh16, b_hh, Wf_fc1, Wf_fc1h, b_fc1, Wf_fc2, b_fc2;
    DevPtr<float> w_fc1, w_fc2;          // plain (rows, K) copies for the teacher-forced scan's batched GEMMs
    DevPtr<float> mulaw_tab;
    // A decode call runs as 1 or 2 independent TILE GROUPS (disjoint utterance tiles, own state,
    // own call record, own captured graph).  Two groups run on two streams so that one group's GRU
    // step overlaps the other's fc1/fc2; there is no edge between them inside a graph.
    struct Group {
        DevPtr<ArCall> call;             // device
        DevBuf har, a1, cand_s, cand_k, slot_tab, cur, gcur, candg;   // candg: candidate granules + the abort word behind them
        std::map<int, hipGraphExec_t> graphs;   // key: (tiles in the group, live columns of the last tile, lead6)
        const void *baked[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // workspace pointers the cached graphs captured
    } grp[2];
    int two_groups = 1;                  // 0 = always one group
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DevBuf series, gi, out0, cond, gcond, gbase, hseq, len;
    DevBuf hall, a1c;                    // teacher-forced scan: h_t and fc1 outputs of one chunk
    DevBuf nll_part, nll_len;            // scoring (vqcpc_vocoder_nll): one chunk's (utterance, workgroup) records; scored steps per utterance
    PinnedWord status;                   // the handle's status word: the kernels write it, the host reads it without a HIP call
    HostStage stage;
    DevPtr<float> w_hh;                  // plain (3Hr, Hr) copy of W_hh for the resident decoders
    int fuse_fc2 = 1;                    // fc2 + draw of step t-1 and the GRU step t share one launch
    bool status_pending = false;         // a call with in-kernel hand-offs is in flight: its status word has not been read behind a sync yet
    unsigned epoch = 0;                  // calls of run_ar so far: the resident decoders tag the status word with it
    int last_slots = 0;                  // decode slots the last call's loop actually used
    // Fallback policy.  A placement miss (STATUS_MISPLACED: the 256 workgroups were not dealt 32 per XCD -- another kernel held CUs) wrote
    // nothing and is transient: the call is reported, the handle keeps its options, the caller repeats; only the second miss in
    // a row switches the resident decoders off.  A timeout (STATUS_TIMEOUT) switches the in-kernel hand-offs off at once and the
    // handle re-arms itself after REARM_CLEAN clean calls (or when the option is set again).
    int placement_misses = 0;
    bool fell_back = false;
    int saved_xcd = -1, saved_fuse_fc2 = 1, clean_calls = 0;
    // one resident decoder per XCD (ar_xcd.hip): -1 auto, 0 never, 1 whenever the dimensions allow
    int handoff_timeout_ms = 250;        // bound of the candidate waits of the fused fc2 || GRU launch
    int handoff_debug_drop_step = -1;    // tests: one fc2 team skips its publish at this step
    int xcd = -1;
    int xcd_slots = XCD_SLOTS_DEFAULT;   // decode slots it may use (<= 8 * XD_MAX_BX); more utterances run back to back in them
    int xcd_agent_stores = 0;            // tests / A-B: publish with agent-scope stores
    int xcd_timeout_ms = 250;            // bound of its in-kernel waits
    int xcd_debug_drop_step = -1;        // tests: one worker skips a candidate publish at this step -> the waits time out
    // the same decoders on the matrix cores, 16 slots per XCD (ar_xcm.hip): -1 auto (more than xcm_min and fewer than xcm_max
    // utterances in flight), 0 never, 1 whenever the dimensions allow.  Measured (tools/xcm_probe.py, bench_by_batch): 10.3 us
    // per step whatever the number of slots in use -> 6.2 M samples/s at 64 utterances (ar_xcd.hip through its 32 slots: 8.5 M),
    // 12.3 M at 128 and 256 (launches: 8.2 / 10.8 M), against 12.4 M on the launch path with 512 utterances in flight.
    int xcm = -1;
    int xcm_min = XCM_MIN_DEFAULT, xcm_max = XCM_MAX_DEFAULT;
    int xcm_slots = XCM_SLOTS_DEFAULT;
    int xcd_debug_misplace = 0;          // tests: workgroup 0 reports the wrong XCD -> status 2, nothing written
    DevBuf xd_x, xd_segs;                // exchange area, slot schedule
    int tf_chunk_replays = 4;            // graph replays (of steps_per_graph steps) per chunk of the teacher-forced scan
    int use_graph = 1, steps_per_graph = 160;
    int n_slots = 0;                     // 0 = one slot per utterance; else continuous batching over this many
    int big_min_tiles = 5;               // utterance tiles from which the LDS-staged GRU kernel is used (0 = never);
                                         // measured (profiles/r02_gru_variants.csv): 17.2 vs 19.0 us per step at 5 tiles, 17.2 vs 14.9 at 4
    bool big_attr_set = false;
    hipStream_t cap_stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int last_steps = 0;
    ArCall last_call{};                  // host copies of group 0 of the last decode call (kernel timing)
    ArModel last_model{};
    int last_path = 1;                   // vqcpc_vocoder_last_path: 0 launch path (last_call / last_model valid), 1 none, 2 / 3 resident
};

// ------------------------------------------------------------------------------------------
// decode planner (vocoder_plan.hip): pure host arithmetic, no HIP call
// ------------------------------------------------------------------------------------------

// What the planner reads of the handle (plan_opts fills it): the first row decides the path (plan_decode), the second lays
// out the launch path (plan_launch_tables).
struct PlanOpts {
    int xcd, xcm, xcm_min, xcm_max, xcd_slots, xcm_slots, n_slots; bool supported;
    int upsample_t, steps_per_graph, fuse_fc2, big_min_tiles, two_groups, use_graph;
};

// path 2 / 3: the per-XCD decoders (VALU / matrix-core form) through `xs` slots, slot q running lists[q] back to back;
// path 0: the launch-per-step kernels.
struct DecodePlan {
    int path = 0, xs = 0, bxt = 0;
    long longest = 0;
    std::vector<std::vector<XdSeg>> lists;
    std::vector<long> xend;
};

// The utterances of a call (or of a stream) as laid out on the host.
struct UttLayout {
    std::vector<int> lens;               // [frames | samples] per utterance, Bp = B rounded up to 16 entries each
    std::vector<unsigned> utt;           // sampling-stream id per utterance
    std::vector<int> gbase;              // first conditioning row per utterance (prefix sums of the frame counts), Bp entries
    long grows = 0;                      // conditioning rows in all
};

// A decode call as planned on the host before anything is uploaded.
struct CallPlan : UttLayout {
    DecodePlan dp;                       // path 0: the launch path's dp.xs slots, utterances starting at replay boundaries
    int n_grp = 1, tiles[2] = {0, 0}, rep[2] = {0, 0}, gmax[2] = {0, 0};   // launch path: tile groups (tiles, replays, steps)
    std::vector<XdSeg> table[2];         // launch path: per group [replay][slot] what every decode slot is doing
};

std::vector<int> longest_first(const int *samples, int B);
int utt_layout(int B, int Tc, const int *n_codes_host, int upsample_t, unsigned utt_base, const uint32_t *utt_ids_host, UttLayout &u);
bool plan_decode(const PlanOpts &o, const int *samples, const unsigned *utt, const std::vector<int> &order, DecodePlan &pl);
int plan_call(const PlanOpts &o, int B, int Tc, const int *n_codes_host, bool tf, int Ts, int max_steps, unsigned utt_base, const uint32_t *utt_ids_host, CallPlan &cp, const int *tf_len = nullptr);
int plan_launch_tables(const PlanOpts &o, const int *samples, const std::vector<int> &order, bool tf, int B, int s0, CallPlan &cp);

// ------------------------------------------------------------------------------------------
// what the stream (vocoder_stream.hip) calls in vocoder_host.hip
// ------------------------------------------------------------------------------------------
// What a stream chunk (vqcpc_vocoder_stream_next) hands the decode loops: every utterance resumes at absolute sample x.s0 from
// (x.h_in, x.x_in) -- null at s0 = 0 -- and leaves its final h in x.h_out.  wav / mulaw are the stream's (B, Lout = n + 1) buffers:
// sample s0 + j at column 1 + j, column 0 takes what the first step re-emits.  The conditioning is the stream's own.
// gbase: device copy of the layout's gbase (the launch path reads it).
struct Resume { XdResume x; int Lout; const float *Gcond; const int *gbase; };
struct NllCall;

PlanOpts plan_opts(const vqcpc_vocoder *v);
// Start of every call that uploads: an earlier call's report, the next epoch, the staging arena sized for this plan.
int begin_call(vqcpc_vocoder *v, const CallPlan &cp, int B);
// Upload the layout's frame counts and row bases, run the prenet over every utterance's own frames and make the Gcond rows.
// w_cond, b_ih: the last product's operands (an ArView's), null = the handle's copies.  cond_in (B, 2Tc, 2Hp) or null: the
// conditioning series given -- its rows of the utterances' own frames are packed into `cond` and the prenet does not run.
int run_conditioning(vqcpc_vocoder *v, const UttLayout &u, const int64_t *idx, const int64_t *spk, int B, int Tc, DevBuf &cond, DevBuf &gcond, DevBuf &gbase, hipStream_t s,
                     const float *w_cond = nullptr, const float *b_ih = nullptr, const float *cond_in = nullptr);

// ------------------------------------------------------------------------------------------
// what the conditioning path's gradient entries (prenet_grad.hip) call in vocoder_host.hip
// ------------------------------------------------------------------------------------------
CondView vq_cond_view(const vqcpc_vocoder *v);
// The layout's frame counts (-> v->len) and row bases (-> gbase) on the device, through the staging arena of the call begun.
int vq_upload_layout(vqcpc_vocoder *v, const UttLayout &u, DevBuf &gbase, hipStream_t s);
// run_conditioning's first half: upload the layout's frame counts (v->len) and row bases (gbase), then glue -> layer 0 -> layer 1
// with the weights of `cv` over the utterances' own frames.  series, out0: where the glued series and layer 0's output go (null =
// the handle's work space); cond: layer 1's output, rows of the layout.
int vq_cond_run(vqcpc_vocoder *v, const UttLayout &u, const CondView &cv, const int64_t *idx, const int64_t *spk, int B, int Tc, DevBuf &gbase,
                float *series, float *out0, float *cond, hipStream_t s);
// Rows of the utterances' own frames (gbase[b] + f, f < frames[b]) <-> (B, T2, C).  to_dense: dst (B, T2, C), +0 past an utterance's
// frames; else dst = the ragged rows, and the dense rows past an utterance's frames are not read.
void vq_cond_rows(const float *src, float *dst, const int *frames, const int *gbase, int B, int T2, int C, bool to_dense, hipStream_t s);

// ------------------------------------------------------------------------------------------
// what the gradient entries (vocoder_grad.hip) call in vocoder_host.hip
// ------------------------------------------------------------------------------------------
ArView vq_vocoder_view(const vqcpc_vocoder *v);
// The layouts of ArView from a caller's tensors, enqueued on s into v->gw.  scan: also what only the step kernels read (unit quads,
// W_hh fragments); without it the view serves the conditioning's last product and the Gemb table alone.
int vq_vocoder_relayout(vqcpc_vocoder *v, const float *embedding, const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        const float *fc1_weight, const float *fc1_bias, const float *fc2_weight, const float *fc2_bias, bool scan, ArView *out, hipStream_t s);
// The host-visible conditions of a scoring call (vqcpc_vocoder_nll's), and its scored steps per utterance.
int vq_tf_check(const vqcpc_vocoder *v, int B, int Tc, int L, const int *n_codes, const int *n_audio, std::vector<int> &slen, int *longest);
// The scoring call itself: vqcpc_vocoder_nll's scan and head with the weights of `w` (null = the handle's); hsave (B, L - 1, Hr) or
// null receives h_t of every scored step.
int vq_tf_score(vqcpc_vocoder *v, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc, int L, const int *n_codes,
                const std::vector<int> &slen, int longest, const ArView *w, double *nll_sum, int64_t *n_scored, int64_t *n_correct, float *nll,
                float *hsave, hipStream_t s, const float *cond_in = nullptr);
// Conditioning of a backward call: a call's start (begin_call), then cond (ragged rows), Gcond, the frame counts (v->len) and row
// bases (v->gbase) on the device, and the scored steps in v->nll_len.  cond_in: run_conditioning's.
int vq_tf_condition(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes, const std::vector<int> &slen,
                    const ArView *w, UttLayout &u, hipStream_t s, const float *cond_in = nullptr);
int run_resident(vqcpc_vocoder *v, const CallPlan &cp, int T2, unsigned long long seed, float *wav, int64_t *mulaw, hipStream_t s, const Resume *rs = nullptr);
int run_launch_path(vqcpc_vocoder *v, const CallPlan &cp, const int64_t *inputs, int T2, int Ts, unsigned long long seed, float *wav, int64_t *mulaw, float *logits, hipStream_t s, const Resume *rs = nullptr, const NllCall *nc = nullptr);
