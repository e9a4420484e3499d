// vocoder.hip -- Vocoder.generate / Vocoder.forward on gfx950 (reference call sites
// network_vocoder.py:41-78; the RNN_MS arithmetic is the project's spec of the absent
// third-party `rnnms` package -- see oracle/vqcpc_oracle.c and DESIGN.md).  The prenet's bi-GRU scans run in scan.hip.
//
// Design (DESIGN.md "Decode loop"): every recurrence is WEIGHT-STATIONARY across the chip
// and BATCHED over utterances.  One step = a skinny fp32 GEMM [rows x K] x [K x B]; each
// workgroup owns 16 gate rows (4 hidden units x their gates), streams its own 16 x K weight
// fragment from L2 (fragment-ordered, 16 B per lane), multiplies it with the whole state
// matrix h (K x 16-utterance tiles) on v_mfma_f32_16x16x4_f32, reduces the 4 K-quarters
// through LDS and applies the cell update.  The all-gather of h between steps is the kernel
// boundary; the per-sample kernels are replayed from a hipGraph.  Two launches per sample: fc1, then ONE launch that
// carries fc2 + draw of the previous sample in front of the GRU step (W_hh h does not depend on the drawn sample; the
// candidates reach the GRU's gate waves through in-kernel granules).  A call on a single utterance runs on the
// per-XCD resident decoders instead (ar_xcd.hip / ar_xcm.hip: weights in registers, no launches per sample).
#include "common.h"
#include "ar_shared.h"
#include "ar_xcd.h"
#include "nll.h"
#include <math.h>
#include <stdio.h>
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <vector>

int vq_require_gfx950();
#define TRY(x) do { int rc_ = (x); if (rc_ != VQCPC_OK) return rc_; } while (0)

// Packed GRU fragments: the 12 gate rows of a 4-unit row group WITHOUT the 4 padding rows of the 16-row MFMA
// tile.  Per (rg, K quarter w, super-step s): 48 float4 = [kq 0..3][i 0..11], 768 B = six whole 128-B lines;
//   Wp[(((rg*4 + w)*SW + s)*48 + kq*12 + i] = W[(i>>2)*H + 4*rg + (i&3)][16*(w*SW + s) + 4*kq + 0..3]
// A lane of a padding row (i >= 12) re-reads row 0 of its kq group (an address a live lane also loads, so it
// costs no traffic); its MFMA output rows are never read.  The padded layout streams 12.8 MB for 9.6 MB of W_hh
// and masking lanes does not help (the holes are 64 B inside 128-B lines): VERDICT r1 item 4.
__global__ void build_wfrag12_kernel(const float *__restrict__ W, int ldw, float *__restrict__ Wp, int n_rg, int K, int H) {
    const int SW = K / 64;
    const size_t total = (size_t)n_rg * 4 * SW * 48;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int e = (int)(id % 48);
    size_t r = id / 48;
    const int s = (int)(r % SW); r /= SW;
    const int w = (int)(r % 4);
    const int rg = (int)(r / 4);
    const int kq = e / 12, i = e % 12;
    const int row = (i >> 2) * H + 4 * rg + (i & 3);
    ((float4 *)Wp)[id] = *(const float4 *)(W + (size_t)row * ldw + 16 * (w * SW + s) + 4 * kq);
}
static int build_wfrag12(const float *W, int ldw, int n_rg, int K, int H, float **out) {
    VQ_REQUIRE(K % 64 == 0 && ldw % 4 == 0, "build_wfrag12: K=%d not a multiple of 64", K);
    const size_t n4 = (size_t)n_rg * (K / 16) * 48;
    HIP_TRY(hipMalloc((void **)out, n4 * sizeof(float4)));
    hipLaunchKernelGGL(build_wfrag12_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, 0, W, ldw, *out, n_rg, K, H);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

// ------------------------------------------------------------------------------------------
// Autoregressive sample loop.  Per sample t, three launches (each an all-gather boundary):
//   ar_gru : x_{t-1} = argmax of the fc2 candidates; h_t = GRUCell(Gemb[x_{t-1}] + Gcond, h_{t-1})
//   ar_fc1 : a_t = relu(W1 h_t + b1)
//   ar_fc2 : l_t = W2 a_t + b2; per 16-class row group the Gumbel-max candidate (score, class)
// The categorical draw is an exponential race (argmax_k l_k + g_k, the algorithm of ATen's
// Categorical.sample), which decomposes over class subsets: fc2 is spread over 16 CUs and the
// 16 candidates per utterance are merged by the next step's GRU kernel.
// Per-call quantities live in a device-side ArCall so one captured graph serves every call.
// ------------------------------------------------------------------------------------------
// Continuous batching: a decode SLOT (one MFMA column) runs utterances back to back.  Utterances
// start at replay boundaries, so per (replay, slot) there is at most one: row = its index in this
// call's inputs/outputs (-1 = idle), t0 = global step of its sample 0, len = its samples,
// utt = its sampling-stream id.
struct ArSlot { int row, t0, len; unsigned utt; };

struct ArCall {
    const float *Gcond;        // [sum of the utterances' frames][3Hr] = W_ih[:, de:] cond + b_ih, ragged: utterance `row` starts at row gbase[row]
    const int *gbase;          // [B] first Gcond row of every utterance (prefix sums of the conditioning frame counts)
    const int64_t *inputs;     // teacher forcing (B, Ts) or null
    float *wav;                // (B, Lout) or null
    int64_t *mulaw;            // (B, Lout) or null
    float *logits;             // (B, Ts, n_cls) or null
    const ArSlot *slots;       // [replays][Sp] what every decode slot is doing during each graph replay
    int S, Sp;                 // steps per replay (t_base is a multiple of it), slots (multiple of 16)
    int n_rep;                 // rows of `slots`
    int F, Ts, Lout, max_t, nbt;
    unsigned long long seed;
    int t_base;                // advanced on device after every graph replay
    // teacher-forced scan (Vocoder.forward): only the GRU step runs per sample; h_t of every step of the current
    // chunk is kept, row-major, for the two batched GEMMs (fc1 + ReLU, fc2) that follow the chunk
    float *hall;               // [B][CH][Hr] or null
    int CH, hall_t0;           // chunk length (a multiple of S); first step of the chunk in flight (advanced on device)
    // A chunk of a stream (vqcpc_vocoder_stream_next).  Every utterance resumes at absolute sample s0: its slot rows carry
    // t0 - s0 and s0 + len, so the step kernels see absolute sample indices (Philox counter, conditioning frame) unchanged, and
    // wav / mulaw point s0 - 1 columns in front of a buffer whose column 0 takes sample s0 - 1 again.  ar_next_row_kernel
    // seeds a resumed slot (h_in in its state column, x_in as every candidate of its first step) and copies a finished one's
    // final state to h_out.  All null / 0 for a one-shot call.
    const float *h_in;         // [B][Hr] or null: fresh start (s0 == 0)
    const int *x_in;           // [B]
    float *h_out;              // [B][Hr] or null
    int s0;
    // A scoring call (vqcpc_vocoder_nll): every utterance starts at step 0 in its own slot, so `slots` holds ONE row for all replays
    // and a slot goes idle (row -1, what the full table says) once its utterance's steps are done: the table does not grow with
    // the length of the call.  0 for every other call.
    int one_row;
};

// Timeline stamps of workgroup (0, 0) (100 MHz wall clock) for tools/decode_timeline.py: compiled in only
// with -DVQCPC_AR_STAMPS (a debug build under build/stamps/, never the shipped library).
#ifdef VQCPC_AR_STAMPS
__device__ unsigned long long g_ar_stamps[160 * 3 * 6];
#define AR_STAMP(cond, kern, i) do { if ((cond) && blockIdx.x == 1 && blockIdx.y == 0 && t_local < 160) \
        g_ar_stamps[(t_local * 3 + (kern)) * 6 + (i)] = wall_clock64(); } while (0)
extern "C" int vqcpc_debug_ar_stamps(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ar_stamps), sizeof(g_ar_stamps)) == hipSuccess ? 0 : -1;
}
#else
#define AR_STAMP(cond, kern, i) do { } while (0)
#endif

struct ArModel {               // constant per handle (baked into the captured graph)
    // Cell-update operands in "unit quads": for row group rg (4 hidden units) and unit u, ONE float4 = (r, z, n, 0).
    // A gate wave's lane then needs one 16-byte load per table instead of three 4-byte loads H apart, and the 16
    // slots of a tile read 1 KiB contiguous (gcur4) -- the [3H] layouts cost a whole 128-B line per 16 bytes used.
    const float4 *bh4;         // [Hr/4][4]            b_hh
    const float4 *Gemb4;       // [n_cls][Hr/4][4]     emb . W_ih[:, :de]^T
    const float *Gemb;         // [n_cls][3Hr] (unused by the step kernels; kept for tools)
    const float *Wf_hh12;      // W_hh in packed 12-row groups (ar_gru_kernel: no padding rows streamed)
    const float *Wf_hh16;      // W_hh in gate-major 16-row tiles (large-batch kernel: no padding rows)
    float4 *gcur4;             // [Hr/4][Sp][4] the Gcond row every slot uses during the replay in flight (gc_replay), unit quads
    int gc_replay;             // 1: upsample % steps_per_graph == 0, so a slot stays on one conditioning frame per replay
    int live_last;             // decode slots in use in the last tile (1..16): lanes of dead columns re-read column 0
    int lead6;                 // ar_gru_kernel requests fragments 6 super-steps ahead instead of 3 (see there)
    const float *Wf_fc1, *b_fc1, *Wf_fc2, *b_fc2, *mulaw_tab;
    const float *Wf_fc1h;      // fc1 in 8-row groups (few tiles in flight: twice the workgroups, half the weight bytes each)
    float *hbuf;               // [2][nbt][Hr*16]
    float *a1;                 // [nbt][Hf*16]
    float *cand_s;             // [Bpad][n_cls / 16] best score of each 16-class row group
    int *cand_k;               // [Bpad][n_cls / 16] its class
    ArSlot *cur;               // [Sp] the slot row of the replay in flight (copied from ArCall::slots between
                               // replays): a fixed address, so the step kernels read it without first waiting for ArCall
    // fused fc2 || GRU launch: candidates as 8-byte granules {(tag << 10 | class), score}, tag = step + 1, one 128-B
    // line per producing workgroup: [tile][16 row groups][16 slots]
    unsigned long long *candg;
    unsigned *abort_dev;       // set when a candidate wait timed out: later steps stop waiting
    unsigned *abort_host;      // the same, host-mapped: the next call on the handle reports it
    unsigned timeout_ticks;    // bound of the in-kernel candidate waits (100 MHz ticks)
    int dbg_drop_t;            // tests: the fc2 team of row group 3, tile 0 skips its candidate publish at this step (-1: never)
    int fused;                 // 0: three launches per sample; 1: fc2 + draw ride in the GRU launch (candidates in candg)
    int Hr, Hf, n_cls, upsample;
};


// The 16 row-group candidates of a decode slot (row groups are in class order): request, then
// first-argmax, split so that the request can be issued early.  (A 4-lanes-per-slot variant that
// combined by __shfl_xor made the wave-specialised kernel 5x slower on gfx950 -- measured, dropped.)
struct Cand16 { float4 s[4]; int4 k[4]; };
__device__ __forceinline__ void load_candidates16(const ArModel &m, int sg, int c0, Cand16 &cd) {
    const int nrg = m.n_cls >> 4;
    const float4 *ps = (const float4 *)(m.cand_s + (size_t)sg * nrg + c0);
    const int4 *pk = (const int4 *)(m.cand_k + (size_t)sg * nrg + c0);
#pragma unroll
    for (int q = 0; q < 4; ++q) { cd.s[q] = ps[q]; cd.k[q] = pk[q]; }
}
__device__ __forceinline__ void merge16(const Cand16 &cd, float &best, int &k) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (cd.s[q].x > best) { best = cd.s[q].x; k = cd.k[q].x; }
        if (cd.s[q].y > best) { best = cd.s[q].y; k = cd.k[q].y; }
        if (cd.s[q].z > best) { best = cd.s[q].z; k = cd.k[q].z; }
        if (cd.s[q].w > best) { best = cd.s[q].w; k = cd.k[q].w; }
    }
}
// all n_cls / 16 candidates of the slot: the first 16 were requested early (cd), further chunks (n_cls > 256) follow
__device__ __forceinline__ int merge_candidates(const ArModel &m, int sg, const Cand16 &cd) {
    float best = -INFINITY;
    int k = 0;
    merge16(cd, best, k);
    for (int c0 = 16; c0 < (m.n_cls >> 4); c0 += 16) {
        Cand16 more;
        load_candidates16(m, sg, c0, more);
        merge16(more, best, k);
    }
    return k;
}
// The same from the granules of the fused launch: wait until the slot's candidates carry step t's tag (from the fc2 workgroups
// of THIS launch, or, at the first step of a replay, of the trailing fc2 launch of the previous one), 16 row groups at a
// time, and take the first argmax.  Bounded; a timeout raises the abort words and returns class 0.
#define CAND_TAG_BITS 22
__device__ __forceinline__ int wait_candidates(const ArModel &m, int sg, int t, bool need, int lane) {
    const int nrg = m.n_cls >> 4;
    const unsigned tag = (unsigned)t & ((1u << CAND_TAG_BITS) - 1u);
    const u64 t0 = __builtin_amdgcn_s_memrealtime();
    bool gave_up = __hip_atomic_load(m.abort_dev, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
    float best = -INFINITY;
    int xf = 0;
    for (int c0 = 0; c0 < nrg; c0 += 16) {
        const u64 *cg = m.candg + ((size_t)(sg >> 4) * nrg + c0) * 16 + (sg & 15);
        u64 gv[16];
        for (unsigned spins = 0; !gave_up; ++spins) {
            bool ok = true;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                gv[q] = ps_load(cg + q * 16);
                ok &= (unsigned)(gv[q] >> 42) == tag;
            }
            if (__all(ok || !need)) break;
            if ((spins & 255) == 255 && __builtin_amdgcn_s_memrealtime() - t0 > (u64)m.timeout_ticks) {      // default 0.25 s
                if (lane == 0) {
                    __hip_atomic_store(m.abort_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(m.abort_host, STATUS_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
                gave_up = true;
            }
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {                               // row groups are in class order: first argmax
            const float sq = __uint_as_float((unsigned)gv[q]);
            if (!gave_up && sq > best) { best = sq; xf = (int)((gv[q] >> 32) & 1023u); }
        }
    }
    return xf;
}

// `live` = columns (decode slots) of tile bt in use: a lane of a dead column re-reads column 0 of its k group
// (same address as a live lane, so it costs no traffic) instead of streaming padding -- at one utterance
// that is 15/16 of the state bytes.
template <int SW>
__device__ __forceinline__ void load_hfrag(const float *hL, int K, int bt, int wave, int lane, int live, float4 (&hv)[SW]) {
    const int hl = (lane & 15) < live ? lane : (lane & 48);
    const float4 *hp = (const float4 *)hL + ((size_t)bt * (K >> 2)) * 16 + (size_t)wave * SW * 64 + hl;
#pragma unroll
    for (int s = 0; s < SW; ++s) hv[s] = hp[s * 64];
}
template <int SW>
__device__ __forceinline__ f32x4 mfma_frag(const float4 (&wf)[SW], const float4 (&hv)[SW]) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < SW; ++s) {
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].x, hv[s].x, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].y, hv[s].y, a1, 0, 0, 0);
        a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].z, hv[s].z, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].w, hv[s].w, a1, 0, 0, 0);
    }
    return a0 + a1;
}

// Scheduling notes (checked in the .s and with tools/decode_timeline.py): hipcc otherwise sinks each fragment
// load down to its MFMA (load 2, wait, 4 MFMA, ...), hoists the call-record load and the exit branch above
// everything, and falls back to vmcnt(0) around divergent branches.  So: sched_barrier(0) pins the request
// order; there is no early return (stores are predicated); the ping-pong parity of the state buffers comes
// from the launch index (steps_per_graph is even, t_base a multiple of it); and the GRU kernel is
// WAVE-SPECIALISED: the first NB waves (one per utterance tile in flight) chase the dependent loads of the
// cell update (candidates -> x -> Gemb row; slot record, Gcond row, biases and old state at fixed addresses),
// the next four run a branch-free load -> MFMA -> LDS stream over the four K quarters.
// FUSED = 1: ONE launch carries fc2 + draw of step t-1 AND the GRU step t.  W_hh h_{t-1} -- the heavy part of the GRU step
// -- does not depend on x_{t-1}, so it runs while the fc2 workgroups (the first n_fc2 blocks of the grid, so that they
// are dispatched first) compute the candidates; only the gate waves wait, on 16 candidate granules per decode slot
// ({tag = step, class, score}, written with agent-scope atomics, one 128-B line per producing workgroup: the data is the
// flag, MI355X_MICROARCH.md "Valid forms" R2).  This takes the fc2 -> GRU kernel boundary (1.5 us) and fc2's whole body
// (1.6 us after a cold start) off the critical path of a sample step.  Every wait is wall-clock bounded; a timeout sets
// an abort word that makes every later wait of the call return at once, and the host reports it.
// FUSED = 0 (teacher-forced scan, eager timing, > 4 tiles): candidates come from the previous launch's plain arrays.
// fc2 over one 16-class row group + its Gumbel-max candidate per utterance, for local step `ts` (Hf = 256: SW = 4).
// Used by ar_fc2_kernel (plain candidate arrays) and by the fused launch (granules).  All threads of the workgroup must
// call it (two barriers); threads >= 256 only take part in those.
// Bounded wait shared by the in-kernel hand-offs: true once `deadline` has passed (the abort words are then set).
__device__ __forceinline__ bool handoff_timed_out(const ArModel &m, u64 t0, unsigned spins, int lane) {
    if ((spins & 255) != 255 || __builtin_amdgcn_s_memrealtime() - t0 <= (u64)m.timeout_ticks) return false;      // default 0.25 s
    if (lane == 0) {
        __hip_atomic_store(m.abort_dev, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(m.abort_host, STATUS_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return true;
}

// fc1 + ReLU over ROWS rows x one utterance tile for local step `ts` (the GRU of that step has written its state).
// `tid` / `worker` as in fc2_body.
template <int SW, int ROWS>
__device__ __forceinline__ void fc1_body(const ArModel &m, const ArCall *__restrict__ cp, int ts, int rg, int bt, int nbt,
                                         float (*red)[16][17], int tid, bool worker) {
    const int lane = tid & 63, wave = (tid >> 6) & 3;
    const int wv = worker ? wave : 0;
    if (!worker) { rg = 0; bt = 0; }
    const float *h = m.hbuf + (size_t)((ts + 1) & 1) * nbt * m.Hr * 16;
    float4 wf[SW], hv[SW];
    load_wfrag<SW>(ROWS == 8 ? m.Wf_fc1h : m.Wf_fc1, rg, 4, wv, (lane & 15) < ROWS ? lane : (lane & 48), wf);
    load_hfrag<SW>(h, m.Hr, bt, wv, lane, bt == nbt - 1 ? m.live_last : 16, hv);
    const bool own = ((tid >> 4) & 15) < ROWS;
    const int row = own ? ROWS * rg + ((tid >> 4) & 15) : 0;
    const float bias = m.b_fc1[row];
    __builtin_amdgcn_sched_barrier(0);
    const ArCall c = *cp;
    const bool valid = ts >= 0 && c.t_base + ts < c.max_t;
    const f32x4 acc = mfma_frag<SW>(wf, hv);
    if (worker) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) * 4 + r][lane & 15] = acc[r];
    }
    __syncthreads();
    if (worker && valid && own) {
        const int rr = (tid >> 4) & 15, bb = tid & 15;
        float v = ((red[0][rr][bb] + red[1][rr][bb]) + red[2][rr][bb]) + red[3][rr][bb];
        v += bias;
        v = v > 0.f ? v : 0.f;
        const size_t at = hl_index(m.Hf, bt * 16 + bb, row);
        m.a1[at] = v;
    }
}

// `tid` = index inside the 256-thread team that computes (rg, bt); `worker` = false for threads that only keep the
// workgroup's barriers company (the tail of a 320/384-thread block, teams past the last (rg, bt) of a 1024-thread block).
template <int GRANULES>
__device__ __forceinline__ void fc2_body(const ArModel &m, const ArCall *__restrict__ cp, int ts, int rg, int bt, int nbt,
                                         float (*red)[16][17], float (*sc)[17], int tid, bool worker) {
    const int lane = tid & 63, wave = (tid >> 6) & 3;
    const int wv = worker ? wave : 0;
    if (!worker) { rg = 0; bt = 0; }
    // K = size_h_fc = 64 swf: this wave's quarter is swf super-steps, taken four at a time (256: once)
    const int swf = m.Hf >> 6, nrg = m.n_cls >> 4;
    const int live_cols = bt == nbt - 1 ? m.live_last : 16;
    const float4 *wfp = (const float4 *)m.Wf_fc2 + ((size_t)rg * (m.Hf >> 4) + (size_t)wv * swf) * 64 + lane;
    const float4 *hfp = (const float4 *)m.a1 + ((size_t)bt * (m.Hf >> 2)) * 16 + (size_t)wv * swf * 64 + ((lane & 15) < live_cols ? lane : (lane & 48));
    float4 wf[4], hv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { wf[q] = wfp[q * 64]; hv[q] = hfp[q * 64]; }
    const int rr = (tid >> 4) & 15, bb = tid & 15, cls = 16 * rg + rr, bg = bt * 16 + bb;      // bg = decode slot
    const float bias = m.b_fc2[cls];
    __builtin_amdgcn_sched_barrier(0);
    const ArCall c = *cp;
    const int t = c.t_base + ts;
    const ArSlot sl = m.cur[bg];
    const int lt = t - sl.t0;
    // noise of (class, utterance, sample) while the loads fly
    const unsigned w = philox_word((unsigned)lt, sl.utt, (unsigned)(cls >> 2), (unsigned)c.seed,
                                   (unsigned)(c.seed >> 32), cls & 3);
    // 23 random bits + 0.5: every value is exact in fp32 and strictly inside (0, 1) -- a 24-bit form rounds to 1.0f
    // at w >> 8 == 0xFFFFFF, i.e. +inf noise that wins whatever the logit is
    const float g = gumbel_from_word(w);
    const bool live = ts >= 0 && t < c.max_t && sl.row >= 0 && lt >= 0 && lt < sl.len;
    __builtin_amdgcn_sched_barrier(0);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0;;) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[q].x, hv[q].x, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[q].y, hv[q].y, a1, 0, 0, 0);
            a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[q].z, hv[q].z, a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[q].w, hv[q].w, a1, 0, 0, 0);
        }
        s0 += 4;
        if (s0 >= swf) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) { wf[q] = wfp[(s0 + q) * 64]; hv[q] = hfp[(s0 + q) * 64]; }
    }
    const f32x4 acc = a0 + a1;
    if (worker) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) * 4 + r][lane & 15] = acc[r];
    }
    __syncthreads();
    if (worker) {
        float v = ((red[0][rr][bb] + red[1][rr][bb]) + red[2][rr][bb]) + red[3][rr][bb];
        v += bias;
        if (c.logits && live) c.logits[((size_t)sl.row * c.Ts + lt) * m.n_cls + cls] = v;
        sc[rr][bb] = v + g;
    }
    __syncthreads();
    if (worker && tid < 16 && live) {
        float best = sc[0][bb];
        int k = 0;
#pragma unroll
        for (int r = 1; r < 16; ++r)
            if (sc[r][bb] > best) { best = sc[r][bb]; k = r; }
        if (GRANULES) {
            const unsigned tag = (unsigned)(t + 1) & ((1u << CAND_TAG_BITS) - 1u);
            if (!(m.dbg_drop_t >= 0 && t == m.dbg_drop_t && rg == 3 && bt == 0))
            ps_store(m.candg + ((size_t)(bt * nrg + rg) * 16 + bb), ((u64)((tag << 10) | (unsigned)(16 * rg + k)) << 32) | __float_as_uint(best));
        } else {
            m.cand_s[(size_t)bg * nrg + rg] = best;
            m.cand_k[(size_t)bg * nrg + rg] = 16 * rg + k;
        }
    }
}

template <int SW, int NB, int LEADP, int FUSED>      // NB = utterance tiles (of 16) in flight per pass: 1 or 2
__global__ __launch_bounds__(64 * (4 + NB)) void ar_gru_kernel(ArModel m, const ArCall *__restrict__ cp, int t_local, int nbt,
                                                               int n_fc2) {
    __shared__ float red[NB][4][16][17];
    __shared__ __attribute__((aligned(16))) float mt[256];            // mu-law decode table (row group 0 emits the samples)
    __shared__ float sc[16][17];                                       // FUSED: scores of an fc2 workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, Hr = m.Hr;
    int rg = blockIdx.x, pass = blockIdx.y;
    if (FUSED) {
        if ((int)blockIdx.x < n_fc2) {                                 // fc2 + draw of the PREVIOUS step
            const int fb = blockIdx.x, nrg = m.n_cls >> 4;
            fc2_body<1>(m, cp, t_local - 1, fb % nrg, fb / nrg, nbt, red[0], sc, tid, tid < 256);
            return;
        }
        const int gb = blockIdx.x - n_fc2;
        rg = gb % (Hr >> 2);
        pass = gb / (Hr >> 2);
    }
    const size_t hsz = (size_t)nbt * Hr * 16;
    const float *hin = m.hbuf + (size_t)(t_local & 1) * hsz;
    float *hout = m.hbuf + (size_t)((t_local + 1) & 1) * hsz;
    // Waves 0..NB-1 chase the cell update's operands, waves NB..NB+3 run the MFMAs: the memory pipeline serves
    // the oldest wave first, so the short dependent chain must live in the low wave slots (with the roles the
    // other way round its requests arrived after the whole fragment stream: tools/decode_timeline.py).
    const bool mfma_wave = wave >= NB;               // wave-uniform
    const int g = wave, kw = wave - NB;              // gate wave index = tile slot; MFMA wave's K quarter
    const int u = lane >> 4, b = lane & 15, unit = 4 * rg + u;
    AR_STAMP(tid == 64 * NB, 0, 0);

    // one pass of NB tiles per workgroup: grid.y = passes, so co-resident workgroups overlap one
    // pass's fragment loads with another's MFMAs when many utterances are in flight
    {
        const int bt0 = pass * NB;
        bool active = false, first = false;
        float ge0 = 0.f, ge1 = 0.f, ge2 = 0.f, gc0 = 0.f, gc1 = 0.f, gc2 = 0.f, bh0 = 0.f, bh1 = 0.f, bh2 = 0.f, hold = 0.f;
        size_t hi = 0;
        int xraw = 0;
        bool emit = false;
        float *wavp = nullptr, *hallp = nullptr;
        int64_t *mulp = nullptr;
        if (mfma_wave) {
            // Fragments are requested LEADP super-steps ahead of their MFMAs, not all at once.  Measured
            // (bench.py, us per sample step): all 14 at once 12.76 at 32 utterances / 22.7 at 112; 6 ahead
            // 12.17 / 23.2 and 14.5 at 64; 3 ahead 12.13 / 20.75 but 15.6 at 64 (two 2-tile groups on two
            // streams want more in flight).  launch_ar_steps picks 6 for that case, 3 otherwise.
            constexpr int LEAD = SW < LEADP ? SW : LEADP;
            float4 wf[SW], hv[NB][SW];
            const float4 *wp = (const float4 *)m.Wf_hh12 + ((size_t)(rg * 4 + kw) * SW) * 48 + (lane >> 4) * 12 +
                               ((lane & 15) < 12 ? (lane & 15) : 0);          // packed rows; padding lanes alias row 0
            const float4 *hp[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int bt = bt0 + q < nbt ? bt0 + q : nbt - 1;        // clamped: no branch around loads
                const int live = bt == nbt - 1 ? m.live_last : 16;       // dead columns re-read column 0 (load_hfrag)
                const int hl = (lane & 15) < live ? lane : (lane & 48);
                hp[q] = (const float4 *)hin + ((size_t)bt * (Hr >> 2)) * 16 + (size_t)kw * SW * 64 + hl;
            }
#pragma unroll
            for (int s = 0; s < LEAD; ++s) {
                wf[s] = wp[s * 48];
#pragma unroll
                for (int q = 0; q < NB; ++q) hv[q][s] = hp[q][s * 64];
            }
            __builtin_amdgcn_sched_barrier(0);
            f32x4 a0[NB], a1[NB];
#pragma unroll
            for (int q = 0; q < NB; ++q) { a0[q] = f32x4{0.f, 0.f, 0.f, 0.f}; a1[q] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                if (s + LEAD < SW) {
                    wf[s + LEAD] = wp[(s + LEAD) * 48];
#pragma unroll
                    for (int q = 0; q < NB; ++q) hv[q][s + LEAD] = hp[q][(s + LEAD) * 64];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = 0; q < NB; ++q) {                           // same chains as mfma_frag: (x, z) -> a0, (y, w) -> a1
                    a0[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].x, hv[q][s].x, a0[q], 0, 0, 0);
                    a1[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].y, hv[q][s].y, a1[q], 0, 0, 0);
                    a0[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].z, hv[q][s].z, a0[q], 0, 0, 0);
                    a1[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].w, hv[q][s].w, a1[q], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const f32x4 acc = a0[q] + a1[q];
#pragma unroll
                for (int r = 0; r < 4; ++r) red[q][kw][(lane >> 4) * 4 + r][lane & 15] = acc[r];
            }
            AR_STAMP(tid == 64 * NB, 0, 1);
        } else {
            const int bt = bt0 + g;
            const int sg = (bt < nbt ? bt : nbt - 1) * 16 + b;           // decode slot
            // The cell update's operands form a dependent chain (candidates -> x -> Gemb row).  Everything that
            // has a fixed address is requested up front -- candidates, slot record, call record, biases, old
            // state, the slot's Gcond row of this replay (gcur) -- so that only the Gemb row is a second level.
            Cand16 cd;
            if (!FUSED) load_candidates16(m, sg, 0, cd);
            const ArSlot sl = m.cur[sg];
            const ArCall c = *cp;
            const float4 bq = m.bh4[rg * 4 + u];
            hi = hl_index(Hr, sg, unit);
            const float hprev = hin[hi];
            const float4 gq = m.gcur4[((size_t)rg * (nbt * 16) + sg) * 4 + u];     // no branch around loads: gcur4 always exists
            bh0 = bq.x; bh1 = bq.y; bh2 = bq.z;
            gc0 = gq.x; gc1 = gq.y; gc2 = gq.z;
            float4 mtl = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rg == 0 && wave == 0) mtl = ((const float4 *)m.mulaw_tab)[4 * lane < m.n_cls ? lane : 0];
            __builtin_amdgcn_sched_barrier(0);
            const int t = c.t_base + t_local;
            const int lt = t - sl.t0;                                    // sample index inside the utterance
            active = bt < nbt && t < c.max_t && sl.row >= 0 && lt < sl.len;
            AR_STAMP(tid == 0 && (active || !active), 0, 4);
            first = lt == 0;
            int xf = 0;
            if (FUSED) xf = wait_candidates(m, sg, t, active && !first, lane);
            if (active) {
                int x;
                if (c.inputs) x = (int)c.inputs[(size_t)sl.row * c.Ts + lt];
                else if (first) x = m.n_cls / 2;
                else {
                    if (!FUSED) x = merge_candidates(m, sg, cd);
                    else x = xf;
                    emit = rg == 0 && u == 0;                   // sample lt-1 goes out after the barrier
                    if (emit) { wavp = c.wav ? c.wav + (size_t)sl.row * c.Lout + lt - 1 : nullptr;
                                mulp = c.mulaw ? c.mulaw + (size_t)sl.row * c.Lout + lt - 1 : nullptr; xraw = x; }
                }
                x = x < 0 ? 0 : (x >= m.n_cls ? m.n_cls - 1 : x);
                const float4 eq = m.Gemb4[((size_t)x * (Hr >> 2) + rg) * 4 + u];
                ge0 = eq.x; ge1 = eq.y; ge2 = eq.z;
                if (!m.gc_replay) {
                    const float *gc = c.Gcond + ((size_t)c.gbase[sl.row] + lt / m.upsample) * 3 * Hr + unit;
                    gc0 = gc[0]; gc1 = gc[Hr]; gc2 = gc[2 * Hr];
                }
                hold = first ? 0.f : hprev;                     // a new utterance starts from h = 0
                if (c.hall) hallp = c.hall + ((size_t)sl.row * c.CH + (lt - c.hall_t0)) * Hr + unit;
            }
            if (rg == 0 && wave == 0) ((float4 *)mt)[lane] = mtl;
            AR_STAMP(tid == 0, 0, 2);
        }
        __syncthreads();
        // cell update (PyTorch GRUCell equations, gate order r, z, n), K quarters summed in fixed order
        if (emit) {                                  // network_vocoder.py:78 output: the sample the candidates decided
            if (wavp) *wavp = m.n_cls <= 256 ? mt[xraw] : m.mulaw_tab[xraw];
            if (mulp) *mulp = xraw;
        }
        if (active) {
            // the slot's previous occupant left its state in the MFMA operand: W_hh . 0 = 0 on a first step
            const float gr = first ? 0.f : ((red[g][0][u][b] + red[g][1][u][b]) + red[g][2][u][b]) + red[g][3][u][b];
            const float gz = first ? 0.f : ((red[g][0][4 + u][b] + red[g][1][4 + u][b]) + red[g][2][4 + u][b]) + red[g][3][4 + u][b];
            const float gn = first ? 0.f : ((red[g][0][8 + u][b] + red[g][1][8 + u][b]) + red[g][2][8 + u][b]) + red[g][3][8 + u][b];
            const float r = gate_sigmoid((ge0 + gc0) + (gr + bh0));
            const float z = gate_sigmoid((ge1 + gc1) + (gz + bh1));
            const float n = gate_tanh((ge2 + gc2) + r * (gn + bh2));
            const float hn = (1.0f - z) * n + z * hold;
            hout[hi] = hn;
            if (hallp) *hallp = hn;
        }
        AR_STAMP(tid == 0, 0, 3);
    }
}

// Large-batch GRU step (>= 8 utterance tiles in flight).  The wave-specialised kernel above re-reads
// the state tile once per row group; at many tiles the per-CU L2 read rate (~65 GB/s) is the limit
// (DESIGN "what bounds K7a"), and behind it the MFMA pipe: 16 waves x 112 MFMAs = 6.8 us per SIMD when every
// 16-row MFMA tile carries 4 padding rows.  Here one 1024-thread workgroup owns 16 hidden units and TWO tiles:
//  * the two state tiles (2 x 57 KB) are staged ONCE in LDS and shared by all MFMA waves;
//  * the 48 gate rows are three FULL 16-row tiles (r, z, n of the 16 units: fragment layout Wf_hh16), so 12
//    waves (gate x K quarter) do the MFMAs -- 25 % fewer MFMAs and weight bytes (172 KB) than padded 12-row groups;
//  * the 4 oldest waves do nothing but the cell update's operand chain and the update itself (2 units per lane).
// Per-row arithmetic is unchanged (same K quarters, same accumulator pairs): bit-identical to ar_gru_kernel.
// Grid = (Hr/16, ceil(nbt/2)).
// staging of one state tile by all 1024 threads: request / store halves (the barrier is the caller's)
__device__ __forceinline__ void big_stage_load(const float4 *src, int t4, int tid, bool on, float4 (&st)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 1024 * j;
        st[j] = (on && i < t4) ? src[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
__device__ __forceinline__ void big_stage_store(float4 *dst, int t4, int tid, const float4 (&st)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 1024 * j;
        if (i < t4) dst[i] = st[j];
    }
}

// FUSED = 1: as in ar_gru_kernel, the first n_fc2 blocks of the launch run fc2 + draw of the PREVIOUS step and the
// cell-update waves pick the candidates up through granules -- after the staging barriers, while the MFMA waves compute.
template <int SW, int FUSED>
__global__ __launch_bounds__(1024) void ar_gru_big_kernel(ArModel m, const ArCall *__restrict__ cp, int t_local, int nbt, int n_fc2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int Hr = m.Hr;
    float4 *hs = (float4 *)smem;                                             // [2][Hr*4] float4 = two state tiles
    float (*red)[3][4][16][17] = (float (*)[3][4][16][17])(smem + (size_t)2 * Hr * 16 * sizeof(float));   // [tile][gate][kq][unit][slot]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int blk = blockIdx.x, passy = blockIdx.y;
    if (FUSED) {
        // four 256-thread teams per workgroup, one (row group, tile) each: 4 nbt fc2 workgroups in front of the GRU ones
        const int team = tid >> 8;
        char *base = smem + (size_t)team * (5 * 16 * 17 * sizeof(float));
        if ((int)blockIdx.x < n_fc2) {
            const int pair = blockIdx.x * 4 + team;
            const int nrg = m.n_cls >> 4;
            fc2_body<1>(m, cp, t_local - 1, pair % nrg, pair / nrg, nbt, (float (*)[16][17])base,
                        (float (*)[17])(base + 4 * 16 * 17 * sizeof(float)), tid & 255, pair < nrg * nbt);
            return;
        }
        const int gb = blockIdx.x - n_fc2;
        blk = gb % (Hr >> 4);
        passy = gb / (Hr >> 4);
    }
    const int bt0 = passy * 2, nb = nbt - bt0 < 2 ? nbt - bt0 : 2;
    const size_t hsz = (size_t)nbt * Hr * 16;
    const float *hin = m.hbuf + (size_t)(t_local & 1) * hsz;
    float *hout = m.hbuf + (size_t)((t_local + 1) & 1) * hsz;
    const int t4 = Hr * 4;                                                   // float4 per state tile
    const float4 *src = (const float4 *)hin + (size_t)bt0 * t4;
    float4 st[4];

    // The two roles are separate code paths (their registers never coexist); both pass the same three barriers.
    if (wave < 4) {
        // ---- cell-update waves: tile q, units 16 blk + 8 uh + 4 p + u (p = 0, 1), slot b
        const int q = wave & 1, uh = wave >> 1, u = lane >> 4, b = lane & 15;
        const int gbt = bt0 + q;
        const int sg = (gbt < nbt ? gbt : nbt - 1) * 16 + b;
        float ge[2][3] = {}, gc[2][3], bh[2][3], hold[2] = {0.f, 0.f}, hprev[2];
        size_t hi[2];
        float *hallp = nullptr;
        // first level of the operand chain: everything with a fixed address (as in ar_gru_kernel)
        Cand16 cd;
        if (!FUSED) load_candidates16(m, sg, 0, cd);
        const ArSlot sl = m.cur[sg];
        const ArCall c = *cp;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int unit = 16 * blk + 8 * uh + 4 * p + u, rgq = 4 * blk + 2 * uh + p;
            const float4 bq = m.bh4[rgq * 4 + u];
            const float4 gq = m.gcur4[((size_t)rgq * (nbt * 16) + sg) * 4 + u];
            bh[p][0] = bq.x; bh[p][1] = bq.y; bh[p][2] = bq.z;
            gc[p][0] = gq.x; gc[p][1] = gq.y; gc[p][2] = gq.z;
            hi[p] = hl_index(Hr, sg, unit);
            hprev[p] = hin[hi[p]];
        }
        __builtin_amdgcn_sched_barrier(0);
        big_stage_load(src, t4, tid, true, st);
        __builtin_amdgcn_sched_barrier(0);
        // second level: x picks the Gemb rows
        const int t = c.t_base + t_local;
        const int lt = t - sl.t0;
        const bool active = gbt < nbt && t < c.max_t && sl.row >= 0 && lt < sl.len;
        const bool first = lt == 0;
        int xf = 0;
        if (FUSED) {                                             // this wave's share of the staging first: the MFMA waves
            big_stage_store(hs, t4, tid, st);                    // must not wait behind the candidate hand-off
            __syncthreads();
            big_stage_load(src + t4, t4, tid, nb > 1, st);
            big_stage_store(hs + t4, t4, tid, st);
            __syncthreads();
            xf = wait_candidates(m, sg, t, active && !first, lane);
        }
        if (active) {
            int x;
            if (c.inputs) x = (int)c.inputs[(size_t)sl.row * c.Ts + lt];
            else if (first) x = m.n_cls / 2;
            else {
                x = FUSED ? xf : merge_candidates(m, sg, cd);
                if (blk == 0 && uh == 0 && u == 0) {             // emit sample lt-1 (network_vocoder.py:78 output)
                    if (c.wav) c.wav[(size_t)sl.row * c.Lout + lt - 1] = m.mulaw_tab[x];
                    if (c.mulaw) c.mulaw[(size_t)sl.row * c.Lout + lt - 1] = x;
                }
            }
            x = x < 0 ? 0 : (x >= m.n_cls ? m.n_cls - 1 : x);
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int unit = 16 * blk + 8 * uh + 4 * p + u, rgq = 4 * blk + 2 * uh + p;
                const float4 eq = m.Gemb4[((size_t)x * (Hr >> 2) + rgq) * 4 + u];
                ge[p][0] = eq.x; ge[p][1] = eq.y; ge[p][2] = eq.z;
                if (!m.gc_replay) {
                    const float *pg = c.Gcond + ((size_t)c.gbase[sl.row] + lt / m.upsample) * 3 * Hr + unit;
                    gc[p][0] = pg[0]; gc[p][1] = pg[Hr]; gc[p][2] = pg[2 * Hr];
                }
                hold[p] = first ? 0.f : hprev[p];
            }
            if (c.hall) hallp = c.hall + ((size_t)sl.row * c.CH + (lt - c.hall_t0)) * Hr + 16 * blk + 8 * uh + u;
        }
        if (!FUSED) {
            big_stage_store(hs, t4, tid, st);
            __syncthreads();
            big_stage_load(src + t4, t4, tid, nb > 1, st);
            big_stage_store(hs + t4, t4, tid, st);
            __syncthreads();
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int ul = 8 * uh + 4 * p + u;
                const float gr = first ? 0.f : ((red[q][0][0][ul][b] + red[q][0][1][ul][b]) + red[q][0][2][ul][b]) + red[q][0][3][ul][b];
                const float gz = first ? 0.f : ((red[q][1][0][ul][b] + red[q][1][1][ul][b]) + red[q][1][2][ul][b]) + red[q][1][3][ul][b];
                const float gn = first ? 0.f : ((red[q][2][0][ul][b] + red[q][2][1][ul][b]) + red[q][2][2][ul][b]) + red[q][2][3][ul][b];
                const float rr = gate_sigmoid((ge[p][0] + gc[p][0]) + (gr + bh[p][0]));
                const float z = gate_sigmoid((ge[p][1] + gc[p][1]) + (gz + bh[p][1]));
                const float n = gate_tanh((ge[p][2] + gc[p][2]) + rr * (gn + bh[p][2]));
                const float hn = (1.0f - z) * n + z * hold[p];
                hout[hi[p]] = hn;
                if (hallp) hallp[4 * p] = hn;
            }
        }
    } else {
        // ---- MFMA waves: gate tile gt (r, z, n of the 16 units), K quarter kq
        const int gt = (wave - 4) >> 2, kq = (wave - 4) & 3;
        big_stage_load(src, t4, tid, true, st);              // state before weights: vmcnt retires in order, so the
        float4 wf[SW];                                       // staging barrier waits for the state only
        load_wfrag<SW>(m.Wf_hh16, blk * 3 + gt, 4, kq, lane, wf);
        __builtin_amdgcn_sched_barrier(0);
        big_stage_store(hs, t4, tid, st);
        __syncthreads();
        big_stage_load(src + t4, t4, tid, nb > 1, st);       // tile 1 streams in underneath tile 0's MFMAs
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
            if (qq == 1) {
                big_stage_store(hs + t4, t4, tid, st);
                __syncthreads();
            }
            const float4 *hp = hs + (size_t)qq * t4 + (size_t)kq * SW * 64 + lane;
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < SW; ++s) {
                const float4 hv = hp[s * 64];
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].x, hv.x, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].y, hv.y, a1, 0, 0, 0);
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].z, hv.z, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[s].w, hv.w, a1, 0, 0, 0);
            }
            const f32x4 acc = a0 + a1;
#pragma unroll
            for (int k = 0; k < 4; ++k) red[qq][gt][kq][(lane >> 4) * 4 + k][lane & 15] = acc[k];
        }
        __syncthreads();
    }
}

// fc1 / fc2: grid = (row groups, utterance tiles).  fc1 is bound by the bytes one CU pulls (57 KB of weights +
// 57 KB of state per workgroup at ~70 GB/s): with ROWS = 8 a workgroup owns 8 output rows -- the other 8 rows of
// the MFMA tile are dead lanes that re-read row 0 (exactly one 128-B line less per 16-lane group) -- so twice the
// workgroups pull 28 + 57 KB each.  Used while few tiles are in flight (launch_ar_steps).
template <int SW, int ROWS>
__global__ __launch_bounds__(256) void ar_fc1_kernel(ArModel m, const ArCall *__restrict__ cp, int t_local, int nbt) {
    __shared__ float red[4][16][17];
    AR_STAMP(threadIdx.x == 0, 1, 0);
    fc1_body<SW, ROWS>(m, cp, t_local, blockIdx.x, blockIdx.y, nbt, red, threadIdx.x, true);
    AR_STAMP(threadIdx.x == 0, 1, 3);
}

// fc2 + draw as a launch of its own (plain candidate arrays; GRANULES = 1: the trailing launch of a fused replay).
template <int GRANULES>
__global__ __launch_bounds__(256) void ar_fc2_kernel(ArModel m, const ArCall *__restrict__ cp, int t_local) {
    __shared__ float red[4][16][17];
    __shared__ float sc[16][17];
    AR_STAMP(threadIdx.x == 0, 2, 0);
    fc2_body<GRANULES>(m, cp, t_local, blockIdx.x, blockIdx.y, gridDim.y, red, sc, threadIdx.x, true);
    AR_STAMP(threadIdx.x == 0, 2, 3);
}

__global__ void ar_advance_kernel(ArCall *c, int n) {
    c->t_base += n;
    if (c->hall && c->t_base - c->hall_t0 >= c->CH) c->hall_t0 += c->CH;      // next chunk of the teacher-forced scan
}
// Between replays (and once before the first): the slot row of the replay that starts at t_base, and -- when a
// slot stays on one conditioning frame per replay (gc_replay) -- that frame's Gcond row per slot.
// One workgroup per decode slot.
__global__ __launch_bounds__(256) void ar_next_row_kernel(ArModel m, const ArCall *__restrict__ cp) {
    const int sg = blockIdx.x;
    const ArCall c = *cp;
    const int r = c.t_base / c.S;
    if (sg >= c.Sp) return;
    if (c.h_out && r > 0 && r - 1 < c.n_rep) {
        // stream chunk: an utterance that ended in the replay just run leaves its state (nothing has written its column since)
        const ArSlot pv = c.slots[(size_t)(r - 1) * c.Sp + sg];
        const int end = pv.t0 + pv.len;
        if (pv.row >= 0 && end > c.t_base - c.S && end <= c.t_base) {
            const float *hb = m.hbuf + (size_t)(end & 1) * c.nbt * m.Hr * 16;
            for (int k = threadIdx.x; k < m.Hr; k += 256) c.h_out[(size_t)pv.row * m.Hr + k] = hb[hl_index(m.Hr, sg, k)];
        }
        __syncthreads();
    }
    if (r >= c.n_rep) return;
    ArSlot sl = c.slots[(size_t)(c.one_row ? 0 : r) * c.Sp + sg];
    if (c.one_row && c.t_base - sl.t0 >= sl.len) sl.row = -1;
    if (threadIdx.x == 0) m.cur[sg] = sl;
    if (c.h_in && sl.row >= 0 && c.t_base - sl.t0 == c.s0) {
        // stream chunk: a resumed utterance starts in this replay (at local step 0: state parity 0) -- its first step is then an
        // ordinary continuing one that finds h_in as its state and x_in as the drawn sample
        for (int k = threadIdx.x; k < m.Hr; k += 256) m.hbuf[hl_index(m.Hr, sg, k)] = c.h_in[(size_t)sl.row * m.Hr + k];
        const int nrg = m.n_cls >> 4, x = c.x_in[sl.row];
        for (int q = threadIdx.x; q < nrg; q += 256) {
            if (m.fused) {
                const unsigned tag = (unsigned)c.t_base & ((1u << CAND_TAG_BITS) - 1u);
                m.candg[((size_t)(sg >> 4) * nrg + q) * 16 + (sg & 15)] = ((u64)((tag << 10) | (unsigned)x) << 32) | __float_as_uint(0.f);
            } else {
                m.cand_s[(size_t)sg * nrg + q] = 0.f;
                m.cand_k[(size_t)sg * nrg + q] = x;
            }
        }
    }
    if (!m.gc_replay || sl.row < 0 || c.t_base < sl.t0) return;
    const int f = (c.t_base - sl.t0) / m.upsample;
    if (f >= c.F) return;
    const float *src = c.Gcond + ((size_t)c.gbase[sl.row] + f) * 3 * m.Hr;
    for (int rg = threadIdx.x; rg < (m.Hr >> 2); rg += 256) {           // [3][Hr] row -> unit quads of row group rg
        const float4 r4 = *(const float4 *)(src + 4 * rg), z4 = *(const float4 *)(src + m.Hr + 4 * rg),
                     n4 = *(const float4 *)(src + 2 * m.Hr + 4 * rg);
        float4 *dst = m.gcur4 + ((size_t)rg * c.Sp + sg) * 4;
        dst[0] = make_float4(r4.x, z4.x, n4.x, 0.f);
        dst[1] = make_float4(r4.y, z4.y, n4.y, 0.f);
        dst[2] = make_float4(r4.z, z4.z, n4.z, 0.f);
        dst[3] = make_float4(r4.w, z4.w, n4.w, 0.f);
    }
}

// [rows][3][H] -> unit quads [rows][H/4][4] float4 (r, z, n, 0)
__global__ void quads_build_kernel(const float *__restrict__ src, float4 *__restrict__ dst, int rows, int H) {
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)rows * H) return;
    const int unit = (int)(id % H);
    const size_t row = id / H;
    const float *s = src + row * 3 * H + unit;
    dst[row * H + unit] = make_float4(s[0], s[H], s[2 * H], 0.f);
}

// End of every replay: an utterance whose last sample fell inside this replay still has that sample
// only as candidates (the next GRU step would have merged them): emit it before the slot is reused.
__global__ void ar_finalize_kernel(ArModel m, const ArCall *__restrict__ cp) {
    const int sg = blockIdx.x * blockDim.x + threadIdx.x;
    const ArCall c = *cp;
    if (sg >= c.Sp || c.inputs) return;
    const ArSlot sl = m.cur[sg];
    if (sl.row < 0) return;
    const int end = sl.t0 + sl.len;
    if (end <= c.t_base || end > c.t_base + c.S) return;
    float best;
    int x;
    const int nrg = m.n_cls >> 4;
    if (m.fused) {
        const u64 *cg = m.candg + ((size_t)(sg >> 4) * nrg) * 16 + (sg & 15);
        u64 gq = ps_load(cg);
        best = __uint_as_float((unsigned)gq);
        x = (int)((gq >> 32) & 1023u);
        for (int q = 1; q < nrg; ++q) {
            gq = ps_load(cg + q * 16);
            const float sc = __uint_as_float((unsigned)gq);
            if (sc > best) { best = sc; x = (int)((gq >> 32) & 1023u); }
        }
    } else {
        best = m.cand_s[(size_t)sg * nrg];
        x = m.cand_k[(size_t)sg * nrg];
        for (int q = 1; q < nrg; ++q) {
            const float sc = m.cand_s[(size_t)sg * nrg + q];
            if (sc > best) { best = sc; x = m.cand_k[(size_t)sg * nrg + q]; }
        }
    }
    if (c.wav) c.wav[(size_t)sl.row * c.Lout + sl.len - 1] = m.mulaw_tab[x];
    if (c.mulaw) c.mulaw[(size_t)sl.row * c.Lout + sl.len - 1] = x;
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

// Pinned staging arena for host-built tables (lengths, decode-slot schedule, call records): the tables are copied in
// and uploaded from there with hipMemcpyAsync, so a decode call never synchronises the caller's stream ("no
// hidden sync").  The arena is reused by the next call only after the event recorded behind this call's uploads.
struct HostStage {
    char *p = nullptr;
    size_t cap = 0, used = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;
    int begin(size_t need) {
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        if (pending) { HIP_TRY(hipEventSynchronize(ev)); pending = false; }       // the PREVIOUS call's uploads only
        if (need > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr; cap = 0;
            const size_t want = need + need / 2 + 4096;
            HIP_TRY(hipHostMalloc((void **)&p, want, hipHostMallocDefault));
            cap = want;
        }
        used = 0;
        return VQCPC_OK;
    }
    int upload(void *dst, const void *src, size_t n, hipStream_t s) {
        const size_t at = (used + 15) & ~(size_t)15;
        VQ_REQUIRE(at + n <= cap, "host staging arena too small (%zu + %zu > %zu)", at, n, cap);
        memcpy(p + at, src, n);
        used = at + n;
        HIP_TRY(hipMemcpyAsync(dst, p + at, n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(ev, s));
        pending = true;
        return VQCPC_OK;
    }
    void release() {
        if (pending && ev) (void)hipEventSynchronize(ev);
        if (p) (void)hipHostFree(p);
        if (ev) (void)hipEventDestroy(ev);
        p = nullptr; ev = nullptr; cap = 0; pending = false;
    }
};

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
// Defaults of the decode-loop options: the handle starts with them, and vqcpc_vocoder_plan takes them for -1 / 0.
constexpr int XCM_MIN_DEFAULT = 68, XCM_MAX_DEFAULT = 512, XCD_SLOTS_DEFAULT = 8 * XD_MAX_BX, XCM_SLOTS_DEFAULT = 8 * XM_BX;

struct vqcpc_vocoder {
    vqcpc_vocoder_weights d;             // dims only (pointers below are owned copies)
    float *code_emb = nullptr, *spk_emb = nullptr;
    float *p_wih[2] = {}, *p_bih[2] = {}, *p_bhh[2] = {}, *p_wf[2] = {};   // per layer, both directions stacked
    float *w_cond = nullptr, *b_ih = nullptr, *Gemb = nullptr;
    float4 *Gemb4 = nullptr, *bh4 = nullptr;
    float *Wf_hh12 = nullptr, *Wf_hh16 = nullptr, *b_hh = nullptr, *Wf_fc1 = nullptr, *Wf_fc1h = nullptr, *b_fc1 = nullptr, *Wf_fc2 = nullptr, *b_fc2 = nullptr;
    float *w_fc1 = nullptr, *w_fc2 = nullptr;      // plain (rows, K) copies for the teacher-forced scan's batched GEMMs
    float *mulaw_tab = nullptr;
    // A decode call runs as 1 or 2 independent TILE GROUPS (disjoint utterance tiles, own state,
    // own call record, own captured graph).  Two groups run on two streams so that one group's GRU
    // step overlaps the other's fc1/fc2; there is no edge between them inside a graph.
    struct Group {
        ArCall *call = nullptr;          // device
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
    unsigned *status_host = nullptr;     // the handle's status word: pinned host memory the kernels write and the host reads without a HIP call
    unsigned *status_dev = nullptr;      // the device's view of it
    HostStage stage;
    float *w_hh = nullptr;               // plain (3Hr, Hr) copy of W_hh for it
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

static void clear_graphs(vqcpc_vocoder::Group &G) {
    for (auto &kv : G.graphs) (void)hipGraphExecDestroy(kv.second);
    G.graphs.clear();
}
static void clear_graphs(vqcpc_vocoder *v) {
    for (auto &G : v->grp) clear_graphs(G);
}

// The handle's grow-only work buffers: freed by vqcpc_vocoder_destroy, counted by vqcpc_vocoder_workspace_bytes.
static std::vector<DevBuf *> work_buffers(vqcpc_vocoder *v) {
    std::vector<DevBuf *> b = {&v->series, &v->gi, &v->out0, &v->cond, &v->gcond, &v->gbase, &v->hseq, &v->len, &v->hall, &v->a1c, &v->nll_part, &v->nll_len,
                               &v->xd_x, &v->xd_segs};
    for (auto &G : v->grp) b.insert(b.end(), {&G.har, &G.a1, &G.cand_s, &G.cand_k, &G.slot_tab, &G.cur, &G.gcur, &G.candg});
    return b;
}

static int dcopy(float **dst, const float *src, size_t n) {
    HIP_TRY(hipMalloc((void **)dst, n * sizeof(float)));
    HIP_TRY(hipMemcpy(*dst, src, n * sizeof(float), hipMemcpyDeviceToDevice));
    return VQCPC_OK;
}

extern "C" void vqcpc_vocoder_destroy(vqcpc_vocoder *v) {
    if (!v) return;
    clear_graphs(v);
    for (auto &g : v->grp) if (g.call) (void)hipFree(g.call);
    for (DevBuf *b : work_buffers(v)) b->release();
    if (v->side_stream) (void)hipStreamDestroy(v->side_stream);
    if (v->ev_fork) (void)hipEventDestroy(v->ev_fork);
    if (v->ev_join) (void)hipEventDestroy(v->ev_join);
    float *ptrs[] = {v->code_emb, v->spk_emb, v->p_wih[0], v->p_wih[1], v->p_bih[0], v->p_bih[1], v->p_bhh[0],
                     v->p_bhh[1], v->p_wf[0], v->p_wf[1], v->w_cond, v->b_ih, v->Gemb, v->Wf_hh12, v->Wf_hh16, v->b_hh,
                     v->Wf_fc1, v->Wf_fc1h, v->b_fc1, v->Wf_fc2, v->b_fc2, v->mulaw_tab, v->w_fc1, v->w_fc2};
    for (float *p : ptrs) if (p) (void)hipFree(p);
    v->stage.release();
    if (v->status_host) (void)hipHostFree(v->status_host);
    if (v->w_hh) (void)hipFree(v->w_hh);
    if (v->Gemb4) (void)hipFree(v->Gemb4);
    if (v->bh4) (void)hipFree(v->bh4);
    if (v->cap_stream) (void)hipStreamDestroy(v->cap_stream);
    if (v->ev0) (void)hipEventDestroy(v->ev0);
    if (v->ev1) (void)hipEventDestroy(v->ev1);
    delete v;
}

static int vocoder_create_impl(const vqcpc_vocoder_weights *w, vqcpc_vocoder *v) {
    v->d = *w;
    const int F = w->dz + w->ds, Hp = w->Hp, dl = 2 * Hp, Hr = w->Hr, de = w->de;
    TRY(dcopy(&v->code_emb, w->code_embedding, (size_t)w->n_codes * w->dz));
    TRY(dcopy(&v->spk_emb, w->speaker_embedding, (size_t)w->n_speakers * w->ds));
    for (int l = 0; l < 2; ++l) {
        const int I = l == 0 ? F : dl;
        HIP_TRY(hipMalloc((void **)&v->p_wih[l], (size_t)6 * Hp * I * sizeof(float)));
        HIP_TRY(hipMalloc((void **)&v->p_bih[l], (size_t)6 * Hp * sizeof(float)));
        HIP_TRY(hipMalloc((void **)&v->p_bhh[l], (size_t)6 * Hp * sizeof(float)));
        HIP_TRY(hipMalloc((void **)&v->p_wf[l], (size_t)2 * (Hp / 4) * (Hp / 16) * 64 * sizeof(float4)));
        for (int d = 0; d < 2; ++d) {
            HIP_TRY(hipMemcpy(v->p_wih[l] + (size_t)d * 3 * Hp * I, w->prenet_w_ih[l][d], (size_t)3 * Hp * I * sizeof(float), hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(v->p_bih[l] + (size_t)d * 3 * Hp, w->prenet_b_ih[l][d], (size_t)3 * Hp * sizeof(float), hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(v->p_bhh[l] + (size_t)d * 3 * Hp, w->prenet_b_hh[l][d], (size_t)3 * Hp * sizeof(float), hipMemcpyDeviceToDevice));
            float *tmp = nullptr;
            TRY(vq_build_wfrag(w->prenet_w_hh[l][d], Hp, Hp / 4, Hp, 4, 3, Hp, &tmp));
            const size_t nb = (size_t)(Hp / 4) * (Hp / 16) * 64 * sizeof(float4);
            HIP_TRY(hipMemcpy((char *)v->p_wf[l] + d * nb, tmp, nb, hipMemcpyDeviceToDevice));
            HIP_TRY(hipFree(tmp));
        }
    }
    // AR input weights split: [:, :de] feeds the sample embedding (-> lookup table Gemb), [:, de:] the conditioning
    float *w_emb = nullptr;
    HIP_TRY(hipMalloc((void **)&w_emb, (size_t)3 * Hr * de * sizeof(float)));
    HIP_TRY(hipMalloc((void **)&v->w_cond, (size_t)3 * Hr * dl * sizeof(float)));
    hipLaunchKernelGGL(copy_submatrix_kernel, dim3((unsigned)(((size_t)3 * Hr * de + 255) / 256)), dim3(256), 0, 0,
                       w->ar_w_ih, de + dl, 0, w_emb, 3 * Hr, de);
    hipLaunchKernelGGL(copy_submatrix_kernel, dim3((unsigned)(((size_t)3 * Hr * dl + 255) / 256)), dim3(256), 0, 0,
                       w->ar_w_ih, de + dl, de, v->w_cond, 3 * Hr, dl);
    HIP_TRY(hipGetLastError());
    TRY(dcopy(&v->b_ih, w->ar_b_ih, (size_t)3 * Hr));
    TRY(dcopy(&v->b_hh, w->ar_b_hh, (size_t)3 * Hr));
    HIP_TRY(hipMalloc((void **)&v->Gemb, (size_t)w->n_cls * 3 * Hr * sizeof(float)));
    float *emb = nullptr;
    TRY(dcopy(&emb, w->ar_embedding, (size_t)w->n_cls * de));
    TRY(vq_gemm_chain(emb, de, w_emb, nullptr, v->Gemb, 3 * Hr, w->n_cls, 3 * Hr, de, de, 0));
    HIP_TRY(hipMalloc((void **)&v->Gemb4, (size_t)w->n_cls * Hr * sizeof(float4)));
    HIP_TRY(hipMalloc((void **)&v->bh4, (size_t)Hr * sizeof(float4)));
    hipLaunchKernelGGL(quads_build_kernel, dim3((unsigned)(((size_t)w->n_cls * Hr + 255) / 256)), dim3(256), 0, 0, v->Gemb, v->Gemb4, w->n_cls, Hr);
    hipLaunchKernelGGL(quads_build_kernel, dim3((unsigned)((Hr + 255) / 256)), dim3(256), 0, 0, v->b_hh, v->bh4, 1, Hr);
    HIP_TRY(hipGetLastError());
    TRY(build_wfrag12(w->ar_w_hh, Hr, Hr / 4, Hr, Hr, &v->Wf_hh12));
    if (Hr % 16 == 0) TRY(vq_build_wfrag(w->ar_w_hh, Hr, 3 * (Hr / 16), Hr, 4, 16, Hr, &v->Wf_hh16));
    TRY(vq_build_wfrag(w->fc1_weight, Hr, w->Hf / 16, Hr, 4, 0, 0, &v->Wf_fc1));
    TRY(vq_build_wfrag(w->fc1_weight, Hr, w->Hf / 8, Hr, 4, 8, 0, &v->Wf_fc1h));
    TRY(vq_build_wfrag(w->fc2_weight, w->Hf, w->n_cls / 16, w->Hf, 1, 0, 0, &v->Wf_fc2));
    TRY(dcopy(&v->w_hh, w->ar_w_hh, (size_t)3 * Hr * Hr));
    TRY(dcopy(&v->w_fc1, w->fc1_weight, (size_t)w->Hf * Hr));
    TRY(dcopy(&v->w_fc2, w->fc2_weight, (size_t)w->n_cls * w->Hf));
    TRY(dcopy(&v->b_fc1, w->fc1_bias, w->Hf));
    TRY(dcopy(&v->b_fc2, w->fc2_bias, w->n_cls));
    // mu-law decode table (preprocess.py:30-35, evaluated in float64 like the reference's numpy)
    std::vector<float> tab(w->n_cls);
    const double mu = (double)((1 << w->bits_mu_law) - 1);
    for (int s = 0; s < w->n_cls; ++s) {
        const double y = 2.0 * (double)s / mu - 1.0, sg = (y > 0) - (y < 0);
        tab[s] = (float)(sg / mu * (pow(1.0 + mu, fabs(y)) - 1.0));
    }
    HIP_TRY(hipMalloc((void **)&v->mulaw_tab, tab.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(v->mulaw_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    for (auto &g : v->grp) HIP_TRY(hipMalloc((void **)&g.call, sizeof(ArCall)));
    if (w->Hf == NLL_HF && w->n_cls == NLL_CLS) TRY(vq_tf_nll_prepare());      // the scoring head's LDS attribute, once per handle
    HIP_TRY(hipHostMalloc((void **)&v->status_host, 64, hipHostMallocMapped));
    *v->status_host = 0u;
    HIP_TRY(hipHostGetDevicePointer((void **)&v->status_dev, v->status_host, 0));
    HIP_TRY(hipStreamCreateWithFlags(&v->side_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&v->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&v->ev_join, hipEventDisableTiming));
    HIP_TRY(hipStreamCreateWithFlags(&v->cap_stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&v->ev0));
    HIP_TRY(hipEventCreate(&v->ev1));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipFree(w_emb));
    HIP_TRY(hipFree(emb));
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
static int status_check(vqcpc_vocoder *v, bool synced) {
    if (!v->status_pending) return VQCPC_OK;
    const unsigned flag = *(volatile unsigned *)v->status_host;        // written by the kernel; no HIP call
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
    *(volatile unsigned *)v->status_host = 0u;
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
            if (!v->fell_back) { v->saved_xcd = v->xcd; v->saved_fuse_fc2 = v->fuse_fc2; }
            v->fell_back = true; v->clean_calls = 0;
            v->xcd = 0;
            vq_set_error("decode not run (%s): the resident decoders' workgroups were not dealt 32 to each XCD, twice in a row (no output was "
                         "written; the GPU is probably shared) -- this handle now uses one launch per kernel and step; repeat the call", which);
        } else {
            vq_set_error("decode not run (%s): the resident decoders' workgroups were not dealt 32 to each XCD (no output was written; "
                         "another kernel held compute units) -- repeat the call", which);
        }
        return VQCPC_ERR_HIP;
    }
    if (!v->fell_back) { v->saved_xcd = v->xcd; v->saved_fuse_fc2 = v->fuse_fc2; }
    v->fell_back = true; v->clean_calls = 0;
    v->xcd = 0;
    if (v->fuse_fc2) { v->fuse_fc2 = 0; clear_graphs(v); }
    vq_set_error("decode aborted (%s): an in-kernel exchange timed out (outputs of that call are incomplete); this handle now uses one launch "
                 "per kernel and step, and re-arms after %d clean calls or set_option xcd / fuse_fc2 -- repeat the call", which, REARM_CLEAN);
    return VQCPC_ERR_HIP;
}

extern "C" int vqcpc_vocoder_last_path(vqcpc_vocoder *v) {
    if (!v) return -1;
    return v->last_path;
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
    for (DevBuf *b : work_buffers(v)) n += b->cap;
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
static int run_condition(vqcpc_vocoder *v, const int64_t *idx, const int64_t *spk, int B, int Tc,
                         const int *frames_dev, const int *row0_dev, size_t n_rows, float *cond_out, hipStream_t s) {
    const auto &d = v->d;
    const int F = d.dz + d.ds, Hp = d.Hp, dl = 2 * Hp, T2 = 2 * Tc, nbt = (B + 15) / 16;
    const size_t rows = row0_dev ? (n_rows ? n_rows : 1) : (size_t)B * T2;
    TRY(v->series.reserve(rows * F * sizeof(float)));
    TRY(v->gi.reserve(rows * 6 * Hp * sizeof(float)));
    TRY(v->out0.reserve(rows * dl * sizeof(float)));
    const size_t hsz = (size_t)2 * nbt * Hp * 16 * sizeof(float);
    TRY(v->hseq.reserve(2 * hsz));
    const size_t ng = (size_t)B * T2 * F;
    hipLaunchKernelGGL(glue_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, s, idx, spk, v->code_emb,
                       v->spk_emb, v->series.as<float>(), B, Tc, d.dz, d.ds, d.n_codes, d.n_speakers, v->status_dev, v->epoch << 8,
                       frames_dev, row0_dev);
    v->status_pending = true;            // an index outside its table is reported through the status word
    for (int l = 0; l < 2; ++l) {
        const float *xin = l == 0 ? v->series.as<float>() : v->out0.as<float>();
        const int I = l == 0 ? F : dl;
        float *xout = l == 0 ? v->out0.as<float>() : cond_out;
        TRY(vq_gemm_chain(xin, I, v->p_wih[l], v->p_bih[l], v->gi.as<float>(), 6 * Hp, (int)rows, 6 * Hp, I, I, s));
        if (frames_dev && !row0_dev) HIP_TRY(hipMemsetAsync(xout, 0, rows * dl * sizeof(float), s));      // dense rows past an utterance's end
        TRY(vq_bigru_scan(v->p_wf[l], v->p_bhh[l], v->gi.as<float>(), v->hseq.as<float>(), xout, frames_dev, row0_dev, Hp, B, T2, s));
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

// Hidden sizes the per-sample kernels are instantiated for (size_h_rnn = 64 SW): 512, 896 (the reference's, config.py:76), 1024.
// (Round 2 compiled nine values x every variant = ~190 kernels; a size outside the list is an explicit error at create.)
#define AR_SW_CASES(X) X(8) X(14) X(16)

static size_t big_lds_bytes(int Hr) { return (size_t)2 * Hr * 16 * sizeof(float) + (size_t)2 * 3 * 4 * 16 * 17 * sizeof(float); }
static bool use_big(const vqcpc_vocoder *v, int nbt) {
    return v->big_min_tiles > 0 && nbt >= v->big_min_tiles && v->d.Hr % 16 == 0 && big_lds_bytes(v->d.Hr) <= 160 * 1024;
}
// One GRU-step launch for local step `tl`; nf = fc2 blocks of the previous step in front (fused launch, 0 = none).
static int launch_gru_step(vqcpc_vocoder *v, const ArModel &m, const ArCall *call, int tl, int nbt, int nf, hipStream_t s) {
    const int Hr = v->d.Hr, rgs = Hr / 4, npass = (nbt + 1) / 2;
    const bool big = use_big(v, nbt);
    const size_t lds = big_lds_bytes(Hr);
    switch (Hr / 64) {
#define CASE(k) case k: \
        if (m.fused && big) hipLaunchKernelGGL((ar_gru_big_kernel<k, 1>), dim3(nf + (Hr / 16) * npass), dim3(1024), lds, s, m, call, tl, nbt, nf); \
        else if (m.fused && nbt == 1) hipLaunchKernelGGL((ar_gru_kernel<k, 1, 3, 1>), dim3(nf + rgs), dim3(320), 0, s, m, call, tl, nbt, nf); \
        else if (m.fused) hipLaunchKernelGGL((ar_gru_kernel<k, 2, 3, 1>), dim3(nf + rgs * npass), dim3(384), 0, s, m, call, tl, nbt, nf); \
        else if (nbt == 1) hipLaunchKernelGGL((ar_gru_kernel<k, 1, 3, 0>), dim3(rgs), dim3(320), 0, s, m, call, tl, nbt, 0); \
        else if (big) hipLaunchKernelGGL((ar_gru_big_kernel<k, 0>), dim3(Hr / 16, npass), dim3(1024), lds, s, m, call, tl, nbt, 0); \
        else if (m.lead6) hipLaunchKernelGGL((ar_gru_kernel<k, 2, 6, 0>), dim3(rgs, npass), dim3(384), 0, s, m, call, tl, nbt, 0); \
        else hipLaunchKernelGGL((ar_gru_kernel<k, 2, 3, 0>), dim3(rgs, npass), dim3(384), 0, s, m, call, tl, nbt, 0); \
        break;
        AR_SW_CASES(CASE)
#undef CASE
        default: vq_set_error("AR step: size_h_rnn %d unsupported", Hr); return VQCPC_ERR_INVALID;
    }
    return VQCPC_OK;
}
static int launch_fc1_step(vqcpc_vocoder *v, const ArModel &m, const ArCall *call, int tl, int nbt, hipStream_t s) {
    const dim3 blk(256);
    switch (v->d.Hr / 64) {
#define CASE(k) case k: \
        if (nbt <= 4) hipLaunchKernelGGL((ar_fc1_kernel<k, 8>), dim3(v->d.Hf / 8, nbt), blk, 0, s, m, call, tl, nbt); \
        else hipLaunchKernelGGL((ar_fc1_kernel<k, 16>), dim3(v->d.Hf / 16, nbt), blk, 0, s, m, call, tl, nbt); \
        break;
        AR_SW_CASES(CASE)
#undef CASE
        default: vq_set_error("AR step: size_h_rnn %d unsupported", v->d.Hr); return VQCPC_ERR_INVALID;
    }
    return VQCPC_OK;
}

// tf: teacher-forced scan -- x_{t-1} comes from the inputs, so only the GRU step runs per sample (fc1 / fc2 follow
// as batched GEMMs over the whole chunk, run_launch_path)
static int launch_ar_steps(vqcpc_vocoder *v, const ArModel &m, ArCall *call, int nbt, int n, bool tf, hipStream_t s) {
    const dim3 blk(256);
    const bool big = use_big(v, nbt);
    if (big && !v->big_attr_set) {
        switch (v->d.Hr / 64) {
#define CASE(k) case k: HIP_TRY(hipFuncSetAttribute((const void *)ar_gru_big_kernel<k, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds_bytes(v->d.Hr))); \
                        HIP_TRY(hipFuncSetAttribute((const void *)ar_gru_big_kernel<k, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds_bytes(v->d.Hr))); break;
            AR_SW_CASES(CASE)
#undef CASE
            default: break;
        }
        v->big_attr_set = true;
    }
    // Fused schedule (m.fused): step i = { fc2 of step i-1  ||  GRU of step i } in ONE launch, then fc1 of step i; the
    // fc2 of the replay's last step runs as a trailing launch (before the slot records change), so the first launch of a
    // replay carries no fc2 blocks.  (fc1 in the same launch as well -- one launch per sample -- was built and measured in
    // round 2 and loses at every batch size: profiles/r02_gru_variants_one_launch.csv; removed.)
    const int f2_full = big ? (v->d.n_cls / 16) * nbt / 4 : (v->d.n_cls / 16) * nbt;
    for (int i = 0; i < n; ++i) {
        TRY(launch_gru_step(v, m, call, i, nbt, (m.fused && i > 0) ? f2_full : 0, s));
        if (tf) continue;
        TRY(launch_fc1_step(v, m, call, i, nbt, s));
        if (!m.fused) hipLaunchKernelGGL(ar_fc2_kernel<0>, dim3(v->d.n_cls / 16, nbt), blk, 0, s, m, (const ArCall *)call, i);
    }
    if (!tf && m.fused) hipLaunchKernelGGL(ar_fc2_kernel<1>, dim3(v->d.n_cls / 16, nbt), blk, 0, s, m, (const ArCall *)call, n - 1);
    if (!tf) hipLaunchKernelGGL(ar_finalize_kernel, dim3((nbt * 16 + 63) / 64), dim3(64), 0, s, m, (const ArCall *)call);
    hipLaunchKernelGGL(ar_advance_kernel, dim3(1), dim3(1), 0, s, call, n);
    hipLaunchKernelGGL(ar_next_row_kernel, dim3(nbt * 16), dim3(256), 0, s, m, (const ArCall *)call);
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
};

static int tf_chunk_nll(vqcpc_vocoder *v, int B, int CH, int chunk, const NllCall &nc, hipStream_t s) {
    NllHead h{};
    h.hall = v->hall.as<float>(); h.w1 = v->w_fc1; h.b1 = v->b_fc1; h.w2 = v->w_fc2; h.b2 = v->b_fc2;
    h.audio = nc.audio; h.slen = v->nll_len.as<int>(); h.nll = nc.nll; h.part = v->nll_part.as<NllPart>();
    h.status = v->status_dev; h.status_tag = v->epoch << 8;
    h.B = B; h.L = nc.L; h.CH = CH; h.t0 = chunk * CH; h.Hr = v->d.Hr;
    return vq_tf_nll_chunk(h, nc.nll_sum, nc.n_scored, nc.n_correct, s);
}

// Which decode loop takes a call, and the resident decoders' slot schedule: pure host arithmetic (no HIP call), so that it can be
// tested without a GPU (vqcpc_vocoder_plan).  samples[b] = samples utterance b produces; `order` = utterances longest first.
// path 2 / 3: the per-XCD decoders (VALU / matrix-core form) through `xs` slots, slot q running lists[q] back to back;
// path 0: the launch-per-step kernels.  A slot's schedule must stay below 2^24 - 1 steps (the candidate tag of step t is
// (t + 1) << 8 in 32 bits): a call `auto` would have put on the resident decoders then takes the launch path; asked for by name
// (xcd / xcm = 1) it is an error (returns false).
struct DecodePlan {
    int path = 0, xs = 0, bxt = 0;
    long longest = 0;
    std::vector<std::vector<XdSeg>> lists;
    std::vector<long> xend;
};
struct PlanOpts { int xcd, xcm, xcm_min, xcm_max, xcd_slots, xcm_slots, n_slots; bool supported; };

static std::vector<int> longest_first(const int *samples, int B) {
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return samples[a] > samples[b]; });
    return order;
}

// Longest-first assignment (LPT) of the utterances of `order` over xs slots: each onto the slot that frees up first (the lowest
// on a tie), where it starts; a slot frees up at the first multiple of `gran` steps from the end of its last utterance
// (steps_per_graph on the launch path, whose utterances start at replay boundaries; 1 on the resident decoders).
static void lpt(const std::vector<int> &order, const int *samples, const unsigned *utt, int xs, int gran, DecodePlan &pl) {
    pl.xend.assign(xs, 0);
    pl.lists.assign(xs, {});
    for (int row : order) {
        const int len = samples[row];
        if (len <= 0) continue;
        int best = 0;
        for (int q = 1; q < xs; ++q) if (pl.xend[q] < pl.xend[best]) best = q;
        pl.lists[best].push_back(XdSeg{row, (int)pl.xend[best], len, utt ? utt[row] : (unsigned)row});
        pl.xend[best] = (pl.xend[best] + len + gran - 1) / gran * gran;
    }
    pl.longest = 0;
    for (long e : pl.xend) pl.longest = e > pl.longest ? e : pl.longest;
}

static bool plan_decode(const PlanOpts &o, const int *samples, const unsigned *utt, const std::vector<int> &order, DecodePlan &pl) {
    int nz = 0;
    long max_len = 0;
    for (int row : order) { nz += samples[row] > 0; max_len = samples[row] > max_len ? samples[row] : max_len; }
    pl = DecodePlan{};
    // auto: up to xcm_min (68) utterances in flight ar_xcd.hip (8.5 M samples/s through its 32 slots at 32 and 64 utterances
    // against 3.4 / 4.7 M on the launch path), from there to xcm_max the 16-slot matrix-core form through its 128 slots (9.3 M at 96,
    // 12.4 M from 128), above that the launch-per-step kernels; `xcd` = 0 turns both off, = 1 asks for ar_xcd.hip whatever the count
    const int in_flight = o.n_slots > 0 && o.n_slots < nz ? o.n_slots : nz;
    const bool xcm_wanted = o.xcd != 0 && (o.xcm == 1 || (o.xcm == -1 && o.xcd == -1 && in_flight > o.xcm_min && in_flight < o.xcm_max));
    const bool xcd_wanted = xcm_wanted || o.xcd == 1 || (o.xcd == -1 && in_flight <= o.xcm_min);
    if (!xcd_wanted || !o.supported || max_len <= 0 || nz <= 0) return true;
    int xs = xcm_wanted ? o.xcm_slots : (o.xcd_slots < 1 ? 1 : o.xcd_slots);
    if (o.n_slots > 0 && o.n_slots < xs) xs = o.n_slots;
    if (nz < xs) xs = nz;
    const int bxt = xcm_wanted ? XM_BX : xd_pick_bxt((xs + 7) / 8);
    lpt(order, samples, utt, xs, 1, pl);
    const bool fits = bxt > 0 && pl.longest + 1 < (1L << 24);
    if (!fits) {
        pl.lists.clear(); pl.xend.clear();
        return !(o.xcd == 1 || o.xcm == 1);
    }
    pl.path = xcm_wanted ? 3 : 2; pl.xs = xs; pl.bxt = bxt;
    return true;
}

extern "C" int vqcpc_vocoder_plan(int xcd, int xcm, int xcm_min, int xcm_max, int xcd_slots, int xcm_slots, int slots,
                                  const int *n_samples, int B, int *path, int *slots_used, int64_t *longest) {
    VQ_REQUIRE(n_samples && B > 0 && path && slots_used && longest, "vqcpc_vocoder_plan: bad argument");
    DecodePlan pl;
    const PlanOpts o{xcd, xcm, xcm_min < 0 ? XCM_MIN_DEFAULT : xcm_min, xcm_max < 0 ? XCM_MAX_DEFAULT : xcm_max,
                     xcd_slots <= 0 ? XCD_SLOTS_DEFAULT : xcd_slots, xcm_slots <= 0 ? XCM_SLOTS_DEFAULT : xcm_slots, slots, true};
    VQ_REQUIRE(plan_decode(o, n_samples, nullptr, longest_first(n_samples, B), pl), "vocoder: a decode slot's schedule does not fit "
               "the resident decoders (< 2^24 - 1 samples); use more slots or xcd = -1");
    *path = pl.path; *slots_used = pl.path ? pl.xs : (slots > 0 && slots < B ? slots : B); *longest = pl.longest;
    return VQCPC_OK;
}

// A decode call as planned on the host before anything is uploaded (no HIP call).
struct CallPlan {
    std::vector<int> lens;               // [frames | samples] per utterance, Bp entries each
    std::vector<unsigned> utt;           // sampling-stream id per utterance
    std::vector<int> gbase;              // first conditioning row per utterance (prefix sums of the frame counts)
    long grows = 0;                      // conditioning rows in all
    DecodePlan dp;                       // path 0: the launch path's dp.xs slots, utterances starting at replay boundaries
    int n_grp = 1, tiles[2] = {0, 0}, rep[2] = {0, 0}, gmax[2] = {0, 0};   // launch path: tile groups (tiles, replays, steps)
    std::vector<ArSlot> table[2];        // launch path: per group [replay][slot] what every decode slot is doing
};

static int plan_launch_tables(const vqcpc_vocoder *v, const int *samples, const std::vector<int> &order, bool tf, int B, int s0,
                              CallPlan &cp);
static int plan_call(const vqcpc_vocoder *v, int B, int Tc, const int *n_codes_host, bool tf, int Ts, int max_steps,
                     unsigned utt_base, const uint32_t *utt_ids_host, CallPlan &cp, const int *tf_len = nullptr) {
    const auto &d = v->d;
    const int Bp = (B + 15) / 16 * 16;
    // per-utterance lengths: frames for the prenet, samples for the AR loop
    cp.lens.assign(2 * Bp, 0);
    cp.utt.resize(B);
    for (int b = 0; b < B; ++b) {
        int nc = n_codes_host ? n_codes_host[b] : Tc;
        VQ_REQUIRE(nc >= 0 && nc <= Tc, "vocoder: n_codes[%d] = %d outside [0, %d]", b, nc, Tc);
        cp.lens[b] = 2 * nc;
        int ns = d.upsample_t * 2 * nc;
        if (tf) ns = ns < Ts ? ns : Ts;
        if (tf && tf_len) ns = ns < tf_len[b] ? ns : tf_len[b];      // a scoring call: the utterance's own scored length
        if (max_steps > 0 && ns > max_steps) ns = max_steps;
        cp.lens[Bp + b] = ns;
        cp.utt[b] = utt_ids_host ? utt_ids_host[b] : utt_base + (unsigned)b;
    }
    // Conditioning over every utterance's own frames (ragged rows)
    cp.gbase.assign(Bp, 0);
    for (int b = 0; b < B; ++b) { cp.gbase[b] = (int)cp.grows; cp.grows += cp.lens[b]; }
    VQ_REQUIRE(cp.grows < (1L << 31), "vocoder: %ld conditioning frames in one call", cp.grows);
    const int *samples = cp.lens.data() + Bp;
    const std::vector<int> order = longest_first(samples, B);
    const PlanOpts po{v->xcd, v->xcm, v->xcm_min, v->xcm_max, v->xcd_slots, v->xcm_slots, tf ? 0 : v->n_slots,
                      !tf && xd_supported(d.Hr, d.Hf, d.n_cls)};
    VQ_REQUIRE(plan_decode(po, samples, cp.utt.data(), order, cp.dp), "vocoder: a decode slot's schedule does not fit the resident "
               "decoders (< 2^24 - 1 samples); use more slots or xcd = -1");
    if (cp.dp.path != 0) return VQCPC_OK;
    return plan_launch_tables(v, samples, order, tf, B, 0, cp);
}

// The launch path's schedule: slots, tile groups and per-replay slot tables.  s0 > 0 (a stream chunk): every utterance resumes at
// absolute sample s0, and its slot rows say t0 - s0 and s0 + len (ArCall::s0).
static int plan_launch_tables(const vqcpc_vocoder *v, const int *samples, const std::vector<int> &order, bool tf, int B, int s0,
                              CallPlan &cp) {
    const int S = v->steps_per_graph;
    // Launch path (continuous batching): n_slots >= B: everything starts at 0.
    DecodePlan &dp = cp.dp;
    dp.xs = !tf && v->n_slots > 0 && v->n_slots < B ? v->n_slots : B;
    lpt(order, samples, cp.utt.data(), dp.xs, S, dp);
    VQ_REQUIRE(dp.longest < (1L << 30), "vocoder: schedule too long");
    const int nbt = (dp.xs + 15) / 16;
    // Tile groups: 3..big_min_tiles-1 tiles, or >= 2*big_min_tiles (both halves on the large-batch kernel), split in two.  (Measured: 2 x 16 utterances is slower than one
    // group of 32 -- the chip retires only ~0.43 dependent launches per us across queues -- while
    // 2 x 32 runs at 14.5 us per sample against 17.3 us for one group of 64.)  A teacher-forced scan runs as one group.
    // With the fused fc2 || GRU launch the overlap two groups were for happens inside one launch, and two fused launches in
    // flight only compete (64 utterances: 17.4 us per step on two groups, 13.4 on one: profiles/r02_gru_variants.csv): the
    // small kernel runs as ONE group; only large-batch calls of >= 2 * big_min_tiles tiles are still split.
    const bool small_fused = v->fuse_fc2 && !(v->big_min_tiles > 0 && nbt >= v->big_min_tiles);
    const bool split = !tf && v->two_groups && v->use_graph && nbt >= 3 && !small_fused &&
                       !(v->big_min_tiles > 0 && nbt >= v->big_min_tiles && nbt < 2 * v->big_min_tiles);
    cp.n_grp = split ? 2 : 1;
    cp.tiles[0] = split ? (nbt + 1) / 2 : nbt;
    cp.tiles[1] = split ? nbt / 2 : 0;
    for (int g = 0; g < cp.n_grp; ++g) {
        const int slot0 = g * cp.tiles[0] * 16, Spg = cp.tiles[g] * 16;
        const int q_end = slot0 + Spg < dp.xs ? slot0 + Spg : dp.xs;
        long end = 0;
        for (int q = slot0; q < q_end; ++q) end = dp.xend[q] > end ? dp.xend[q] : end;
        cp.gmax[g] = (int)end; cp.rep[g] = cp.gmax[g] / S;
        cp.table[g].assign((size_t)(cp.rep[g] > 0 ? cp.rep[g] : 1) * Spg, ArSlot{-1, 0, 0, 0u});
        for (int q = slot0; q < q_end; ++q)
            for (const XdSeg &sg : dp.lists[q])
                for (int r = sg.t0 / S; r < (sg.t0 + sg.len + S - 1) / S; ++r)
                    cp.table[g][(size_t)r * Spg + (q - slot0)] = ArSlot{sg.row, sg.t0 - s0, sg.len + s0, sg.utt};
    }
    return VQCPC_OK;
}

// What a stream chunk (vqcpc_vocoder_stream_next) hands the decode loops: every utterance resumes at absolute sample s0 from
// (h_in, x_in) -- null at s0 = 0 -- and leaves its final h in h_out.  wav / mulaw are the stream's (B, Lout = n + 1) buffers:
// sample s0 + j at column 1 + j, column 0 takes what the first step re-emits.  The conditioning is the stream's own.
struct Resume {
    int s0, Lout;
    const float *Gcond;
    const int *gbase;                    // device copy of cp.gbase (the launch path reads it)
    const float *h_in;
    const int *x_in;
    float *h_out;
};

// One resident, weight-stationary decoder per XCD (ar_xcd.hip, or its matrix-core form ar_xcm.hip): slot q runs the utterances
// of cp.dp.lists[q] back to back (no replay boundaries here).
static int run_resident(vqcpc_vocoder *v, const CallPlan &cp, int T2, unsigned long long seed, float *wav, int64_t *mulaw,
                        hipStream_t s, const Resume *rs = nullptr) {
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
    xp.segs = v->xd_segs.as<XdSeg>(); xp.xg = v->xd_x.as<unsigned long long>(); xp.status = v->status_dev;
    xp.status_tag = v->epoch << 8;
    xp.wav = wav; xp.mulaw = mulaw; xp.seed = seed; xp.max_seg = (int)max_seg; xp.n_slots = pl.xs; xp.bxt = pl.bxt;
    xp.Lout = d.upsample_t * T2; xp.F = T2; xp.upsample = d.upsample_t; xp.agent_stores = v->xcd_agent_stores;
    xp.timeout_ticks = (unsigned)v->xcd_timeout_ms * 100000u; xp.dbg_drop_step = v->xcd_debug_drop_step;
    xp.dbg_misplace = v->xcd_debug_misplace;
    XdResume xr{};
    if (rs) {
        xp.Lout = rs->Lout; xp.Gcond = rs->Gcond;
        xr = XdResume{rs->s0, rs->h_in, rs->x_in, rs->h_out};
    }
    v->xcd_debug_misplace = 0;                     // one shot: the repeated call finds the workgroups where they are
    HIP_TRY(hipEventRecord(v->ev0, s));
    TRY(pl.path == 3 ? xm_launch(xp, s) : xd_launch(xp, s, rs ? &xr : nullptr));
    HIP_TRY(hipEventRecord(v->ev1, s));
    v->last_steps = (int)pl.longest;
    v->last_slots = pl.xs;
    v->last_path = pl.path;
    v->status_pending = true;
    return VQCPC_OK;
}

// The cached graph of one replay of group g (captured on first use).  A graph bakes its ArModel's buffer pointers: when a
// workspace of the group moved, the group's cached graphs are dropped first.
static int group_graph(vqcpc_vocoder *v, int g, const ArModel &m, int nbt, bool tf, hipGraphExec_t *out) {
    auto &G = v->grp[g];
    const void *now[8] = {G.har.p, G.a1.p, G.cand_s.p, G.cand_k.p, G.cur.p, G.gcur.p, G.candg.p, nullptr};
    if (memcmp(G.baked, now, sizeof now) != 0) {
        clear_graphs(G);
        memcpy(G.baked, now, sizeof now);
    }
    const int gkey = (((nbt * 17 + m.live_last) * 2 + m.lead6) * 2 + (tf ? 1 : 0)) * 3 + m.fused;   // what the capture bakes
    auto it = G.graphs.find(gkey);
    if (it == G.graphs.end()) {
        hipGraph_t gr = nullptr;
        hipGraphExec_t ge = nullptr;
        HIP_TRY(hipStreamBeginCapture(v->cap_stream, hipStreamCaptureModeThreadLocal));
        int rc = launch_ar_steps(v, m, G.call, nbt, v->steps_per_graph, tf, v->cap_stream);
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
static int run_launch_path(vqcpc_vocoder *v, const CallPlan &cp, const int64_t *inputs, int T2, int Ts, unsigned long long seed,
                           float *wav, int64_t *mulaw, float *logits, hipStream_t s, const Resume *rs = nullptr,
                           const NllCall *nc = nullptr) {
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
        TRY(G.slot_tab.reserve(tab_n * sizeof(ArSlot)));
        TRY(G.cur.reserve((size_t)Spg * sizeof(ArSlot)));
        TRY(v->stage.upload(G.slot_tab.p, cp.table[g].data(), tab_n * sizeof(ArSlot), s));
        TRY(v->stage.upload(G.cur.p, cp.table[g].data(), (size_t)Spg * sizeof(ArSlot), s));
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
        c.slots = G.slot_tab.as<ArSlot>(); c.S = S; c.Sp = Spg; c.n_rep = cp.rep[g] > 0 ? cp.rep[g] : 1;
        c.F = T2; c.Ts = Ts; c.Lout = d.upsample_t * T2; c.max_t = cp.gmax[g]; c.nbt = nb; c.seed = seed; c.t_base = 0;
        if (rs) {
            // sample s0 + j of a row goes to column 1 + j: the step kernels index with the absolute sample from a base s0 - 1 columns back
            c.Gcond = rs->Gcond; c.gbase = rs->gbase; c.Lout = rs->Lout;
            c.wav = wav ? (float *)((uintptr_t)wav - (uintptr_t)(rs->s0 - 1) * sizeof(float)) : nullptr;
            c.mulaw = mulaw ? (int64_t *)((uintptr_t)mulaw - (uintptr_t)(rs->s0 - 1) * sizeof(int64_t)) : nullptr;
            c.h_in = rs->s0 > 0 ? rs->h_in : nullptr; c.x_in = rs->x_in; c.h_out = rs->h_out; c.s0 = rs->s0;
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
        TRY(v->stage.upload(G.call, &c, sizeof c, s));
        ArModel &m = models[g];
        m = ArModel{};
        m.Wf_hh12 = v->Wf_hh12; m.Wf_hh16 = v->Wf_hh16; m.bh4 = v->bh4; m.Gemb4 = v->Gemb4; m.Gemb = v->Gemb; m.Wf_fc1 = v->Wf_fc1; m.Wf_fc1h = v->Wf_fc1h; m.b_fc1 = v->b_fc1;
        m.Wf_fc2 = v->Wf_fc2; m.b_fc2 = v->b_fc2; m.mulaw_tab = v->mulaw_tab;
        m.hbuf = G.har.as<float>(); m.a1 = G.a1.as<float>(); m.cand_s = G.cand_s.as<float>(); m.cand_k = G.cand_k.as<int>(); m.cur = G.cur.as<ArSlot>(); m.gcur4 = G.gcur.as<float4>();
        m.gc_replay = d.upsample_t % S == 0;
        const int live = (n_slots - slot0 < Spg ? n_slots - slot0 : Spg) - (nb - 1) * 16;
        m.live_last = live < 1 ? 1 : (live > 16 ? 16 : live);
        m.lead6 = cp.n_grp == 2 && nb <= 2;
        m.candg = G.candg.as<u64>();
        m.abort_dev = (unsigned *)((char *)G.candg.p + cg_bytes);
        m.abort_host = v->status_dev;
        m.timeout_ticks = (unsigned)v->handoff_timeout_ms * 100000u;
        m.dbg_drop_t = v->handoff_debug_drop_step;
        m.fused = (v->fuse_fc2 && !tf && cp.gmax[g] < (1 << CAND_TAG_BITS)) ? 1 : 0;
        m.Hr = Hr; m.Hf = d.Hf; m.n_cls = d.n_cls; m.upsample = d.upsample_t;
    }
    for (int g = 0; g < cp.n_grp; ++g)    // replay 0's slot row and Gcond rows
        hipLaunchKernelGGL(ar_next_row_kernel, dim3(cp.tiles[g] * 16), dim3(256), 0, s, models[g], (const ArCall *)v->grp[g].call);

    HIP_TRY(hipEventRecord(v->ev0, s));
    if (v->use_graph) {
        hipGraphExec_t exec[2] = {nullptr, nullptr};
        for (int g = 0; g < cp.n_grp; ++g) TRY(group_graph(v, g, models[g], cp.tiles[g], tf, &exec[g]));
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
            TRY(launch_ar_steps(v, models[0], v->grp[0].call, cp.tiles[0], S, tf, s));
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

// Shared driver of generate() and logits(): validate and plan on the host, upload the tables and run the conditioning, then
// the decode loop the plan chose.
static int run_ar(vqcpc_vocoder *v, const int64_t *idx, const int64_t *spk, int B, int Tc, const int *n_codes_host,
                  const int64_t *inputs, int Ts, unsigned long long seed, unsigned utt_base,
                  const uint32_t *utt_ids_host, float *wav,
                  int64_t *mulaw, float *logits, int max_steps, hipStream_t s, const NllCall *nc = nullptr) {
    const auto &d = v->d;
    const int Hr = d.Hr, dl = 2 * d.Hp, Lout = d.upsample_t * 2 * Tc;
    CallPlan cp;
    TRY(plan_call(v, B, Tc, n_codes_host, inputs != nullptr, Ts, max_steps, utt_base, utt_ids_host, cp, nc ? nc->slen.data() : nullptr));
    TRY(status_check(v, false));          // has an earlier call's hand-off reported already?  (nothing is cleared without a sync)
    v->epoch = (v->epoch + 1u) & 0xffffffu;
    if (v->epoch == 0) v->epoch = 1;
    // upload through the pinned arena: no synchronisation of the caller's stream
    TRY(v->stage.begin(cp.lens.size() * sizeof(int) + (cp.table[0].size() + cp.table[1].size()) * sizeof(ArSlot) +
                       (size_t)(cp.tiles[0] + cp.tiles[1]) * 16 * sizeof(ArSlot) + 2 * sizeof(ArCall) + 256 +
                       (size_t)8 * XM_BX * (B + 1) * sizeof(XdSeg) + (size_t)3 * (B + 16) * sizeof(int)));
    TRY(v->len.reserve(cp.lens.size() * sizeof(int)));
    TRY(v->stage.upload(v->len.p, cp.lens.data(), cp.lens.size() * sizeof(int), s));
    TRY(v->gbase.reserve(cp.gbase.size() * sizeof(int)));
    TRY(v->stage.upload(v->gbase.p, cp.gbase.data(), cp.gbase.size() * sizeof(int), s));
    const size_t crows = cp.grows > 0 ? (size_t)cp.grows : 1;
    TRY(v->cond.reserve(crows * dl * sizeof(float)));
    TRY(run_condition(v, idx, spk, B, Tc, v->len.as<int>(), v->gbase.as<int>(), (size_t)cp.grows, v->cond.as<float>(), s));
    TRY(v->gcond.reserve(crows * 3 * Hr * sizeof(float)));
    if (cp.grows > 0)
        TRY(vq_gemm_chain(v->cond.as<float>(), dl, v->w_cond, v->b_ih, v->gcond.as<float>(), 3 * Hr, (int)cp.grows, 3 * Hr, dl, dl, s));
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
    VQ_REQUIRE(B > 0 && Tc > 0 && L > 0, "vocoder.nll: need B > 0, Tc > 0 and L > 0 (got %d, %d, %d)", B, Tc, L);
    const auto &d = v->d;
    VQ_REQUIRE(d.Hf == NLL_HF && d.n_cls == NLL_CLS, "vocoder.nll: the scoring head is built for size_h_fc %d and %d classes "
               "(config.py:69,77), this model has %d and %d", NLL_HF, NLL_CLS, d.Hf, d.n_cls);
    hipStream_t s = (hipStream_t)stream;
    NllCall nc{audio, L, std::vector<int>(B, 0), nll, nll_sum, n_scored, n_correct};
    int longest = 0;
    for (int b = 0; b < B; ++b) {
        const int na = n_audio ? n_audio[b] : L, ncd = n_codes ? n_codes[b] : Tc;
        VQ_REQUIRE(na >= 0 && na <= L, "vocoder.nll: n_audio[%d] = %d outside [0, %d]", b, na, L);
        VQ_REQUIRE(ncd >= 0 && ncd <= Tc, "vocoder: n_codes[%d] = %d outside [0, %d]", b, ncd, Tc);
        VQ_REQUIRE((long)na - 1 <= (long)2 * d.upsample_t * ncd, "vocoder.nll: utterance %d has %d samples to score but its %d codes "
                   "cover %ld (n_audio - 1 <= 2 * upsample_t * n_codes)", b, na - 1, ncd, (long)2 * d.upsample_t * ncd);
        nc.slen[b] = na >= 2 ? na - 1 : 0;
        longest = nc.slen[b] > longest ? nc.slen[b] : longest;
    }
    HIP_TRY(hipMemsetAsync(nll_sum, 0, (size_t)B * sizeof(double), s));
    HIP_TRY(hipMemsetAsync(n_scored, 0, (size_t)B * sizeof(int64_t), s));
    HIP_TRY(hipMemsetAsync(n_correct, 0, (size_t)B * sizeof(int64_t), s));
    if (nll && L > 1) HIP_TRY(hipMemsetAsync(nll, 0, (size_t)B * (L - 1) * sizeof(float), s));
    if (longest == 0) return VQCPC_OK;         // no row has two samples: nothing to score
    return run_ar(v, idx, speaker, B, Tc, n_codes, audio, longest, 0, 0, nullptr, nullptr, nullptr, nullptr, 0, s, &nc);
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
    HIP_TRY(hipMemcpyAsync(call, &c, sizeof c, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    const ArModel m = v->last_model;
    const dim3 blk(256);
    const bool tbig = use_big(v, c.nbt);
    const int nf = tbig ? (v->d.n_cls / 16) * c.nbt / 4 : (v->d.n_cls / 16) * c.nbt;   // fused launch: fc2 blocks of step t-1 in front of the GRU blocks of step t
    int fresh = 0;                       // fused launches so far
    for (int which = 0; which < 3; ++which) {
        for (int pass = 0; pass < 2; ++pass) {          // pass 0 = warm-up
            if (pass == 1) HIP_TRY(hipEventRecord(v->ev0, s));
            const int n = pass == 0 ? 20 : reps;
            for (int i = 0; i < n; ++i) {
                if (which == 2) { hipLaunchKernelGGL(ar_fc2_kernel<0>, dim3(v->d.n_cls / 16, c.nbt), blk, 0, s, m, (const ArCall *)call, 0); continue; }
                if (which == 1) { TRY(launch_fc1_step(v, m, call, 0, c.nbt, s)); continue; }
                const int period = c.max_t > 5 ? (c.max_t - 3) / 2 : 1;              // keep t = t_base + tl inside the call (reps beyond
                const int tl = m.fused ? 1 + 2 * (fresh++ % period) : 0;             // that reuse steps, i.e. find their tags in place)
                TRY(launch_gru_step(v, m, call, tl, c.nbt, m.fused ? nf : 0, s));
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
                       v->spk_emb, series, B, Tc, d.dz, d.ds, d.n_codes, d.n_speakers, v->status_dev, v->epoch << 8, nullptr, nullptr);
    v->status_pending = true;
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_condition(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                                       float *cond, void *stream) {
    VQ_REQUIRE(v && idx && speaker && cond && B > 0 && Tc > 0, "vqcpc_vocoder_condition: bad argument");
    return run_condition(v, idx, speaker, B, Tc, nullptr, nullptr, 0, cond, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// streaming decode (vqcpc_vocoder_stream_*): the prenet runs once at open over every utterance's full length (it is
// bidirectional); each chunk is then one call of the decode loop whose utterances RESUME -- at absolute sample pos, from the h
// and x the previous chunk left -- so the chunks concatenate to exactly what one generate() call gives (same Philox counters,
// same conditioning frames, same state).  Chunks plan with xcm = 0: up to xcm_max utterances run on the per-XCD decoders of
// ar_xcd.hip (more than 32 back to back in their slots, each one a resumed segment), beyond that on the launch path.
// ------------------------------------------------------------------------------------------
struct vqcpc_vocoder_stream {
    vqcpc_vocoder *v = nullptr;
    int B = 0, Tc = 0;
    unsigned long long seed = 0;
    std::vector<unsigned> utt;
    std::vector<int> samples, gbase;     // per utterance: samples in all, first conditioning row
    long grows = 0;
    DevBuf cond, gcond, gbase_dev;       // the stream's own prenet output [grows][2Hp] and conditioning rows (W_ih[:, de:] cond + b_ih) [grows][3Hr]
    DevBuf h, x;                         // [2][B][Hr] fp32, [2][B] int: chunk c resumes from half c & 1 and leaves half (c + 1) & 1
    DevBuf owav, omul;                   // (B, n + 1) decode buffers of the chunk in flight
    int64_t pos = 0, total = 0, last_pos = 0;
    int last_n = 0, chunks = 0;
};

// (B, n + 1) decode buffers -> the caller's (B, n) outputs; the row's last class is the next chunk's x_in
__global__ void stream_out_kernel(const float *__restrict__ owav, const int64_t *__restrict__ omul, int B, int n, float *wav,
                                  int64_t *mulaw, int *x_next) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * n) return;
    const size_t b = i / n, j = i % n, src = b * (n + 1) + 1 + j;
    wav[i] = owav[src];
    if (mulaw) mulaw[i] = omul[src];
    if (j == (size_t)n - 1) x_next[b] = (int)omul[src];
}

static int stream_chunk(vqcpc_vocoder_stream *st, int64_t pos, int n, int ci, float *wav, int64_t *mulaw, hipStream_t s) {
    vqcpc_vocoder *v = st->v;
    const auto &d = v->d;
    const int B = st->B, Bp = (B + 15) / 16 * 16, Hr = d.Hr;
    // samples of every utterance in [pos, pos + n); the resident decoders take one priming step in front of them
    std::vector<int> nr(B), res(B);
    for (int b = 0; b < B; ++b) {
        const int64_t left = st->samples[b] - pos;
        nr[b] = left <= 0 ? 0 : (left < n ? (int)left : n);
        res[b] = nr[b] > 0 ? nr[b] + 1 : 0;
    }
    CallPlan cp;
    cp.lens.assign(2 * Bp, 0);
    cp.utt = st->utt; cp.gbase = st->gbase; cp.grows = st->grows;
    const PlanOpts po{v->xcd, 0, v->xcm_max, v->xcm_max, v->xcd_slots, v->xcm_slots, v->n_slots, xd_supported(d.Hr, d.Hf, d.n_cls)};
    VQ_REQUIRE(plan_decode(po, res.data(), cp.utt.data(), longest_first(res.data(), B), cp.dp), "vocoder stream: a decode slot's "
               "schedule does not fit the resident decoders; use more slots or xcd = -1");
    if (cp.dp.path == 0) TRY(plan_launch_tables(v, nr.data(), longest_first(nr.data(), B), false, B, (int)pos, cp));
    TRY(status_check(v, false));
    v->epoch = (v->epoch + 1u) & 0xffffffu;
    if (v->epoch == 0) v->epoch = 1;
    TRY(v->stage.begin((cp.table[0].size() + cp.table[1].size()) * sizeof(ArSlot) + (size_t)(cp.tiles[0] + cp.tiles[1]) * 16 * sizeof(ArSlot) +
                       2 * sizeof(ArCall) + 256 + (size_t)8 * XD_MAX_BX * (B + 1) * sizeof(XdSeg) + (size_t)(B + 16) * sizeof(int)));
    const size_t ob = (size_t)B * (n + 1);
    TRY(st->owav.reserve(ob * sizeof(float)));
    TRY(st->omul.reserve(ob * sizeof(int64_t)));
    HIP_TRY(hipMemsetAsync(st->owav.p, 0, ob * sizeof(float), s));
    HIP_TRY(hipMemsetAsync(st->omul.p, 0, ob * sizeof(int64_t), s));
    const int in = ci & 1, out = (ci + 1) & 1;
    Resume rs{(int)pos, n + 1, st->gcond.as<float>(), st->gbase_dev.as<int>(),
              ci > 0 ? st->h.as<float>() + (size_t)in * B * Hr : nullptr, ci > 0 ? st->x.as<int>() + (size_t)in * B : nullptr,
              st->h.as<float>() + (size_t)out * B * Hr};
    if (v->last_path != 0) v->last_path = 1;      // a chunk that fails from here on ran no decode loop
    if (cp.dp.path != 0) TRY(run_resident(v, cp, 2 * st->Tc, st->seed, st->owav.as<float>(), st->omul.as<int64_t>(), s, &rs));
    else TRY(run_launch_path(v, cp, nullptr, 2 * st->Tc, 0, st->seed, st->owav.as<float>(), st->omul.as<int64_t>(), nullptr, s, &rs));
    hipLaunchKernelGGL(stream_out_kernel, dim3((unsigned)(((size_t)B * n + 255) / 256)), dim3(256), 0, s, st->owav.as<float>(),
                       st->omul.as<int64_t>(), B, n, wav, mulaw, st->x.as<int>() + (size_t)out * B);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_stream_open(vqcpc_vocoder *v, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                                         const int *n_codes, uint64_t seed, uint32_t utt_base, const uint32_t *utt_ids,
                                         vqcpc_vocoder_stream **out, void *stream) {
    VQ_REQUIRE(v && idx && speaker && out, "vqcpc_vocoder_stream_open: null argument");
    VQ_REQUIRE(B > 0 && Tc > 0, "vocoder stream: need B > 0 and Tc > 0 (got %d, %d)", B, Tc);
    *out = nullptr;
    const auto &d = v->d;
    const int Bp = (B + 15) / 16 * 16, dl = 2 * d.Hp, Hr = d.Hr;
    hipStream_t s = (hipStream_t)stream;
    vqcpc_vocoder_stream *st = new vqcpc_vocoder_stream();
    st->v = v; st->B = B; st->Tc = Tc; st->seed = seed;
    st->total = (int64_t)2 * d.upsample_t * Tc;
    std::vector<int> lens(2 * Bp, 0);
    st->utt.resize(B); st->samples.resize(B); st->gbase.assign(Bp, 0);
    int rc = VQCPC_OK;
    DevBuf &cond = st->cond;
    auto fail = [&](int code) { vqcpc_vocoder_stream_close(st); return code; };
    for (int b = 0; b < B; ++b) {
        const int nc = n_codes ? n_codes[b] : Tc;
        if (nc < 0 || nc > Tc) { vq_set_error("vocoder stream: n_codes[%d] = %d outside [0, %d]", b, nc, Tc); return fail(VQCPC_ERR_INVALID); }
        lens[b] = 2 * nc;
        st->samples[b] = d.upsample_t * 2 * nc;
        st->utt[b] = utt_ids ? utt_ids[b] : utt_base + (unsigned)b;
        st->gbase[b] = (int)st->grows;
        st->grows += 2 * nc;
    }
    if (st->grows >= (1L << 31)) { vq_set_error("vocoder stream: %ld conditioning frames", st->grows); return fail(VQCPC_ERR_INVALID); }
    const size_t crows = st->grows > 0 ? (size_t)st->grows : 1;
#define STRY(x) do { rc = (x); if (rc != VQCPC_OK) return fail(rc); } while (0)
    STRY(status_check(v, false));
    v->epoch = (v->epoch + 1u) & 0xffffffu;
    if (v->epoch == 0) v->epoch = 1;
    STRY(v->stage.begin(lens.size() * sizeof(int) + st->gbase.size() * sizeof(int) + 64));
    STRY(v->len.reserve(lens.size() * sizeof(int)));
    STRY(v->stage.upload(v->len.p, lens.data(), lens.size() * sizeof(int), s));
    STRY(st->gbase_dev.reserve(st->gbase.size() * sizeof(int)));
    STRY(v->stage.upload(st->gbase_dev.p, st->gbase.data(), st->gbase.size() * sizeof(int), s));
    STRY(cond.reserve(crows * dl * sizeof(float)));
    STRY(run_condition(v, idx, speaker, B, Tc, v->len.as<int>(), st->gbase_dev.as<int>(), (size_t)st->grows, cond.as<float>(), s));
    STRY(st->gcond.reserve(crows * 3 * Hr * sizeof(float)));
    if (st->grows > 0)
        STRY(vq_gemm_chain(cond.as<float>(), dl, v->w_cond, v->b_ih, st->gcond.as<float>(), 3 * Hr, (int)st->grows, 3 * Hr, dl, dl, s));
    STRY(st->h.reserve((size_t)2 * B * Hr * sizeof(float)));
    STRY(st->x.reserve((size_t)2 * B * sizeof(int)));
#undef STRY
    *out = st;
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_stream_next(vqcpc_vocoder_stream *st, int n_samples, float *wav, int64_t *mulaw, void *stream) {
    VQ_REQUIRE(st && wav, "vqcpc_vocoder_stream_next: null argument");
    const int up = st->v->d.upsample_t;
    VQ_REQUIRE(n_samples > 0 && n_samples % up == 0, "vocoder stream: n_samples = %d must be a positive multiple of %d", n_samples, up);
    VQ_REQUIRE(st->pos < st->total, "vocoder stream: all %lld samples have been decoded", (long long)st->total);
    TRY(stream_chunk(st, st->pos, n_samples, st->chunks, wav, mulaw, (hipStream_t)stream));
    st->last_pos = st->pos; st->last_n = n_samples;
    st->chunks += 1;
    st->pos = st->pos + n_samples < st->total ? st->pos + n_samples : st->total;
    return VQCPC_OK;
}

extern "C" int vqcpc_vocoder_stream_redo(vqcpc_vocoder_stream *st, float *wav, int64_t *mulaw, void *stream) {
    VQ_REQUIRE(st && wav, "vqcpc_vocoder_stream_redo: null argument");
    VQ_REQUIRE(st->chunks > 0, "vocoder stream: no chunk to repeat");
    return stream_chunk(st, st->last_pos, st->last_n, st->chunks - 1, wav, mulaw, (hipStream_t)stream);
}

extern "C" int vqcpc_vocoder_stream_position(const vqcpc_vocoder_stream *st, int64_t *done, int64_t *total) {
    VQ_REQUIRE(st && done && total, "vqcpc_vocoder_stream_position: null argument");
    *done = st->pos; *total = st->total;
    return VQCPC_OK;
}

extern "C" void vqcpc_vocoder_stream_close(vqcpc_vocoder_stream *st) {
    if (!st) return;
    for (DevBuf *b : {&st->cond, &st->gcond, &st->gbase_dev, &st->h, &st->x, &st->owav, &st->omul}) b->release();
    delete st;
}
