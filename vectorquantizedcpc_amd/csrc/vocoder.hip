// vocoder.hip -- the launch-per-step sample loop of Vocoder.generate / Vocoder.forward on gfx950: its kernels and their
// launchers (interface: ar_step.h).  The handle, conditioning and dispatch are in vocoder_host.hip, the decode planner in
// vocoder_plan.hip, the streaming decode in vocoder_stream.hip.  (Reference call sites network_vocoder.py:41-78; the RNN_MS
// arithmetic is the project's spec of the absent third-party `rnnms` package -- see oracle/vqcpc_oracle.c and DESIGN.md.)
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
#include "ar_step.h"
#include <math.h>

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
int build_wfrag12(const float *W, int ldw, int n_rg, int K, int H, DevBuf &out, hipStream_t s) {
    VQ_REQUIRE(K % 64 == 0 && ldw % 4 == 0, "build_wfrag12: K=%d not a multiple of 64", K);
    const size_t n4 = (size_t)n_rg * (K / 16) * 48;
    TRY(out.reserve(n4 * sizeof(float4)));
    hipLaunchKernelGGL(build_wfrag12_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, W, ldw, out.as<float>(), n_rg, K, H);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

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
        if (cd.s[q].x > best) { best = cd.s[q].x; k = cd.k[q].x; }      // first_max, written out
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
                ok &= cand_tag(gv[q]) == tag;
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
            const float sq = cand_score(gv[q]);
            if (!gave_up && sq > best) { best = sq; xf = cand_class(gv[q]); }      // first_max, written out
        }
    }
    return xf;
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
        float v = sum4(red[0][rr][bb], red[1][rr][bb], red[2][rr][bb], red[3][rr][bb]);
        v += bias;
        v = v > 0.f ? v : 0.f;
        const size_t at = hl_index(m.Hf, bt * 16 + bb, row);
        m.a1[at] = v;
    }
}

// fc2 over one 16-class row group + its Gumbel-max candidate per utterance, for local step `ts` (Hf = 256: SW = 4).
// Used by ar_fc2_kernel (plain candidate arrays) and by the fused launch (granules).  All threads of the workgroup must
// call it (two barriers); threads >= 256 only take part in those.
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
    const XdSeg sl = m.cur[bg];
    const int lt = t - sl.t0;
    // noise of (class, utterance, sample) while the loads fly
    const float g = draw_noise((unsigned)lt, sl.utt, (unsigned)cls, c.seed);
    const bool live = ts >= 0 && t < c.max_t && sl.row >= 0 && lt >= 0 && lt < sl.len;
    __builtin_amdgcn_sched_barrier(0);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0;;) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {                                    // mfma_k4, written out
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
        float v = sum4(red[0][rr][bb], red[1][rr][bb], red[2][rr][bb], red[3][rr][bb]);
        v += bias;
        if (c.logits && live) c.logits[((size_t)sl.row * c.Ts + lt) * m.n_cls + cls] = v;
        sc[rr][bb] = v + g;
    }
    __syncthreads();
    if (worker && tid < 16 && live) {
        float best = sc[0][bb];
        int k = 0;
#pragma unroll
        for (int r = 1; r < 16; ++r) first_max(best, k, sc[r][bb], r);
        if (GRANULES) {
            const unsigned tag = (unsigned)(t + 1) & ((1u << CAND_TAG_BITS) - 1u);
            if (!(m.dbg_drop_t >= 0 && t == m.dbg_drop_t && rg == 3 && bt == 0))
            ps_store(m.candg + ((size_t)(bt * nrg + rg) * 16 + bb), cand_pack(tag, (unsigned)(16 * rg + k), best));
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
        float ge[3] = {0.f, 0.f, 0.f}, gc[3] = {0.f, 0.f, 0.f}, bh[3] = {0.f, 0.f, 0.f}, hold = 0.f;
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
                for (int q = 0; q < NB; ++q) {                           // mfma_k4, written out
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
            const XdSeg sl = m.cur[sg];
            const ArCall c = *cp;
            const float4 bq = m.bh4[rg * 4 + u];
            hi = hl_index(Hr, sg, unit);
            const float hprev = hin[hi];
            const float4 gq = m.gcur4[((size_t)rg * (nbt * 16) + sg) * 4 + u];     // no branch around loads: gcur4 always exists
            bh[0] = bq.x; bh[1] = bq.y; bh[2] = bq.z;
            gc[0] = gq.x; gc[1] = gq.y; gc[2] = gq.z;
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
                ge[0] = eq.x; ge[1] = eq.y; ge[2] = eq.z;
                if (!m.gc_replay) {
                    const float *pg = c.Gcond + ((size_t)c.gbase[sl.row] + lt / m.upsample) * 3 * Hr + unit;
                    gc[0] = pg[0]; gc[1] = pg[Hr]; gc[2] = pg[2 * Hr];
                }
                hold = first ? 0.f : hprev;                     // a new utterance starts from h = 0
                if (c.hall) hallp = c.hall + ((size_t)sl.row * c.CH + (lt - c.hall_t0)) * Hr + unit;
            }
            if (rg == 0 && wave == 0) ((float4 *)mt)[lane] = mtl;
            AR_STAMP(tid == 0, 0, 2);
        }
        __syncthreads();
        // cell update (PyTorch GRUCell equations, gate order r, z, n), K quarters summed in fixed order
        if (emit) {                                  // the sample the candidates decided
            if (wavp) *wavp = m.n_cls <= 256 ? mt[xraw] : m.mulaw_tab[xraw];      // emit_sample with the table picked per store
            if (mulp) *mulp = xraw;
        }
        if (active) {
            // the slot's previous occupant left its state in the MFMA operand: W_hh . 0 = 0 on a first step
            const float gr = first ? 0.f : sum4(red[g][0][u][b], red[g][1][u][b], red[g][2][u][b], red[g][3][u][b]);
            const float gz = first ? 0.f : sum4(red[g][0][4 + u][b], red[g][1][4 + u][b], red[g][2][4 + u][b], red[g][3][4 + u][b]);
            const float gn = first ? 0.f : sum4(red[g][0][8 + u][b], red[g][1][8 + u][b], red[g][2][8 + u][b], red[g][3][8 + u][b]);
            const float r = gate_sigmoid((ge[0] + gc[0]) + (gr + bh[0]));      // gru_cell, written out
            const float z = gate_sigmoid((ge[1] + gc[1]) + (gz + bh[1]));
            const float n = gate_tanh((ge[2] + gc[2]) + r * (gn + bh[2]));
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
        const XdSeg sl = m.cur[sg];
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
                    if (c.wav) c.wav[(size_t)sl.row * c.Lout + lt - 1] = m.mulaw_tab[x];      // emit_sample, written out
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
                const float gr = first ? 0.f : sum4(red[q][0][0][ul][b], red[q][0][1][ul][b], red[q][0][2][ul][b], red[q][0][3][ul][b]);
                const float gz = first ? 0.f : sum4(red[q][1][0][ul][b], red[q][1][1][ul][b], red[q][1][2][ul][b], red[q][1][3][ul][b]);
                const float gn = first ? 0.f : sum4(red[q][2][0][ul][b], red[q][2][1][ul][b], red[q][2][2][ul][b], red[q][2][3][ul][b]);
                const float rr = gate_sigmoid((ge[p][0] + gc[p][0]) + (gr + bh[p][0]));      // gru_cell, written out
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
            for (int s = 0; s < SW; ++s) {                               // mfma_k4, written out
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
        const XdSeg pv = c.slots[(size_t)(r - 1) * c.Sp + sg];
        const int end = pv.t0 + pv.len;
        if (pv.row >= 0 && end > c.t_base - c.S && end <= c.t_base) {
            const float *hb = m.hbuf + (size_t)(end & 1) * c.nbt * m.Hr * 16;
            for (int k = threadIdx.x; k < m.Hr; k += 256) c.h_out[(size_t)pv.row * m.Hr + k] = hb[hl_index(m.Hr, sg, k)];
        }
        __syncthreads();
    }
    if (r >= c.n_rep) return;
    XdSeg sl = c.slots[(size_t)(c.one_row ? 0 : r) * c.Sp + sg];
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
                m.candg[((size_t)(sg >> 4) * nrg + q) * 16 + (sg & 15)] = cand_pack(tag, (unsigned)x, 0.f);
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


// End of every replay: an utterance whose last sample fell inside this replay still has that sample
// only as candidates (the next GRU step would have merged them): emit it before the slot is reused.
__global__ void ar_finalize_kernel(ArModel m, const ArCall *__restrict__ cp) {
    const int sg = blockIdx.x * blockDim.x + threadIdx.x;
    const ArCall c = *cp;
    if (sg >= c.Sp || c.inputs) return;
    const XdSeg sl = m.cur[sg];
    if (sl.row < 0) return;
    const int end = sl.t0 + sl.len;
    if (end <= c.t_base || end > c.t_base + c.S) return;
    float best;
    int x;
    const int nrg = m.n_cls >> 4;
    if (m.fused) {
        const u64 *cg = m.candg + ((size_t)(sg >> 4) * nrg) * 16 + (sg & 15);
        u64 gq = ps_load(cg);
        best = cand_score(gq);
        x = cand_class(gq);
        for (int q = 1; q < nrg; ++q) {
            gq = ps_load(cg + q * 16);
            first_max(best, x, cand_score(gq), cand_class(gq));
        }
    } else {
        best = m.cand_s[(size_t)sg * nrg];
        x = m.cand_k[(size_t)sg * nrg];
        for (int q = 1; q < nrg; ++q) first_max(best, x, m.cand_s[(size_t)sg * nrg + q], m.cand_k[(size_t)sg * nrg + q]);
    }
    emit_sample(c.wav, c.mulaw, (size_t)sl.row * c.Lout + sl.len - 1, x, m.mulaw_tab);
}

// Hidden sizes the per-sample kernels are instantiated for (size_h_rnn = 64 SW): 512, 896 (the reference's, config.py:76), 1024.
// (Round 2 compiled nine values x every variant = ~190 kernels; a size outside the list is an explicit error at create.)
#define AR_SW_CASES(X) X(8) X(14) X(16)

static size_t big_lds_bytes(int Hr) { return (size_t)2 * Hr * 16 * sizeof(float) + (size_t)2 * 3 * 4 * 16 * 17 * sizeof(float); }
bool use_big(const ArStep &a, int nbt) {
    return a.big_min_tiles > 0 && nbt >= a.big_min_tiles && a.Hr % 16 == 0 && big_lds_bytes(a.Hr) <= 160 * 1024;
}
// One GRU-step launch for local step `tl`; nf = fc2 blocks of the previous step in front (fused launch, 0 = none).
int launch_gru_step(const ArStep &a, const ArModel &m, const ArCall *call, int tl, int nbt, int nf, hipStream_t s) {
    const int Hr = a.Hr, rgs = Hr / 4, npass = (nbt + 1) / 2;
    const bool big = use_big(a, nbt);
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
int launch_fc1_step(const ArStep &a, const ArModel &m, const ArCall *call, int tl, int nbt, hipStream_t s) {
    const dim3 blk(256);
    switch (a.Hr / 64) {
#define CASE(k) case k: \
        if (nbt <= 4) hipLaunchKernelGGL((ar_fc1_kernel<k, 8>), dim3(a.Hf / 8, nbt), blk, 0, s, m, call, tl, nbt); \
        else hipLaunchKernelGGL((ar_fc1_kernel<k, 16>), dim3(a.Hf / 16, nbt), blk, 0, s, m, call, tl, nbt); \
        break;
        AR_SW_CASES(CASE)
#undef CASE
        default: vq_set_error("AR step: size_h_rnn %d unsupported", a.Hr); return VQCPC_ERR_INVALID;
    }
    return VQCPC_OK;
}

void launch_fc2_step(const ArStep &a, const ArModel &m, const ArCall *call, int tl, int nbt, hipStream_t s) { hipLaunchKernelGGL(ar_fc2_kernel<0>, dim3(a.n_cls / 16, nbt), dim3(256), 0, s, m, call, tl); }
void launch_next_row(const ArModel &m, const ArCall *call, int nbt, hipStream_t s) { hipLaunchKernelGGL(ar_next_row_kernel, dim3(nbt * 16), dim3(256), 0, s, m, call); }

// tf: teacher-forced scan -- x_{t-1} comes from the inputs, so only the GRU step runs per sample (fc1 / fc2 follow
// as batched GEMMs over the whole chunk, run_launch_path in vocoder_host.hip)
int launch_ar_steps(const ArStep &a, const ArModel &m, ArCall *call, int nbt, int n, bool tf, hipStream_t s) {
    const bool big = use_big(a, nbt);
    if (big && !*a.big_attr_set) {
        switch (a.Hr / 64) {
#define CASE(k) case k: HIP_TRY(hipFuncSetAttribute((const void *)ar_gru_big_kernel<k, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds_bytes(a.Hr))); \
                        HIP_TRY(hipFuncSetAttribute((const void *)ar_gru_big_kernel<k, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)big_lds_bytes(a.Hr))); break;
            AR_SW_CASES(CASE)
#undef CASE
            default: break;
        }
        *a.big_attr_set = true;
    }
    // Fused schedule (m.fused): step i = { fc2 of step i-1  ||  GRU of step i } in ONE launch, then fc1 of step i; the
    // fc2 of the replay's last step runs as a trailing launch (before the slot records change), so the first launch of a
    // replay carries no fc2 blocks.  (fc1 in the same launch as well -- one launch per sample -- was built and measured in
    // round 2 and loses at every batch size: profiles/r02_gru_variants_one_launch.csv; removed.)
    const int f2_full = big ? (a.n_cls / 16) * nbt / 4 : (a.n_cls / 16) * nbt;
    for (int i = 0; i < n; ++i) {
        TRY(launch_gru_step(a, m, call, i, nbt, (m.fused && i > 0) ? f2_full : 0, s));
        if (tf) continue;
        TRY(launch_fc1_step(a, m, call, i, nbt, s));
        if (!m.fused) launch_fc2_step(a, m, call, i, nbt, s);
    }
    if (!tf && m.fused) hipLaunchKernelGGL(ar_fc2_kernel<1>, dim3(a.n_cls / 16, nbt), dim3(256), 0, s, m, (const ArCall *)call, n - 1);
    if (!tf) hipLaunchKernelGGL(ar_finalize_kernel, dim3((nbt * 16 + 63) / 64), dim3(64), 0, s, m, (const ArCall *)call);
    hipLaunchKernelGGL(ar_advance_kernel, dim3(1), dim3(1), 0, s, call, n);
    launch_next_row(m, call, nbt, s);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
