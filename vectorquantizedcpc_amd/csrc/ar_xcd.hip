// ar_xcd.hip -- the WaveRNN-style sample loop of Vocoder.generate (network_vocoder.py:78; RNN_MS spec: DESIGN.md 2.2) as
// EIGHT independent, weight-stationary, resident decoders: one per XCD.
//
// Utterances are independent, so they are dealt over the 8 XCDs (decode slot s lives on XCD s % 8) and each XCD runs its
// own copy of the recurrence on its 32 CUs, with a full copy of the weights held ON the CUs for the whole call:
//   * workgroup `rank` (0..31, one per CU, 768 threads) owns hidden units 28 rank .. 28 rank + 27 = 84 gate rows of W_hh
//     (80 of them in VGPRs, 112 weights per lane = one fp32 fma chain of the row; the last 4 in LDS), 8 rows of fc1 and
//     8 classes of fc2 (36.9 KB, LDS) and its slice of the sample-embedding table Gemb (86 KB, LDS);
//   * nothing is re-fetched per sample: after the prologue the only global traffic is the three all-to-all exchanges of a
//     sample step (h_t, a_t, the draw candidates) as 8-byte {tag, value} granules (the data is the flag), which stay
//     inside the XCD: published with workgroup-scope stores (the write-through L1 leaves them in the XCD's L2) and swept
//     with sc1 loads that bypass L1 -- 0.41 us per exchange against 1.2 us across XCDs
//     (profiles/r02_xcd_exchange_microbench.csv).  The placement is CHECKED, not assumed: every workgroup reads its
//     XCC_ID and takes a ticket; unless each XCD got exactly 32 workgroups the launch gives up (STATUS_MISPLACED) before it
//     touches any output, and the host falls back to the launch-per-step kernels.
// Arithmetic is bit-identical to those kernels: a row's dot product is the same 8 fp32 fma chains (K quarter x x/z|y/w
// accumulator: ar_shared.h), combined in the same order; cell update, fc epilogues and the Gumbel-max draw are the
// same expressions.  A chain lives in ONE lane; the four lanes of a quad hold the same chain of four different rows.
// With ONE or TWO slots per XCD (ar_xcd_kernel<1>, <2>) the quad shares a chain's operand values (each lane loads a quarter of
// h from LDS, v_fmac_f32_dpp quad_perm broadcasts them): a quarter of the LDS operand traffic, one vector instruction per term,
// row and slot.  With FOUR slots per XCD (ar_xcd_kernel<4>, 17..32 utterances) the same chains run on the matrix pipe:
// v_mfma_f32_4x4x1_16B_f32 advances a quad's four rows for the four slots in one instruction (ar_chain.h) -- the vector form was
// vector-ALU bound between the barriers at four slots (3.5 of 5.1 us; profiles/r04_ablation.txt, r04_mfma_chains.txt).
//
// Roles of the 12 waves of a workgroup (the two service waves are waves 0 and 1, the OLDEST of their SIMDs: the instruction
// arbiter serves the oldest wave first -- ar_xcm.hip has the measurements -- and what they do is the critical path; as waves
// 11 / 10 the single-utterance step took 2.90 us, as waves 0 / 1 it takes 2.82):
//   waves 2..11  (chain waves 0..9) W_hh h_t chains of rows 0..79 for every slot of the XCD (8 rows per wave, weights pinned
//                in VGPRs) -> gsum
//   chain wave b < bx  also: sweep of a_t of slot b, fc2 + Gumbel-max candidate of the 8 owned classes -> publish (between its
//                W_hh chains: one slot per wave, in parallel)
//   wave 1       with ONE slot per XCD (up to 8 utterances): fc1 with its 8 rows pinned like a chain wave's (2.82 -> 2.54 us per step)
//   wave 0 / 1   what else is serial in a sample step, for the even / odd slots: cell update of the 28 owned units; publish
//                h_t; the slot's state for the next step in the shadow of the h_t exchange; fc1 (weights streamed from LDS)
//                -> publish a_t; W_hh rows 80..83 for the OTHER wave's slots (one chain pass: a half wave per slot); the
//                next step's Gumbel noise (Philox + two logs per class); x_t from the slot's 32 candidates, picked up
//                before barrier B
//   all waves    sweep h_t into LDS (four slots: the chain waves only, which publish nothing and nap first -- XD_HNAP -- so that their
//                first round is not issued before the data can exist)
// Exchange regions of an XCD (ar_chain.h): h_t [rank][slot][32 units], swept with 8-byte loads; a_t [slot][rank][8] -- a slot's 256
// granules in one run, which a lane of the slot's fc2 wave takes as two 16-byte loads of two granules each; candidates [slot][rank].
// Every granule is published by one 8-byte store and validated by its own tag, whatever the width of the load that fetched it.
// Four slots per XCD: h_t travels as 4-byte WORDS instead -- the value's bits with bit 30, which |h| < 2 leaves free, replaced by the
// step's parity (ar_shared.h: xd_word_h, and why one bit is enough).  A (rank, slot) pair is one 128-byte line, a publisher's half wave
// still writes one contiguous run (112 bytes), and a sweeping lane takes a 16-byte chunk of four units with ONE global_load_dwordx4,
// each word validated by its own bit: 14.3 KB per CU and step instead of 28.7, one load instruction per chain wave instead of four.
// The chain waves take all of it (XD_SVC_SWEEP below).  A hidden value the word cannot carry ends the call (STATUS_RANGE).  a_t can
// be built the same way (XD_WORDS_A, ar_chain.h) and is not: it measured slower.
// Four slots per XCD, what differs: every wave runs ONE dependent chain of 112 matrix instructions per step (waves 2..11 rows
// 0..79 with pinned weights, wave 0 fc1 for all four slots -- its four accumulators combined, biased, rectified and stored together
// (fc1_finish4, xd_put4) -- and wave 1 W_hh rows 80..83, both with weights streamed from LDS);
// fc2 + draw of slots 0..3 on waves 2, 3, 6, 7; waves 4 and 8 -- fc1's SIMD mates -- start their chains when a_t is out (two
// dependent-chain waves keep a SIMD's issue port ~80 % busy, whatever s_setprio says); wave 11 draws the next step's noise
// behind its chain from the slots' clocks the service waves post in LDS.
// Two workgroup barriers per sample.  Every wait is wall-clock bounded; a timeout sets STATUS_TIMEOUT, every workgroup
// leaves, and the call's outputs are incomplete (vqcpc_vocoder_check reports it).
#include "ar_xcd.h"
#include "ar_shared.h"

// Timeline stamps of worker 5 of XCD 0 (100 MHz wall clock), steps 256..383, for tools/xcd_timeline.py: compiled in only
// with -DVQCPC_XD_STAMPS (a debug build under build/stamps/, never the shipped library).
#ifdef VQCPC_XD_STAMPS
__device__ unsigned long long g_xd_stamps[128 * 16];
#define XD_STAMP(wv, i) do { if (rank == 5 && xcc == 0 && wave == (wv) && lane == 0 && t >= 256 && t < 384) \
        g_xd_stamps[(t - 256) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int vqcpc_debug_xd_stamps(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xd_stamps), sizeof(g_xd_stamps)) == hipSuccess ? 0 : -1;
}
// per-worker stamps of XCD 0 (slot 0's events on every worker): [event][worker][step 256..383]
__device__ unsigned long long g_xd_workers[6 * 32 * 128];
#define XD_WSTAMP(ev) do { if (xcc == 0 && lane == 0 && t >= 256 && t < 384) \
        g_xd_workers[((ev) * 32 + rank) * 128 + (t - 256)] = __builtin_amdgcn_s_memrealtime(); } while (0)
extern "C" int vqcpc_debug_xd_workers(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xd_workers), sizeof(g_xd_workers)) == hipSuccess ? 0 : -1;
}
#else
#define XD_STAMP(wv, i) do { } while (0)
#define XD_WSTAMP(ev) do { } while (0)
#endif
// -DVQCPC_XD_BARS (alone: the stamps above perturb what these measure)
#ifdef VQCPC_XD_BARS
// every wave of worker 5 of XCD 0 at the two barriers of a step: [step 256..383][wave][arrives at A, leaves A, arrives at B, leaves B]
__device__ unsigned long long g_xd_bars[128 * 12 * 4];
// (the arrival time waits in a register and is stored behind the barrier: a store in front of it would be waited for by the
// barrier's release fence, and the barrier would look as long as a store takes)
#define XD_BARRIVE() do { xd_arrived = __builtin_amdgcn_s_memrealtime(); } while (0)
#define XD_BLEAVE(i) do { if (rank == 5 && xcc == 0 && lane == 0 && t >= 256 && t < 384) { \
        g_xd_bars[((t - 256) * 12 + wave) * 4 + (i)] = xd_arrived; \
        g_xd_bars[((t - 256) * 12 + wave) * 4 + (i) + 1] = __builtin_amdgcn_s_memrealtime(); } } while (0)
extern "C" int vqcpc_debug_xd_bars(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xd_bars), sizeof(g_xd_bars)) == hipSuccess ? 0 : -1;
}
#else
#define XD_BARRIVE() do { } while (0)
#define XD_BLEAVE(i) do { } while (0)
#endif

// -DVQCPC_XD_POLLS (alone): rounds of the three exchange polls, every wave of worker 5 of XCD 0, summed over steps 256..383, for
// tools/xcd_polls.py: [wave][h_t sweep, a_t poll, candidate poll][failed rounds, all rounds].  Each wave adds to words of its own.
#ifdef VQCPC_XD_POLLS
__device__ unsigned g_xd_polls[12 * 3 * 2];
#define XD_POLLS(ex, failed) do { if (rank == 5 && xcc == 0 && lane == 0 && t >= 256 && t < 384) { \
        g_xd_polls[(wave * 3 + (ex)) * 2] += (failed); g_xd_polls[(wave * 3 + (ex)) * 2 + 1] += (failed) + 1u; } } while (0)
// reads the counters and clears them for the next call
extern "C" int vqcpc_debug_xd_polls(unsigned *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_xd_polls), sizeof(g_xd_polls)) != hipSuccess) return -1;
    void *d = nullptr;
    return hipGetSymbolAddress(&d, HIP_SYMBOL(g_xd_polls)) == hipSuccess && hipMemset(d, 0, sizeof(g_xd_polls)) == hipSuccess ? 0 : -1;
}
#else
#define XD_POLLS(ex, failed) do { } while (0)
#endif

#include "ar_chain.h"

// Ablation of the exchange WAITS, for timing only (results are garbage: stale granules are used as they are found): bit 0 the
// candidate poll, bit 1 the a_t poll, bit 2 the h_t sweep take whatever their first load returns.  What a step still costs then
// is what the workgroup's own instruction streams, LDS traffic, L2 round trips and barriers cost -- profiles/r04_ablation.txt.
// Never set in the shipped library (tools/build_variant.sh A7 "-DXD_ABLATE=7"; tools/ab_libs.py times the builds).
#ifndef XD_ABLATE
#define XD_ABLATE 0
#endif
// four slots per XCD: groups of 8 terms (of 14) a chain wave runs before it turns to fc2 of its slot
#ifndef XD_GSPLIT
#define XD_GSPLIT 10
#endif
// four slots per XCD: groups of 8 terms the service waves' chains request ahead (weights and operands both come from LDS)
#ifndef XD_DEPTH
#define XD_DEPTH 3
#endif
// four slots per XCD: the two chain waves on fc1's SIMD start their chains when a_t is out (0: at once -- A/B builds, profiles/r04_mfma_chains.txt)
#ifndef XD_HOLD
#define XD_HOLD 1
#endif
// four slots per XCD: the chain waves, which publish no h_t, nap XD_HNAP x 64 clocks behind barrier B before the first round of their
// h_t sweep (0: none -- A/B builds).  A round issued at B is answered by L2 before any worker has stored (the service waves publish
// 0.33 us later): it is lost by construction -- 1.0 failed round per chain wave and step, 10 x 2 KB of loads per workgroup on the path the
// publishers' stores travel -- and the second round can start only when the first is back.  With the nap the first round finds everything
// (0.00 failed rounds) and the step is 0.04..0.056 us shorter.  The optimum is sharp: 8 / 10 / 12 / 14 / 17 gave 3.23 / 3.21 / 3.24 / 3.27 / 3.34 us
// against 3.26 without; the load must be on its way BEFORE the workgroup's own h_t is out -- waiting for a word in LDS that says so, with or
// without a nap around it, gave the gain back (profiles/r14_ab_poll_gates.txt).  A timing hint only: every granule is validated by its tag.
// One and two slots per XCD: no gain (the same file), so those kernels do not nap.
#ifndef XD_HNAP
#define XD_HNAP 10
#endif
// four slots per XCD, words: who sweeps h_t.  XD_SVC_SWEEP 0: the service waves do not -- between their h_t store and barrier A they are the
// last of the workgroup (they publish, post the next step's state and only then would load), so every chunk they take, with its
// validation and its LDS stores, is on the step's critical path; the ten chain waves, which wait behind their nap anyway, take all
// 896 chunks: one per thread, and the threads of waves XD_HX .. XD_HX + 3 a second one.  1: every thread takes one chunk and the
// threads of waves XD_HX, XD_HX + 1 a second (XD_HX 0: the granules' shape).  At 32 utterances, us per step: granules 3.21;
// words with the service waves' two chunks each 3.18; their second chunk on waves 10 / 11 instead 3.12; no sweep on the service
// waves and the second chunks on waves 2..5 / 4..7 / 6..9 / 8..11: 3.05 / 3.15 / 3.14 / 3.12 (profiles/r15_ab_exchange_words.txt).
#ifndef XD_SVC_SWEEP
#define XD_SVC_SWEEP 0
#endif
#ifndef XD_HX
#define XD_HX 2
#endif

namespace {

// LDS carve, in floats (ints behind them)
template <int BXT> struct Lds {
    static constexpr int gemb = 0;                        // [NC][3][UPB]   slice of the sample-embedding table
    static constexpr int fc1w = gemb + NC * ROWS;         // [28 words][64 lane-chains (row r8, chain cid)][4]: word-interleaved (chain_lds2)
    static constexpr int fc2w = fc1w + FPB * HR;          // [8 words][64 lane-chains][4]
    static constexpr int whx = fc2w + FPB * HF;           // [28 words][32 lane-chains][4]  W_hh rows 80..83 (the chain waves hold rows 0..79)
    static constexpr int HS = BXT == 4 ? HS4 : HR;        // slot stride of h_t (four slots: the matrix-pipe chains' copy, ar_chain.h)
    static constexpr int hc = whx + 4 * HR;               // [BXT][HS]  h_t, chain by chain (dpp chains: phase order; matrix pipe: term order)
    static constexpr int ac = hc + BXT * HS;              // [BXT][8 chains][AS]  a_t (32 terms per chain, chain stride AS = 48: bank windows)
    static constexpr int gsum = ac + BXT * 8 * 48;            // [BXT][96]  W_hh h of the owned rows [gate][unit]
    static constexpr int noise = gsum + BXT * 96;         // [2][BXT][8] Gumbel noise of the step in flight / the next one
    static constexpr int mtab = noise + 2 * BXT * 8;      // [NC] mu-law decode table
    static constexpr int bq = mtab + NC;                  // [3][32] b_hh of the owned units
    static constexpr int seg = bq + 96;                   // int [BXT][8] {index, row, t0, len, utt, samples into / index of the conditioning frame, first Gcond row}
    static constexpr int sinfo = seg + BXT * 8;           // int [BXT][2] {lt, utt} of the NEXT step, posted by advance() (four slots: chain wave 9 draws the noise)
    static constexpr int ctl = sinfo + BXT * 2;           // int [8] {xcc, rank, ok, abort, the call's status tag}
    static constexpr int total = ctl + 8;
};

// RESUME: every segment is a chunk of a stream (XdResume, ar_xcd.h): a priming step, then its samples from (h_in, x_in, s0).  The
// one-shot kernels ar_xcd_kernel<BXT> are the RESUME = false copies and do not contain that code; ar_xcd_resume_kernel<BXT> the others.
template <int BXT, bool RESUME>
__device__ __forceinline__ void xcd_decoder(const XdParams &p, const XdResume &rp) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    using L = Lds<BXT>;
    constexpr bool W = xd_words_h(BXT), WA = xd_words_a(BXT);      // h_t / a_t travel as 4-byte words (ar_shared.h), not as 8-byte granules
    float *gemb = smem + L::gemb, *fc1w = smem + L::fc1w, *fc2w = smem + L::fc2w, *whx = smem + L::whx, *hc = smem + L::hc,
          *ac = smem + L::ac, *gsum = smem + L::gsum;
    float *noise = smem + L::noise, *mtab = smem + L::mtab, *c_bq = smem + L::bq;
    int *seg_st = (int *)(smem + L::seg), *sinfo = (int *)(smem + L::sinfo), *s_ctl = (int *)(smem + L::ctl);

    const unsigned tid = threadIdx.x, lane = tid & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));

    // ---- placement: which XCD am I on, which of its 32 workers am I?
    if (tid == 0) {
        unsigned xid, r;
        const int ok = xd_place(p, NW, xid, r);
        s_ctl[0] = (int)xid; s_ctl[1] = (int)r; s_ctl[2] = ok; s_ctl[3] = 0; s_ctl[4] = (int)p.status_tag; s_ctl[5] = 0;
    }
    __syncthreads();
    const int xcc = __builtin_amdgcn_readfirstlane(s_ctl[0]), rank = __builtin_amdgcn_readfirstlane(s_ctl[1]);
    if (__builtin_amdgcn_readfirstlane(s_ctl[2]) == 0) return;
    int bx = (p.n_slots - xcc + 7) / 8;                // slots of this XCD: xcc, xcc + 8, ...
    bx = bx < 0 ? 0 : (bx > BXT ? BXT : bx);
    const int n_steps = p.n_steps[xcc];
    if (bx == 0 || n_steps <= 0) return;
    const int agent = p.agent_stores;

    u64 *gh = p.xg + CTL_WORDS / 2 + (size_t)xcc * xg_region(BXT);
    u64 *ga = gh + xg_h(BXT), *gc = ga + xg_a(BXT);

    // ---- lane geometry of the chain waves
    const unsigned R = lane >> 4, kw = (lane >> 2) & 3u, j = lane & 3u, rq = R >> 1, c0 = R & 1u, cid = 2u * kw + c0;
    const unsigned r8 = 4u * rq + j;                                   // row of the wave's 8
    const bool sum_lane = (lane & 0x1Cu) == 0;                         // kw == 0, c0 == 0: holds the row sum after chain_combine

    // ---- resident LDS state
    for (unsigned e = tid; e < NC * ROWS; e += THREADS) {
        const unsigned cls = e / ROWS, rem = e - cls * ROWS, g = rem / UPB, ul = rem - g * UPB;
        gemb[e] = p.Gemb[(size_t)cls * 3 * HR + g * HR + UPB * rank + ul];
    }
    for (unsigned e = tid; e < FPB * HR; e += THREADS) {
        const unsigned rr = e / HR, rem = e - rr * HR, cc = rem / NT_H, n = rem - cc * NT_H;
        fc1w[((n >> 2) * 64 + xd_lane_of(rr, cc)) * 4 + (n & 3)] = p.w_fc1[(size_t)(FPB * rank + rr) * HR + chain_col(HR / 64, cc >> 1, cc & 1, n)];
    }
    for (unsigned e = tid; e < FPB * HF; e += THREADS) {
        const unsigned rr = e / HF, rem = e - rr * HF, cc = rem / NT_A, n = rem - cc * NT_A;
        fc2w[((n >> 2) * 64 + xd_lane_of(rr, cc)) * 4 + (n & 3)] = p.w_fc2[(size_t)(FPB * rank + rr) * HF + chain_col(HF / 64, cc >> 1, cc & 1, n)];
    }
    for (unsigned e = tid; e < 4 * HR; e += THREADS) {                 // W_hh rows 80..83 = gate 2 (n), units 24..27
        const unsigned rr = e / HR, rem = e - rr * HR, cc = rem / NT_H, n = rem - cc * NT_H;
        whx[((n >> 2) * 32 + (xd_lane_of(rr, cc) & 31u)) * 4 + (n & 3)] = p.w_hh[(size_t)(2 * HR + UPB * rank + 24 + rr) * HR + chain_col(HR / 64, cc >> 1, cc & 1, n)];
    }
    for (unsigned e = tid; e < NC; e += THREADS) mtab[e] = p.mulaw_tab[e];
    for (unsigned e = tid; e < 96; e += THREADS) { const unsigned g = e >> 5, u = e & 31; c_bq[e] = u < UPB ? p.b_hh[g * HR + UPB * rank + u] : 0.f; }
    for (unsigned e = tid; e < BXT * 96; e += THREADS) gsum[e] = 0.f;
    for (unsigned e = tid; e < BXT * L::HS; e += THREADS) hc[e] = 0.f;     // four slots: the matrix instruction multiplies all four columns, also those of slots this XCD does not run
    for (unsigned e = tid; e < BXT; e += THREADS) {
        const XdSeg sg = (int)e < bx ? p.segs[(size_t)(xcc + 8 * e) * p.max_seg] : XdSeg{-1, 0, 0, 0u};
        seg_st[e * 8 + 0] = 0; seg_st[e * 8 + 1] = sg.len > 0 ? sg.row : -1; seg_st[e * 8 + 2] = sg.t0; seg_st[e * 8 + 3] = sg.len;
        seg_st[e * 8 + 4] = (int)sg.utt; seg_st[e * 8 + 5] = 0; seg_st[e * 8 + 6] = RESUME ? rp.s0 / p.upsample : 0;      // samples into / index of the conditioning frame
        seg_st[e * 8 + 7] = sg.len > 0 ? ((const int *)(p.segs + (size_t)8 * BXT * p.max_seg))[sg.row] : 0;      // the utterance's first Gcond row
    }
    __syncthreads();

    Waiter wt{p.status, p.timeout_ticks, 0};
#ifdef VQCPC_XD_BARS
    unsigned long long xd_arrived = 0;
#endif
    int *s_abort = s_ctl + 3;

    // h_t gather: every thread takes column tid of every slot, the first 128 threads also column 768 + tid
    const unsigned hk1 = tid, hk2 = THREADS + (tid & 127u);
    const unsigned hoff1 = ((((hk1 / UPB) * BXT) << 5) + hk1 % UPB) * 8u, hoff2 = ((((hk2 / UPB) * BXT) << 5) + hk2 % UPB) * 8u;
    const unsigned hdst1 = BXT == 4 ? chain_pos_plain<HR / 64>(hk1, NT_H) : chain_pos<HR / 64>(hk1, NT_H),
                   hdst2 = BXT == 4 ? chain_pos_plain<HR / 64>(hk2, NT_H) : chain_pos<HR / 64>(hk2, NT_H);
    const bool two = tid < HR - THREADS;
    // words: the sweep deals 16-byte chunks, each four consecutive units of one (rank, slot): chunk c = (rank * BXT + slot) * 7 + q holds
    // units 4 q .. 4 q + 3, so a wave's 64 chunks are consecutive in memory (but for the unused eighth chunk of a line).  Thread tid takes
    // chunk tid, threads 0..127 of four slots also chunk 768 + tid: the shape above, with chunks in place of columns.  A chunk of a slot
    // this XCD does not run is not loaded.  In hc a chunk's units 1 and 3 are the next chain's (NT_H further), unit 2 sits at wd*b.
    constexpr unsigned NCH = NW * BXT * 7;
    unsigned woff1 = XD_NO_CHUNK, woff2 = XD_NO_CHUNK, wd1 = 0, wd1b = 0, wd2 = 0, wd2b = 0;
    constexpr bool SVC = !(W && BXT == 4 && XD_SVC_SWEEP == 0);      // the service waves take part in the sweep
    constexpr unsigned NT1 = SVC ? THREADS : THREADS - 128u;        // threads with a first chunk; the next NCH - NT1 chunks are second chunks
    const unsigned ct = SVC ? tid : tid - 128u;
    const bool hx2 = NCH > NT1 && wave >= XD_HX && wave < XD_HX + (int)((NCH - NT1) / 64u);      // this wave's threads take a second chunk
    if constexpr (W) {
        auto chunk = [&](unsigned c, unsigned &off, unsigned &d0, unsigned &d2) {
            const unsigned rs = c / 7u, q = c - 7u * rs, r = rs / BXT, b = rs - r * BXT, k0 = UPB * r + 4u * q;
            if (c < NCH && (int)b < bx) off = xg_h_off_w(r, b, BXT, 4u * q);
            d0 = b * L::HS + (BXT == 4 ? chain_pos_plain<HR / 64>(k0, NT_H) : chain_pos<HR / 64>(k0, NT_H));
            d2 = BXT == 4 ? d0 + 4u : b * L::HS + chain_pos<HR / 64>(k0 + 2, NT_H);
        };
        if (SVC || wave >= 2) chunk(ct, woff1, wd1, wd1b);
        if (hx2) chunk(NT1 + tid - 64u * XD_HX, woff2, wd2, wd2b);
    }
    static_assert(!(W && (XD_ABLATE & 8)), "XD_ABLATE bit 3 is a proxy on the granule format");
    // XD_ABLATE bit 3 (granules, four slots; timing only): the sweep loads and checks slots 0 and 1, the other two columns of hc keep
    // what they held -- half the sweep's bytes and instructions, an upper bound on what the words can return (profiles/r15_ab_exchange_words.txt)
    constexpr int NL = (BXT == 4 && (XD_ABLATE & 8)) ? 2 : BXT;
#define XD_SWEEP_H()                                                                                              \
    do {                                                                                                          \
        if (BXT == 4 && XD_HNAP > 0 && wave >= 2) __builtin_amdgcn_s_sleep(XD_HNAP);                              \
        wt.start();                                                                                               \
        if constexpr (W) {                                                                                        \
            const unsigned par = tag & 1u;                                                                        \
            u32x4 c1 = {0u, 0u, 0u, 0u}, c2 = {0u, 0u, 0u, 0u};                                                   \
            for (unsigned spins = 0;; ++spins) {                                                                  \
                bool ok = true;                                                                                   \
                if (hx2) {                                                                                        \
                    gran_load_pair(c1, c2, gh, woff1, woff2);                                                     \
                    c2 = xd_chunk_h_open(c2, par);                                                                \
                    ok = (woff2 == XD_NO_CHUNK) | xd_chunk_h_ok(c2);                                              \
                } else gran_load(c1, gh, woff1);                                                                  \
                c1 = xd_chunk_h_open(c1, par);                                                                    \
                ok &= (woff1 == XD_NO_CHUNK) | xd_chunk_h_ok(c1);                                                 \
                if ((XD_ABLATE & 4) || __all(ok)) { XD_POLLS(0, spins); break; }                                  \
                if (wt.expired(spins, lane, s_abort + 1)) { *s_abort = 1; break; }                                \
                __builtin_amdgcn_s_sleep(1);                                                                      \
            }                                                                                                     \
            if (woff1 != XD_NO_CHUNK) {                                                                           \
                hc[wd1] = __uint_as_float(c1[0]); hc[wd1 + NT_H] = __uint_as_float(c1[1]);                        \
                hc[wd1b] = __uint_as_float(c1[2]); hc[wd1b + NT_H] = __uint_as_float(c1[3]);                      \
            }                                                                                                     \
            if (hx2 && woff2 != XD_NO_CHUNK) {                                                                    \
                hc[wd2] = __uint_as_float(c2[0]); hc[wd2 + NT_H] = __uint_as_float(c2[1]);                        \
                hc[wd2b] = __uint_as_float(c2[2]); hc[wd2b + NT_H] = __uint_as_float(c2[3]);                      \
            }                                                                                                     \
        } else {                                                                                                  \
            u64 v1[NL], v2[NL];                                                                                   \
            for (unsigned spins = 0;; ++spins) {                                                                  \
                bool ok = true;                                                                                   \
                if (wave < 2) {                                                                                   \
                    gran_load_pair<NL, 256>(v1, v2, gh, hoff1, hoff2);                                            \
                    _Pragma("unroll") for (int b = 0; b < NL; ++b) ok &= b >= bx || (unsigned)(v2[b] >> 32) == tag; \
                } else gran_load<NL, 256>(v1, gh, hoff1);                                                         \
                _Pragma("unroll") for (int b = 0; b < NL; ++b) ok &= b >= bx || (unsigned)(v1[b] >> 32) == tag;   \
                if ((XD_ABLATE & 4) || __all(ok)) { XD_POLLS(0, spins); break; }                                  \
                if (wt.expired(spins, lane, s_abort + 1)) { *s_abort = 1; break; }                                \
                __builtin_amdgcn_s_sleep(1);                                                                      \
            }                                                                                                     \
            _Pragma("unroll") for (int b = 0; b < NL; ++b) {                                                      \
                if (b < bx) { hc[b * L::HS + hdst1] = __uint_as_float((unsigned)v1[b]); if (two) hc[b * L::HS + hdst2] = __uint_as_float((unsigned)v2[b]); } \
            }                                                                                                     \
        }                                                                                                         \
    } while (0)

    const float *opnd = hc + cid * NT_H + 4 * j;                       // dpp chains: the quad's lane j reads word j of a phase
    // matrix-pipe chains (four slots): lane j reads slot j's chain, the upper half wave the second word of a group
    const float *opm = hc + j * L::HS + cid * NT_H + 4 * rq;
    bool fc1_role = false;
    if constexpr (BXT == 1) fc1_role = wave == 1;
    if (fc1_role) {
        // =====================================================================================  one slot per XCD: wave 1 is fc1
        // With one slot the second service wave has no slot of its own; it holds the 8 fc1 rows like a chain wave holds W_hh rows
        // (112 weights per lane, pinned) and runs fc1 -- the first thing on the step's critical path -- in one chain pass of
        // 0.4 us instead of the 0.75 us of the LDS-streamed pass on wave 0, which takes W_hh rows 80..83 in exchange.
        if constexpr (BXT == 1) {
            float w1[NT_H];
            ps_load_weights<HR / 64>(p.w_fc1 + (size_t)(FPB * rank + r8) * HR, kw, c0, w1);
            const float b1 = p.b_fc1[FPB * rank + r8];
            ps_barrier();                                                  // state and noise of step 0 posted
            for (int t = 0; t < n_steps; ++t) {
                const unsigned tag = (unsigned)t + 1u;
                XD_SWEEP_H();
                XD_BARRIVE();
                ps_barrier();                                            // A: h_t in LDS
                XD_BLEAVE(0);
                if (*s_abort) break;
                float v = chain_combine(chain_regs<NT_H>(w1, opnd));
                v += b1;
                v = v > 0.f ? v : 0.f;
                if (sum_lane) xd_put_a<WA>(ga, (unsigned)rank, r8, 0u, v, tag, agent);
                XD_STAMP(1, 10);
                XD_BARRIVE();
                ps_barrier();                                            // B
                XD_BLEAVE(2);
                if (*s_abort) break;
            }
        }
    } else if (wave >= 2) {
        const int cw = wave - 2;                                           // chain wave 0..9
        // =====================================================================================  chain waves: W_hh rows 0..79
        const unsigned row_local = 8 * cw + r8;                          // gate * UPB + unit
        float w[NT_H];
        {
            const unsigned gate = row_local / UPB, ul = row_local - gate * UPB;
            ps_load_weights<HR / 64>(p.w_hh + (size_t)(gate * HR + UPB * rank + ul) * HR, kw, c0, w);
        }
        // wave b < bx also runs fc2 + the draw of slot b (one slot per wave, in parallel), between its W_hh chains: a_t of the
        // slot arrives while the first chains run
        // which slot's fc2 + draw this wave runs.  Four slots: waves 2, 3, 6, 7 (SIMDs 2 and 3) take slots 0..3 -- the chain waves that share
        // a SIMD with a service wave stay pure chains (their matrix instructions starve the vector instructions of whoever shares the SIMD:
        // profiles/r04_mfma_chains.txt), and wave 11 draws the next step's noise once its chain is through
        const int fs = BXT == 4 ? ((cw & 2) == 0 && cw < 6 ? 2 * (cw >> 2) + (cw & 1) : BXT) : cw;
        const bool fc2_wave = fs < bx;
        const int fc2_after = bx < 3 ? bx : 3;                             // chains done before it looks for a_t
        const float b2 = p.b_fc2[FPB * rank + r8];
        const float4 *wp2 = (const float4 *)fc2w + lane;                   // word i of this lane's chain at wp2[64 i]
        const float *opnd2 = ac + (fs < BXT ? fs : 0) * (8 * 48) + cid * 48 + 4 * j;
        ps_barrier();                                                      // state and noise of step 0 posted
        for (int t = 0; t < n_steps; ++t) {
            const unsigned tag = (unsigned)t + 1u;
            XD_SWEEP_H();
            XD_BARRIVE();
            ps_barrier();                                                // A: h_t in LDS
            XD_BLEAVE(0);
            if (*s_abort) break;
            auto fc2_and_draw = [&]() {
                // ---- a_t of slot fs (256 granules in one run, 4 per lane) -> fc2 -> Gumbel-max candidate of the 8 owned classes
                // the lane's granules are the 16-byte chunks lane and lane + 64 of the run: a_t[2 lane], a_t[2 lane + 1] and the same 128 further
                const unsigned aoff = xg_a_off(0u, 0u, (unsigned)fs) + lane * 16u;
                const unsigned adst = (unsigned)chain_pos<HF / 64>(2 * (int)lane, 48);   // a_t[k + 1]: the chain next door (48 further), a_t[k + 128]: 192 further
                float4 wa = wp2[0], wb = wp2[64];                    // first weights and the noise: on their way during the sweep
                unsigned lno = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));      // the lane id, from the hardware
                asm volatile("" : "+v"(lno));      // opaque, and rebuilt: the hoisted address of this read -- then r8, then the lane id
                const unsigned r8o = ((lno >> 5) << 2) | (lno & 3u);      // itself -- was spilled to scratch and reloaded at every step
                const float nz = noise[(t & 1) * (BXT * 8) + fs * 8 + r8o];
                wt.start();
                if constexpr (WA) {
                    // words: the slot's run is 1 KB, the lane's chunk a_t[4 lane .. 4 lane + 3] -- one load; a_t[k + 1] is the chain next
                    // door (48 further), a_t[k + 2] the second operand word of the same phase (16 further).  The words go into LDS as they are: fc2 takes |word|
                    const unsigned aoffw = xg_a_off_w(0u, 0u, (unsigned)fs) + lane * 16u;
                    const unsigned adw = (unsigned)chain_pos<HF / 64>(4 * (int)lane, 48);
                    u32x4 vw = {0u, 0u, 0u, 0u};
                    for (unsigned spins = 0;; ++spins) {
                        gran_load(vw, ga, aoffw);
                        if ((XD_ABLATE & 2) || __all(xd_chunk_a_ok(vw, tag & 1u))) { XD_POLLS(1, spins); break; }
                        if (wt.expired(spins, lane, s_abort + 1)) { *s_abort = 1; break; }
                    }
                    ac[fs * (8 * 48) + adw] = __uint_as_float(vw[0]);
                    ac[fs * (8 * 48) + 48 + adw] = __uint_as_float(vw[1]);
                    ac[fs * (8 * 48) + 16 + adw] = __uint_as_float(vw[2]);
                    ac[fs * (8 * 48) + 64 + adw] = __uint_as_float(vw[3]);
                } else {
                u32x4 va[2];
                for (unsigned spins = 0;; ++spins) {
                    gran_chunks2(va, ga, aoff);
                    const bool ok = va[0][1] == tag && va[0][3] == tag && va[1][1] == tag && va[1][3] == tag;
                    if ((XD_ABLATE & 2) || __all(ok)) { XD_POLLS(1, spins); break; }
                    if (wt.expired(spins, lane, s_abort + 1)) { *s_abort = 1; break; }
                }
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    ac[fs * (8 * 48) + 192 * i + adst] = __uint_as_float(va[i][0]);
                    ac[fs * (8 * 48) + 192 * i + 48 + adst] = __uint_as_float(va[i][2]);
                }
                }
                XD_STAMP(2, 8);
                const float4 a0 = *(const float4 *)opnd2, a1 = *(const float4 *)(opnd2 + 16);
                const float hv[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                float acc2 = 0.f;
#pragma unroll
                for (int J = 0; J < 4; ++J) {                            // 32 terms: 8 per quad lane, weights two 16-byte words at a time
                    float4 na = wa, nb2 = wb;
                    if (J < 3) { na = wp2[64 * (2 * J + 2)]; nb2 = wp2[64 * (2 * J + 3)]; }
                    const float w8[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
                    if (J == 0) fmac8<0, WA>(acc2, hv, w8);                // words: |a_t| -- the sign bit is the parity
                    if (J == 1) fmac8<1, WA>(acc2, hv, w8);
                    if (J == 2) fmac8<2, WA>(acc2, hv, w8);
                    if (J == 3) fmac8<3, WA>(acc2, hv, w8);
                    wa = na; wb = nb2;
                }
                float v2 = chain_combine(acc2);
                v2 += b2;
                const float sc = v2 + nz;                                // classes 0..3 of the 8 in lanes 0..3, 4..7 in lanes 32..35
                float best;
                int kb;
                first_max_8lanes(sc, best, kb);                          // first argmax in lanes, not 8 v_readlane and a scalar compare / select chain (profiles/r13_ab_at_handoff.txt)
                const bool drop = p.dbg_drop_step >= 0 && t == p.dbg_drop_step && rank == 3 && xcc == 0;
                if (lane == 0 && !drop)
                    xd_put(gc, ((unsigned)fs * NW + (unsigned)rank) * 8u, ((u64)((tag << 8) | (unsigned)(FPB * rank + kb)) << 32) | __float_as_uint(best), agent);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the chain wave has slack here; draining its store now measured 0.035 us/step (profiles/r04_ab_*, section 5)
                XD_STAMP(2, 9); if (fs == 0) XD_WSTAMP(3);
            };
            if constexpr (BXT == 4) {
                // ---- the four slots at once on the matrix pipe (ar_chain.h); the wave of slot cw looks for a_t after XD_GSPLIT of the
                // chain's 14 groups: fc1 is out about then
                v4f a4 = {0.f, 0.f, 0.f, 0.f};
                float4 cur = *(const float4 *)opm;
                // waves 4 and 8 share fc1's SIMD (wave 0): they stand back until a_t is out.  Three dependent-chain waves keep a SIMD's issue port
                // busy; fc1 -- the head of the step's critical path -- ran at a third of the matrix pipe, and the 60 vector instructions between its
                // last term and the a_t stores took 0.4..0.7 us among the others' matrix instructions (profiles/r04_mfma_chains.txt)
#if XD_HOLD
                // Bounded: behind barrier A wave 0 either posts the flag, with no wait in between, or it leaves because it read *s_abort
                // set -- and *s_abort is never cleared within a call.  So the flag comes or *s_abort is seen; then the chain runs on
                // whatever it reads, and the wave leaves at barrier B.
                if ((wave & 3) == 0)
                    while (__hip_atomic_load(s_ctl + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != (int)tag &&
                           __hip_atomic_load(s_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
                        __builtin_amdgcn_s_sleep(2);
#endif
                chain_mfma_regs<0, XD_GSPLIT>(a4, w, opm, cur);
                if (fc2_wave) fc2_and_draw();
                chain_mfma_regs<XD_GSPLIT, NG_H>(a4, w, opm, cur);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = chain_combine(a4[i]);                // row 8 cw + 4 rq + i of slot j
                    if (sum_lane) gsum[j * 96 + 8 * cw + 4 * rq + i] = v;
                }
                if (wave == 11) {
                    // ---- the Gumbel noise of step t + 1's draw, all four slots (class lane & 7 of slot lane >> 3): it depends on nothing but the
                    // slots' clocks, which advance() posted in front of barrier A
                    unsigned ln = lane;
                    asm volatile("" : "+v"(ln));
                    const int b = (int)(ln >> 3);
                    if (ln < 32 && b < bx) {
                        const unsigned cls = FPB * rank + (ln & 7u);
                        noise[((t + 1) & 1) * (BXT * 8) + b * 8 + (ln & 7u)] = draw_noise((unsigned)sinfo[b * 2], (unsigned)sinfo[b * 2 + 1], cls, p.seed);
                    }
                }
            } else {
                for (int b = 0; b < bx; ++b) {
                    const float acc = chain_regs<NT_H>(w, opnd + b * HR);
                    const float v = chain_combine(acc);
                    if (sum_lane) gsum[b * 96 + row_local] = v;
                    if (fc2_wave && b + 1 == fc2_after) fc2_and_draw();
                }
            }
            XD_STAMP(2, 6);
            XD_BARRIVE();
            ps_barrier();                                                // B: gsum of step t complete; hc free for h_{t+1}
            XD_BLEAVE(2);
            if (*s_abort) break;
        }
    } else {
        // =====================================================================================  service waves
        // Wave 0 (sv 0) owns the even slots of the XCD, wave 1 (sv 1) the odd ones, for what is serial in a sample step
        // and not a chain wave's: x_{t-1} from the slot's 32 candidates, the cell update of the 28 owned units, h_t
        // published, fc1 -> a_t published; and, behind those, W_hh rows 80..83 for the OTHER wave's slots and the next
        // step's Gumbel noise.  Half wave hw of the cell update takes slot sv + 2 hw.
        const int sv = wave;
        const int hw = (int)(lane >> 5);
        const int cb = sv + 2 * hw;                                     // slot of this half wave in the cell update
        const unsigned cu = lane & 31u;                                 // unit
        const int n_own = bx > sv ? (bx - sv + 1) / 2 : 0;              // slots sv, sv + 2 < bx
        const bool cell_on = cb < bx;
        const float b1 = p.b_fc1[FPB * rank + r8];
        float b1q[4] = {0.f, 0.f, 0.f, 0.f};                              // four slots: the lane's accumulators are rows 4 rq + 0..3
        if constexpr (BXT == 4) { for (int i = 0; i < 4; ++i) b1q[i] = p.b_fc1[FPB * rank + 4 * rq + i]; }
        const float4 *wp1 = (const float4 *)fc1w + lane;                   // word i of this lane's chain at wp1[64 i]
        const float4 *wpx = (const float4 *)whx + (lane & 31u);            // rows 80..83: both half waves read the same 32 lane-chains, word i at wpx[32 i]
        const float bq0 = c_bq[cu], bq1 = c_bq[32 + cu], bq2 = c_bq[64 + cu];
        // the slot's 32 candidates are contiguous ([slot][worker]: a half wave's poll reads two lines, not one line per worker -- 1.6 % of a
        // single-utterance step, 0.7 % at 32 utterances: profiles/r04_ab_lds_layout_and_encoder_pingpong.txt)
        const u64 *csrc = gc + ((unsigned)(cb < BXT ? cb : 0) * NW + (lane & 31u));
        // W_hh rows 80..83 for the other wave's slots 1 - sv and 3 - sv: the lower half wave takes the first, the upper half the second
        const int xb0 = BXT == 1 ? 0 : 1 - sv;                            // one slot per XCD: wave 0 takes them itself (wave 1 is fc1)
        const bool x_two = xb0 + 2 < bx;
        const int xslot = xb0 + ((hw && x_two) ? 2 : 0);
        const float *opndx = opnd + xslot * HR;

        // ---- slot state, one step ahead: what the cell update of step `tn` will need that does not depend on the data
        bool st_active = false, st_first = false, st_emit = false;
        int st_erow = 0, st_eidx = 0, st_lt = 0;
        unsigned st_utt = 0u;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, hprev = 0.f;
        // RESUME: raw step 0 of a segment primes (publishes h_in), its samples are raw steps 1 .. len - 1
        bool st_prime = false, st_last = false;
        int st_row = 0, st_xin = NC / 2;
        float st_hin = 0.f;
        auto advance = [&](int tn) {
            st_active = false; st_first = false; st_emit = false;
            if constexpr (RESUME) { st_prime = false; st_last = false; }
            if (!cell_on) return;
            int si = seg_st[cb * 8 + 0], row = seg_st[cb * 8 + 1], t0 = seg_st[cb * 8 + 2], len = seg_st[cb * 8 + 3];
            int fpos = seg_st[cb * 8 + 5], fidx = seg_st[cb * 8 + 6], gb = seg_st[cb * 8 + 7];
            unsigned utt = (unsigned)seg_st[cb * 8 + 4];
            int lt = tn - t0;
            if (row >= 0 && lt >= 1 && lt <= len) { st_emit = true; st_erow = row; st_eidx = lt - 1; }    // x_{tn-1} is sample lt - 1 of `row`
            if (row >= 0 && lt >= len) {                             // next utterance of this slot (uniform per half wave)
                si += 1;
                XdSeg sg = XdSeg{-1, 0, 0, 0u};
                if (si < p.max_seg) sg = p.segs[(size_t)(xcc + 8 * cb) * p.max_seg + si];
                row = sg.len > 0 ? sg.row : -1; t0 = sg.t0; len = sg.len; utt = sg.utt;
                lt = tn - t0;
                fpos = 0; fidx = RESUME ? rp.s0 / p.upsample : 0;
                gb = row >= 0 ? ((const int *)(p.segs + (size_t)8 * BXT * p.max_seg))[row] : 0;
                if (cu == 0) { seg_st[cb * 8 + 0] = si; seg_st[cb * 8 + 1] = row; seg_st[cb * 8 + 2] = t0; seg_st[cb * 8 + 3] = len; seg_st[cb * 8 + 4] = (int)utt;
                               seg_st[cb * 8 + 5] = 0; seg_st[cb * 8 + 6] = fidx; seg_st[cb * 8 + 7] = gb; }
            }
            st_active = row >= 0 && lt >= 0 && lt < len;
            st_first = lt == 0;
            st_lt = lt; st_utt = utt;
            if constexpr (RESUME) {
                st_prime = st_active && lt == 0;
                st_last = st_active && lt == len - 1 && lt >= 1;
                st_active = st_active && lt >= 1;
                st_first = lt == 1;
                st_lt = rp.s0 + lt - 1;                               // the Philox counter: the sample's absolute index
                if (st_prime) {
                    st_row = row;
                    st_xin = rp.x_in ? rp.x_in[row] : NC / 2;
                    st_hin = rp.h_in && cu < UPB ? rp.h_in[(size_t)row * HR + UPB * rank + cu] : 0.f;
                }
            }
            if (BXT == 4 && cu == 0) { sinfo[cb * 2] = st_lt; sinfo[cb * 2 + 1] = (int)utt; }
            if (st_active) {
                if (fpos == p.upsample) { fpos = 0; fidx += 1; }
                if (fpos == 0 && cu < UPB) {                         // next conditioning frame (once per hop)
                    const int f = fidx < p.F ? fidx : p.F - 1;
                    const float *gcp = p.Gcond + ((size_t)gb + f) * 3 * HR + UPB * rank + cu;
                    g0 = gcp[0]; g1 = gcp[HR]; g2 = gcp[2 * HR];
                }
                fpos += 1;
                if (cu == 0) { seg_st[cb * 8 + 5] = fpos; seg_st[cb * 8 + 6] = fidx; }
            }
        };
        // the Gumbel noise of step `tn`'s draw (it does not depend on the data): class lane & 7 of slot sv + 2 ((lane >> 3) & 1)
        auto post_noise = [&](int tn) {
            const int lt_b = __builtin_amdgcn_readlane(st_lt, 0), lt_b2 = __builtin_amdgcn_readlane(st_lt, 32);
            const unsigned ut_b = __builtin_amdgcn_readlane(st_utt, 0), ut_b2 = __builtin_amdgcn_readlane(st_utt, 32);
            unsigned ln = lane;
            asm volatile("" : "+v"(ln));           // an opaque copy: hipcc hoisted the store address out of the sample loop and spilled it
            if (ln < 16) {
                const int which = (int)(ln >> 3), b = sv + 2 * which;
                if (b < bx) {
                    const unsigned cls = FPB * rank + (ln & 7u);
                    noise[(tn & 1) * (BXT * 8) + b * 8 + (ln & 7u)] = draw_noise((unsigned)(which ? lt_b2 : lt_b), which ? ut_b2 : ut_b, cls, p.seed);
                }
            }
        };
        advance(0);
        post_noise(0);
        ps_barrier();                                                    // state and noise of step 0 posted

        int x = NC / 2;
        float hsent = 0.f;                                               // words: the h_t this lane published at step t
        for (int t = 0; t < n_steps; ++t) {
            const unsigned tag = (unsigned)t + 1u;
            __builtin_amdgcn_s_setprio(3);
            XD_STAMP(0, 0);
            // ---- cell update: gsum of step t-1 is complete (barrier B), x_{t-1} was picked up before it
            float s0 = 0.f, s1 = 0.f, sn = 0.f, hold = 0.f;
            if (st_active && (RESUME || !st_first)) {                  // resumed: the priming step's chains made W_hh h_in
                s0 = gsum[cb * 96 + cu]; s1 = gsum[cb * 96 + UPB + cu]; sn = gsum[cb * 96 + 2 * UPB + cu];
                hold = hprev;
            }
            s0 += bq0; s1 += bq1; sn += bq2;
            if (cell_on) {
                float hn = 0.f;
                if (st_active && cu < UPB) {
                    const int xe = st_first ? (RESUME ? st_xin : NC / 2) : x;
                    const float e0 = gemb[(xe * 3 + 0) * UPB + cu], e1 = gemb[(xe * 3 + 1) * UPB + cu], e2 = gemb[(xe * 3 + 2) * UPB + cu];
                    const float r = gate_sigmoid((e0 + g0) + s0);            // gru_cell, written out (s = W_hh h + b_hh)
                    const float z = gate_sigmoid((e1 + g1) + s1);
                    const float nn = gate_tanh((e2 + g2) + r * sn);
                    hn = (1.0f - z) * nn + z * hold;
                    hprev = hn;
                }
                if constexpr (RESUME) {
                    if (st_prime && cu < UPB) { hn = st_hin; hprev = hn; }
                    if (st_last && rp.h_out && cu < UPB) rp.h_out[(size_t)st_row * HR + UPB * rank + cu] = hn;
                }
                if constexpr (W) {
                    if (cu < UPB) xd_put_word(gh, xg_h_off_w((unsigned)rank, (unsigned)cb, BXT, cu), xd_word_h(hn, tag & 1u), agent);
                    hsent = hn;                                          // tested for its range where this wave has slack (below)
                } else if (cu < UPB) xd_put(gh, (((unsigned)(rank * BXT + cb) << 5) + cu) * 8u, ((u64)tag << 32) | __float_as_uint(hn), agent);
            }
            XD_STAMP(0, 2); if (wave == 0) XD_WSTAMP(0);
            // ---- in the shadow of the h_t exchange: the sample x_{t-1} goes out (network_vocoder.py:78 output), the slot's state
            // and the noise for step t + 1, the first phase of the fc1 weights
            if (st_emit && cu == 0 && rank == (cb & 31)) {
                if (p.wav) p.wav[(size_t)st_erow * p.Lout + st_eidx] = mtab[x];      // emit_sample, written out
                if (p.mulaw) p.mulaw[(size_t)st_erow * p.Lout + st_eidx] = x;
            }
            advance(t + 1);
            float4 w1p[BXT == 4 ? 2 * XD_DEPTH : 8];                      // the first weights of what follows barrier A, requested in front of it
#pragma unroll
            for (int i = 0; i < (BXT == 4 ? 2 * XD_DEPTH : 8); ++i) w1p[i] = (BXT == 4 && sv == 1) ? wpx[32 * i] : wp1[64 * i];      // four slots: wave 1 runs W_hh rows 80..83
            if constexpr (SVC) XD_SWEEP_H();
            XD_STAMP(0, 3);
            XD_BARRIVE();
            ps_barrier();                                                // A: h_t in LDS
            XD_BLEAVE(0);
            if (*s_abort) break;
            XD_STAMP(0, 4); if (wave == 0) XD_WSTAMP(1);
            // ---- fc1 of the own slots (both together: every weight is used for both and then dropped); one slot per XCD: wave 1
            if constexpr (BXT == 4) {
                // ---- four slots: the matrix pipe takes them together (ar_chain.h), so the two waves split the ROWS instead of the slots:
                // wave 0 fc1 (the step's critical path: a_t goes out first), wave 1 W_hh rows 80..83
                if (sv == 0) {
                    const v4f a4 = chain_mfma_lds<64, XD_DEPTH>(wp1, w1p, opm);
                    XD_STAMP(0, 14);
#ifdef VQCPC_XD_STAMPS
                    { const int done = __builtin_amdgcn_readfirstlane(__float_as_int(a4[0])); asm volatile("" :: "s"(done)); }      // the last term's RESULT is there
                    XD_STAMP(0, 15);
#endif
                    // fc1 rows 4 rq + 0..3 of slot j together: one statement for the combines, bias and ReLU, one exec region, one
                    // statement of four stores 8 bytes apart (profiles/r13_ab_at_handoff.txt)
                    float v[4];
                    fc1_finish4(a4, b1q, v);
                    if constexpr (WA) {              // the four rows are one 16-byte chunk of the slot's run: one store
                        const unsigned par = tag & 1u;
                        if (sum_lane && (int)j < bx)
                            xd_put_chunk(ga, xg_a_off_w((unsigned)rank, 4u * rq, j), u32x4{xd_word_a(v[0], par), xd_word_a(v[1], par), xd_word_a(v[2], par), xd_word_a(v[3], par)}, agent);
                    } else if (sum_lane && (int)j < bx)
                        xd_put4<8>(ga, xg_a_off((unsigned)rank, 4u * rq, j), ((u64)tag << 32) | __float_as_uint(v[0]), ((u64)tag << 32) | __float_as_uint(v[1]),
                                   ((u64)tag << 32) | __float_as_uint(v[2]), ((u64)tag << 32) | __float_as_uint(v[3]), agent);
#if XD_HOLD
                    if (lane == 0) __hip_atomic_store(s_ctl + 5, (int)tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);      // a_t is out: waves 4 and 8 may start
#endif
                } else {
                    const v4f a4 = chain_mfma_lds<32, XD_DEPTH>(wpx, w1p, opm);     // both half waves run the same 32 lane-chains; the lower half's results count
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = chain_combine(a4[i]);
                        if (sum_lane && lane < 32) gsum[j * 96 + 80 + i] = v;
                    }
                }
            } else if (BXT > 1 && n_own > 0) {
                float accA, accB;
                chain_lds2<NT_H, 64>(wp1, w1p, opnd + sv * HR, opnd + (sv + 2 < BXT ? sv + 2 : sv) * HR, n_own > 1, accA, accB);
                float v = chain_combine(accA);
                v += b1;
                v = v > 0.f ? v : 0.f;
                if (sum_lane) xd_put_a<WA>(ga, (unsigned)rank, r8, (unsigned)sv, v, tag, agent);
                if (n_own > 1) {
                    float v2 = chain_combine(accB);
                    v2 += b1;
                    v2 = v2 > 0.f ? v2 : 0.f;
                    if (sum_lane) xd_put_a<WA>(ga, (unsigned)rank, r8, (unsigned)sv + 2u, v2, tag, agent);
                }
            }
            XD_STAMP(0, 5); if (wave == 0) XD_WSTAMP(2);
            XD_STAMP(1, 10);
            __builtin_amdgcn_s_setprio(1);
            // ---- words: was the h_t published above one the word can carry?  Tested HERE, where both service waves wait for the candidates --
            // between the store and barrier A every vector instruction is on the step's critical path (0.03 us there).  If not, the call ends
            // as on a timeout: this workgroup leaves at barrier B, the others when their next wait looks at the status word.
            if constexpr (W) {
                if (__any(cell_on && cu < UPB && !xd_word_h_fits(hsent))) {
                    if (lane == 0) __hip_atomic_store(p.status, (unsigned)s_abort[1] | STATUS_RANGE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    *s_abort = 1;
                }
            }
            // ---- W_hh rows 80..83 of the OTHER wave's slots, behind the a_t exchange and the chain waves' fc2: one chain pass,
            // the lower half wave on slot 1 - sv, the upper half on slot 3 - sv
            if (BXT != 4 && xb0 < bx) {
                float4 wx0[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) wx0[i] = wpx[32 * i];
                float acc, unused;
                chain_lds2<NT_H, 32>(wpx, wx0, opndx, opndx, false, acc, unused);
                const float v = chain_combine(acc);
                if (sum_lane && (lane < 32 || x_two)) gsum[xslot * 96 + 80 + (r8 & 3u)] = v;
            }
            XD_STAMP(0, 7);
            XD_STAMP(1, 11);
            if (BXT != 4) post_noise(t + 1);                             // idle time: the candidates are still on their way (four slots: wave 11 draws)
            XD_STAMP(0, 13);
            // ---- x_t: the slot's 32 candidates (tag t + 1, from the chain waves' fc2), picked up BEFORE barrier B
            __builtin_amdgcn_s_setprio(3);
            if (n_own > 0) {
                u64 g = 0;
                wt.start();
                for (unsigned spins = 0;; ++spins) {
                    g = ps_load(csrc);
                    if ((XD_ABLATE & 1) || __all(!cell_on || (unsigned)(g >> 40) == tag)) { XD_POLLS(2, spins); break; }
                    if (wt.expired(spins, lane, s_abort + 1)) { *s_abort = 1; break; }
                }
                // first argmax per half of 32 lanes (classes ascend with the rank): order-preserving integer image of the score
                const unsigned u = ordered((unsigned)g), m = row_max(u);
                const unsigned m0 = __builtin_amdgcn_readlane(m, 0), m1 = __builtin_amdgcn_readlane(m, 16),
                               m2 = __builtin_amdgcn_readlane(m, 32), m3 = __builtin_amdgcn_readlane(m, 48);
                const unsigned b01 = max(m0, m1), b23 = max(m2, m3);
                const unsigned long long hit = __ballot(u == (lane < 32 ? b01 : b23));
                const int f0 = __ffs((int)(unsigned)hit) - 1, f1 = __ffs((int)(unsigned)(hit >> 32)) - 1;
                const int cls = (int)((g >> 32) & 255u);
                const int x0 = __builtin_amdgcn_readlane(cls, f0 < 0 ? 0 : f0), x1 = __builtin_amdgcn_readlane(cls, 32 + (f1 < 0 ? 0 : f1));
                x = lane < 32 ? x0 : x1;
            }
            XD_STAMP(0, 1); if (wave == 0) XD_WSTAMP(4);
            __builtin_amdgcn_s_setprio(0);
            XD_BARRIVE();
            ps_barrier();                                                // B: gsum of step t complete; hc free for h_{t+1}
            XD_BLEAVE(2);
            if (*s_abort) break;
            XD_STAMP(0, 12); if (wave == 0) XD_WSTAMP(5);
        }
        // ---- the last step's x has nowhere to go: every utterance ended at least one step before n_steps
    }
#undef XD_SWEEP_H
}

template <int BXT>
__global__ __launch_bounds__(THREADS) void ar_xcd_kernel(XdParams p) { xcd_decoder<BXT, false>(p, XdResume{}); }
template <int BXT>
__global__ __launch_bounds__(THREADS) void ar_xcd_resume_kernel(XdParams p, XdResume r) { xcd_decoder<BXT, true>(p, r); }

template <int BXT>
constexpr size_t lds_bytes() { return sizeof(float) * (size_t)Lds<BXT>::total; }

template <int BXT>
int launch_t(const XdParams &p, hipStream_t s, const XdResume *rs) {
    constexpr size_t lds = lds_bytes<BXT>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    // per launch, not once per process: the attribute belongs to the current device, and a process may hold handles on several
    if (rs) {
        HIP_TRY(hipFuncSetAttribute((const void *)ar_xcd_resume_kernel<BXT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((ar_xcd_resume_kernel<BXT>), dim3(8 * NW), dim3(THREADS), lds, s, p, *rs);
        HIP_TRY(hipGetLastError());
        return VQCPC_OK;
    }
    HIP_TRY(hipFuncSetAttribute((const void *)ar_xcd_kernel<BXT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((ar_xcd_kernel<BXT>), dim3(8 * NW), dim3(THREADS), lds, s, p);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

}  // namespace

size_t xd_exchange_bytes(int bxt) { return (size_t)CTL_WORDS * 4 + (size_t)8 * xg_region(bxt) * sizeof(u64); }
bool xd_supported(int Hr, int Hf, int n_cls) { return Hr == HR && Hf == HF && n_cls == NC; }
int xd_pick_bxt(int n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= XD_MAX_BX ? 4 : 0; }

int xd_launch(const XdParams &p, hipStream_t s, const XdResume *rs) {
    VQ_REQUIRE(p.bxt == 1 || p.bxt == 2 || p.bxt == 4, "xd_launch: bxt %d", p.bxt);
    VQ_REQUIRE(p.n_slots >= 1 && p.n_slots <= 8 * p.bxt, "xd_launch: %d slots do not fit 8 x %d", p.n_slots, p.bxt);
    VQ_REQUIRE(!rs || (rs->s0 >= 0 && rs->s0 % p.upsample == 0), "xd_launch: resume at sample %d, not a multiple of %d", rs ? rs->s0 : 0, p.upsample);
    HIP_TRY(hipMemsetAsync(p.xg, 0, xd_exchange_bytes(p.bxt), s));
    switch (p.bxt) {
        case 1: return launch_t<1>(p, s, rs);
        case 2: return launch_t<2>(p, s, rs);
        case 4: return launch_t<4>(p, s, rs);
        default: return launch_t<4>(p, s, rs);
    }
}
