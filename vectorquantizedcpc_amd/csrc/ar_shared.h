// Device helpers shared by the decode kernels of vocoder.hip (launch per step), ar_xcd.hip / ar_xcm.hip (one resident
// decoder per XCD) and the scans of scan.hip.  Everything that decides a BIT of the result lives here once, so that
// an utterance decoded on any of the paths gives the same samples: the Philox stream of the sampling protocol and the noise of
// a draw (draw_noise), the gate non-linearities and the cell update (gru_cell), the four-MFMA step of a row's fp32 fma chains
// (mfma_k4) and the order in which the chains are loaded and combined (sum4), the first argmax over candidates (first_max and its
// 16-lane DPP form ordered / row_max / row_min), the launch path's candidate granules (cand_*) and a sample going out (emit_sample).
// NOT here: the prenet GRU and LSTM cells of scan.hip.  They are another specification -- libm gates, g + (W_hh h + b) in one
// bracket, pinned against the reference's own fixtures -- and stay written out where they are.
#pragma once
#include "common.h"
#include <math.h>

typedef unsigned long long u64;

// Bits of the decoder handle's host-mapped status word (its low byte; the reporting call's epoch sits above it, vqcpc_vocoder_check).
constexpr unsigned STATUS_TIMEOUT = 1u;      // an in-kernel exchange timed out
constexpr unsigned STATUS_MISPLACED = 2u;    // the resident decoders' workgroups were not dealt 32 per XCD (nothing written)
constexpr unsigned STATUS_BAD_INDEX = 4u;    // a code index or speaker id outside its embedding table
constexpr unsigned STATUS_RANGE = 8u;        // a hidden value that a 4-byte exchange word cannot carry (non-finite or |h| >= 2: xd_word_h)

// ---- launch-per-step recurrences (vocoder.hip's sample loop, scan.hip's sequence scans): weights in fragment order
// (scan.hip, build_wfrag_kernel), one 16-row x 16-utterance MFMA tile per workgroup, K split over 4 waves.
// state layout "hL": h[b][k] at ((b/16) * (K/4) + k/4) * 64 + (b%16) * 4 + k%4
__device__ __forceinline__ size_t hl_index(int K, int b, int k) {
    return ((size_t)(b >> 4) * (K >> 2) + (k >> 2)) * 64 + (b & 15) * 4 + (k & 3);
}

template <int SW>
__device__ __forceinline__ void load_wfrag(const float *Wf, int rg, int ksplit, int wave, int lane, float4 (&wf)[SW]) {
    const float4 *p = (const float4 *)Wf + ((size_t)(rg * ksplit + wave) * SW) * 64 + lane;
#pragma unroll
    for (int s = 0; s < SW; ++s) wf[s] = p[s * 64];
}

// ((q0 + q1) + q2) + q3: a row's sum over its four K quarters, on every path
__device__ __forceinline__ float sum4(float q0, float q1, float q2, float q3) { return ((q0 + q1) + q2) + q3; }
// One 16-column block of a K quarter on v_mfma_f32_16x16x4_f32: components x, z feed accumulator a0 and y, w feed a1 (two fma chains
// per row and quarter); the quarter's sum is a0 + a1.
__device__ __forceinline__ void mfma_k4(f32x4 &a0, f32x4 &a1, const float4 &w4, const float4 &h4) {
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.x, h4.x, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.y, h4.y, a1, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.z, h4.z, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w4.w, h4.w, a1, 0, 0, 0);
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
    for (int s = 0; s < SW; ++s) mfma_k4(a0, a1, wf[s], hv[s]);
    return a0 + a1;
}
// 16 rows x 16 utterances partial product over this wave's K quarter, every column live.
template <int SW>
__device__ __forceinline__ f32x4 mv16(const float4 (&wf)[SW], const float *hL, int K, int bt, int wave, int lane) {
    float4 hv[SW];
    load_hfrag<SW>(hL, K, bt, wave, lane, 16, hv);
    return mfma_frag<SW>(wf, hv);
}

// cross-wave reduction of the 4 K-quarters: red[wave][row][b] -> returns sum for (row=tid>>4, b=tid&15)
__device__ __forceinline__ float reduce4(float (*red)[16][17], const f32x4 &acc, int wave, int lane, int tid) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) * 4 + r][lane & 15] = acc[r];
    __syncthreads();
    const int row = tid >> 4, b = tid & 15;
    return sum4(red[0][row][b], red[1][row][b], red[2][row][b], red[3][row][b]);
}


__device__ __forceinline__ u64 ps_load(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ps_store(u64 *p, u64 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// workgroup barrier that also orders LDS traffic around it
__device__ __forceinline__ void ps_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// libm gates: the sequence scans of scan.hip, pinned against the reference's own fixtures
__device__ __forceinline__ float sigmoidf_(float v) { return 1.0f / (1.0f + expf(-v)); }

// Gates of the sample loop's GRU cell update (every decode form: vocoder.hip, ar_xcd.hip, ar_xcm.hip -- they must give the same
// bits) on the hardware transcendentals: v_exp_f32 (2^x) and v_rcp_f32, ~1 ulp each, without the range reduction of OCML's expf
// and the IEEE divide sequence and their branches -- the cell update runs on one wave on the step's critical path
// (profiles/r05_ab_gate_math.txt).  The ends saturate exactly: 2^x overflows to +inf and rcp(+inf) = 0, so sigmoid -> 0 / 1 and tanh -> -1 / +1.
// Every product and sum is written out (-ffp-contract=off).
constexpr float GATE_LOG2E = 1.44269504088896340736f;
__device__ __forceinline__ float gate_sigmoid(float v) {
    const float e = __builtin_amdgcn_exp2f(-v * GATE_LOG2E);
    return __builtin_amdgcn_rcpf(1.0f + e);
}
__device__ __forceinline__ float gate_tanh(float v) {            // 1 - 2 / (1 + e^{2v})
    const float e = __builtin_amdgcn_exp2f(v * (2.0f * GATE_LOG2E));
    const float q = __builtin_amdgcn_rcpf(1.0f + e);
    return 1.0f - 2.0f * q;
}
// The cell update (PyTorch GRUCell equations, gate order r, z, n): e = the embedding row of the sample fed in, g = the conditioning
// row, s = W_hh h of the unit's three gate rows (sum4 of their K quarters; 0 on an utterance's first step), b = b_hh, hold = h_{t-1}.
__device__ __forceinline__ float gru_cell(const float (&e)[3], const float (&g)[3], const float (&s)[3], const float (&b)[3], float hold) {
    const float r = gate_sigmoid((e[0] + g[0]) + (s[0] + b[0]));
    const float z = gate_sigmoid((e[1] + g[1]) + (s[1] + b[1]));
    const float n = gate_tanh((e[2] + g[2]) + r * (s[2] + b[2]));
    return (1.0f - z) * n + z * hold;
}

// Philox4x32-10, word `k & 3` of counter (t, utt, k >> 2, 0): the sampling protocol's stream.
__device__ __forceinline__ unsigned philox_word(unsigned c0, unsigned c1, unsigned c2, unsigned k0, unsigned k1, int w) {
    unsigned c[4] = {c0, c1, c2, 0u};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return w == 0 ? c[0] : w == 1 ? c[1] : w == 2 ? c[2] : c[3];
}
// Gumbel noise of (class, utterance, sample): 23 random bits + 0.5 -- every value is exact in fp32 and strictly inside
// (0, 1) (a 24-bit form rounds to 1.0f at the top word, i.e. +inf noise that wins whatever the logit is).
__device__ __forceinline__ float gumbel_from_word(unsigned w) {
    return -logf(-logf(((float)(w >> 9) + 0.5f) * (1.0f / 8388608.0f)));
}
// the noise of class `cls` in the draw of sample `lt` of utterance `utt`
__device__ __forceinline__ float draw_noise(unsigned lt, unsigned utt, unsigned cls, u64 seed) {
    return gumbel_from_word(philox_word(lt, utt, cls >> 2, (unsigned)seed, (unsigned)(seed >> 32), (int)(cls & 3u)));
}

// First argmax over candidates taken in class order: a later candidate wins only if it is strictly greater.
__device__ __forceinline__ void first_max(float &best, int &k, float score, int cls) {
    if (score > best) { best = score; k = cls; }
}
// The same over the 16 lanes of a DPP row, on the order-preserving integer image of the score: m = row_max(ordered(score)), then
// row_min over the classes of the lanes that hold m.
__device__ __forceinline__ unsigned ordered(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned row_max(unsigned m) {             // result in all 16 lanes
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, false));      // quad_perm [1,0,3,2]
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false));      // quad_perm [2,3,0,1]
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, false));     // row_half_mirror
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, false));     // row_mirror
    return m;
}
__device__ __forceinline__ unsigned row_min(unsigned m) {
    m = min(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xF, 0xF, false));
    m = min(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false));
    m = min(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xF, 0xF, false));
    m = min(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x140, 0xF, 0xF, false));
    return m;
}
// first_max over the 8 scores of a resident decoder's draw, where chain_combine leaves them: classes 0..3 in lanes 0..3, classes 4..7
// in lanes 32..35 (the other lanes hold anything).  Returns, wave-uniform, the winner's class kb and its score `best` (that lane's own
// bits), as first_max taken over classes 0..7 gives them: the quad maximum of the ordered image by two DPP steps, the larger of the
// two quads' maxima, and the lowest class among the lanes that hold it.  `sc + 0.0f` turns -0 into +0 first, so that the two
// zeros tie as they do under `>` (and the lower class wins); the returned bits are the untouched ones.  Equal to first_max for every
// input without NaN, +-inf included.  With a NaN it is not: first_max never lets a NaN in behind class 0 and never replaces one at
// class 0, here a NaN's image orders it above +inf (sign clear) or below -inf (sign set) like any other bit pattern.  Logits and
// noise are finite whenever weights and state are.  Denormal scores keep their order because `sc + 0.0f` keeps them: the library is
// built with fp32 denormals preserved (hipcc's default); flushed, they would all tie with zero (the probe's denormal cases guard it).
__device__ __forceinline__ void first_max_8lanes(float sc, float &best, int &kb) {
    const unsigned u = ordered(__float_as_uint(sc + 0.0f));
    unsigned m = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xF, 0xF, false));      // quad_perm [1,0,3,2]
    m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xF, 0xF, false));               // quad_perm [2,3,0,1]
    const unsigned mx = max((unsigned)__builtin_amdgcn_readlane((int)m, 0), (unsigned)__builtin_amdgcn_readlane((int)m, 32));
    const unsigned long long hit = __ballot(u == mx);
    const unsigned hit8 = ((unsigned)hit & 0xFu) | ((unsigned)(hit >> 28) & 0xF0u);                     // bit k: class k holds the maximum
    kb = __ffs((int)hit8) - 1;                                                                          // some lane holds the maximum: hit8 != 0
    best = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sc), kb < 4 ? kb : 28 + kb));
}

// Candidate granule of the launch path's fused schedule: {tag = step mod 2^22 (CAND_TAG_BITS), class < 1024, score}
__device__ __forceinline__ u64 cand_pack(unsigned tag, unsigned cls, float score) { return ((u64)((tag << 10) | cls) << 32) | __float_as_uint(score); }
__device__ __forceinline__ unsigned cand_tag(u64 g) { return (unsigned)(g >> 42); }
__device__ __forceinline__ int cand_class(u64 g) { return (int)((g >> 32) & 1023u); }
__device__ __forceinline__ float cand_score(u64 g) { return __uint_as_float((unsigned)g); }

// Sample x goes out (network_vocoder.py:78 output): its mu-law decoded value and, if asked for, the class itself.  The pointers keep
// their types (address spaces), so each site stores as it did.
template <class PW, class PM, class TB>
__device__ __forceinline__ void emit_sample(PW wav, PM mulaw, size_t at, int x, TB tab) {
    if (wav) wav[at] = tab[x];
    if (mulaw) mulaw[at] = x;
}

// A row's dot product over K = 64 NS runs as 8 fp32 fma chains, exactly those of the v_mfma_f32_16x16x4_f32 schedule of
// the launch-per-step kernels: K quarter kw (0..3) x accumulator c0 (0: the x/z fragment components, 1: y/w).  Term
// n = 8 s + 4 ci + q of chain (kw, c0) multiplies column k = 16 (kw NS + s) + 4 q + c0 + 2 ci; the row sum is
// ((q0 + q1) + q2) + q3 with q_kw = chain(kw, 0) + chain(kw, 1).
__device__ __forceinline__ int chain_col(int NS, int kw, int c0, int n) {
    return 16 * (kw * NS + (n >> 3)) + 4 * (n & 3) + c0 + 2 * ((n >> 2) & 1);
}
template <int NS>
__device__ __forceinline__ void ps_load_weights(const float *Wrow, int kw, int c0, float (&w)[8 * NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int ci = 0; ci < 2; ++ci)
#pragma unroll
            for (int kq = 0; kq < 4; ++kq) w[8 * s + 4 * ci + kq] = Wrow[16 * (kw * NS + s) + 4 * kq + c0 + 2 * ci];
}

#define PS_DPP(v, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), (ctrl), 0xF, 0xF, false))

// ---- in-kernel exchanges of the resident decoders (ar_xcd.hip, ar_xcm.hip): 8-byte {tag, value} granules -- the data is the
// flag.  Published with a store addressed as (uniform 64-bit base in SGPRs) + (32-bit byte offset in a VGPR): workgroup scope
// (sc0: the write-through L1 leaves the granule in this XCD's L2) or agent scope (sc1).  hipcc does not pad the hazard between
// a VALU write of the base SGPRs (v_readfirstlane) and a vector-memory instruction inside an asm statement reading them:
// every such statement opens with the five wait states itself.
__device__ __forceinline__ void xd_put(u64 *base, unsigned byte_off, u64 v, int agent) {
    if (agent) asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %2 sc1" :: "v"(byte_off), "v"(v), "s"(base) : "memory");
    else asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %2 sc0" :: "v"(byte_off), "v"(v), "s"(base) : "memory");   // stays in this XCD's L2
}

// four granules STEP bytes apart in ONE statement: one base register, immediate offsets, the five wait states once
template <int STEP>
__device__ __forceinline__ void xd_put4(u64 *base, unsigned byte_off, u64 v0, u64 v1, u64 v2, u64 v3, int agent) {
    if (agent) asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %5 sc1\n\tglobal_store_dwordx2 %0, %2, %5 offset:%6 sc1\n\t"
                            "global_store_dwordx2 %0, %3, %5 offset:%7 sc1\n\tglobal_store_dwordx2 %0, %4, %5 offset:%8 sc1"
                            :: "v"(byte_off), "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(base), "i"(STEP), "i"(2 * STEP), "i"(3 * STEP) : "memory");
    else asm volatile("s_nop 4\n\tglobal_store_dwordx2 %0, %1, %5 sc0\n\tglobal_store_dwordx2 %0, %2, %5 offset:%6 sc0\n\t"
                      "global_store_dwordx2 %0, %3, %5 offset:%7 sc0\n\tglobal_store_dwordx2 %0, %4, %5 offset:%8 sc0"
                      :: "v"(byte_off), "v"(v0), "v"(v1), "v"(v2), "v"(v3), "s"(base), "i"(STEP), "i"(2 * STEP), "i"(3 * STEP) : "memory");
}

// ---- 4-byte exchange WORDS (ar_xcd.hip, the instantiations xd_words() names in ar_chain.h): the value's own bits with ONE spare bit
// replaced by the parity of the step, (t + 1) & 1 -- the low bit of what the 8-byte granules carry as their tag.  Half the bytes of a
// granule, and four values per 16-byte load.  The spare bits: h_t is a convex combination of values in [-1, 1], so |h| < 2 and bit 30 of
// its fp32 image (the exponent's top bit) is 0; a_t = max(0, .) is neither negative nor NaN, so bit 31 is 0 (-0 never gets there:
// max(0, -0) and `v > 0 ? v : 0` give +0 -- and if it did, the cleared bit would make it +0, which no fmaf into an accumulator that
// started at +0 can tell from -0).
// Why one bit is enough.  A worker publishes h_t only after it has picked x_{t-1}; that pick needs every worker's candidate of step
// t - 1; a worker publishes its candidate only after its own gathers of h_{t-1} and a_{t-1} are complete.  So when ANY word of step t
// is written, every reader has finished with step t - 1, and a reader looking for step t has already seen step t - 1 at that address:
// the location holds step t - 1 (the other parity) or step t, nothing older -- the sc1 loads are served by L2, where a location does
// not go backwards.  The same chain holds for a_t (published behind the gather of h_t, which is behind x_{t-1}).  The launcher zeroes
// the area, so an untouched word reads parity 0 and the first step (t = 0) publishes parity 1; a call that aborts leaves the kernel,
// and the next launch zeroes the area again.
// A hidden value with bit 30 set -- NaN, +-inf or |h| >= 2, from non-finite weights or conditioning or a resumed h_in -- does not fit:
// xd_word_h_fits says so, and the publisher ends the call (STATUS_RANGE) as a timeout would.
constexpr unsigned XD_HBIT = 1u << 30, XD_ABIT = 1u << 31;
__device__ __forceinline__ unsigned xd_word_h(float v, unsigned parity) { return (__float_as_uint(v) & ~XD_HBIT) | (parity << 30); }
__device__ __forceinline__ bool xd_word_h_fits(float v) { return (__float_as_uint(v) & XD_HBIT) == 0u; }
__device__ __forceinline__ bool xd_word_h_ok(unsigned w, unsigned parity) { return ((w >> 30) & 1u) == parity; }
__device__ __forceinline__ float xd_word_h_value(unsigned w) { return __uint_as_float(w & ~XD_HBIT); }
__device__ __forceinline__ unsigned xd_word_a(float v, unsigned parity) { return (__float_as_uint(v) & ~XD_ABIT) | (parity << 31); }
__device__ __forceinline__ bool xd_word_a_fits(float v) { return (__float_as_uint(v) & XD_ABIT) == 0u; }
__device__ __forceinline__ bool xd_word_a_ok(unsigned w, unsigned parity) { return (w >> 31) == parity; }
__device__ __forceinline__ float xd_word_a_value(unsigned w) { return __uint_as_float(w & ~XD_ABIT); }
// The four words of a 16-byte chunk, each validated by its own bit, with as few vector instructions as it takes: the sweeps run on
// SIMDs whose issue ports the other waves' matrix chains keep busy, where every vector instruction costs 10..20 ns
// (profiles/r15_ab_exchange_words.txt: 13 per chunk instead of 8 gave the format's whole gain back).
// h_t: x = word ^ (parity << 30) IS xd_word_h_value(word) if xd_word_h_ok(word, parity) -- the bit is cleared -- and has bit 30 set
// if the word is of the other parity: four xors open the chunk, xd_chunk_h_ok tests the four bits at once.
typedef unsigned xd_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ xd_u32x4 xd_chunk_h_open(const xd_u32x4 &w, unsigned parity) {
    const unsigned pb = parity << 30;
    return xd_u32x4{w[0] ^ pb, w[1] ^ pb, w[2] ^ pb, w[3] ^ pb};
}
__device__ __forceinline__ bool xd_chunk_h_ok(const xd_u32x4 &x) { return ((x[0] | x[1] | x[2] | x[3]) & XD_HBIT) == 0u; }
// a_t: the bit is the sign, and the reader's products take |word| (fmac8a, ar_chain.h), so the words are used as they are; the four
// xd_word_a_ok at once: parity 1 <=> the AND of the four is negative, parity 0 <=> their OR is not (`parity` is wave-uniform)
__device__ __forceinline__ bool xd_chunk_a_ok(const xd_u32x4 &w, unsigned parity) {
    return parity ? (int)(w[0] & w[1] & w[2] & w[3]) < 0 : (int)(w[0] | w[1] | w[2] | w[3]) >= 0;
}
// one word / one chunk of four published with one store, addressed and scoped as xd_put
__device__ __forceinline__ void xd_put_word(u64 *base, unsigned byte_off, unsigned w, int agent) {
    if (agent) asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %2 sc1" :: "v"(byte_off), "v"(w), "s"(base) : "memory");
    else asm volatile("s_nop 4\n\tglobal_store_dword %0, %1, %2 sc0" :: "v"(byte_off), "v"(w), "s"(base) : "memory");
}
__device__ __forceinline__ void xd_put_chunk(u64 *base, unsigned byte_off, xd_u32x4 w, int agent) {
    if (agent) asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc1" :: "v"(byte_off), "v"(w), "s"(base) : "memory");
    else asm volatile("s_nop 4\n\tglobal_store_dwordx4 %0, %1, %2 sc0" :: "v"(byte_off), "v"(w), "s"(base) : "memory");
}

struct Waiter {                      // bounded spinning shared by all sweeps of the kernel
    unsigned *status;
    unsigned ticks;
    u64 t0;
    // The wall clock (s_memrealtime: a scalar memory read, ~0.3 us) is only consulted once a wait has spun 64 times: a wait
    // that succeeds quickly never pays for it.  t0 = 0: not taken yet.
    __device__ __forceinline__ void start() { t0 = 0; }
    // true: give up (deadline passed -- STATUS_TIMEOUT is then set -- or somebody else already gave up).  `tagp`: an LDS word with the
    // call's epoch << 8, so that the status word says WHICH call of the handle gave up; it is read only when the deadline has
    // passed (kept in a register for the whole call, the tag cost ar_xcd_kernel<2> a VGPR spill inside its sample loop)
    __device__ __forceinline__ bool expired(unsigned spins, int lane, const int *tagp) {
        if ((spins & 63) != 63) return false;
        const u64 now = __builtin_amdgcn_s_memrealtime();
        if (t0 == 0) t0 = now;
        const bool late = now - t0 > (u64)ticks;
        if (late && lane == 0) __hip_atomic_store(status, (unsigned)*tagp | STATUS_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // host-mapped: a plain store, no PCIe atomic
        return late || (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u);
    }
};
