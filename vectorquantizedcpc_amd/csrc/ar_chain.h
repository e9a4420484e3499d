// Device helpers of the per-XCD resident decoders (ar_xcd.hip, and ar_xcm.hip for the dimensions and the placement check; the
// pipelined variant of round 4, measured and dropped: profiles/r04_xcp_experiment.md): dimensions, the placement check, granule
// loads, and a row's fp32 fma chains on the vector ALU, on v_fmac_f32_dpp -- the same 8
// chains per row as the MFMA schedule of the launch-per-step kernels (ar_shared.h), combined in the same order.
#pragma once
#include "ar_xcd.h"
#include "ar_shared.h"

namespace {

constexpr int HR = 896, HF = 256, NC = 256;
constexpr int NW = 32;                 // workgroups per XCD
constexpr int UPB = 28;                // hidden units per workgroup
constexpr int ROWS = 3 * UPB;          // W_hh rows per workgroup
constexpr int FPB = 8;                 // fc1 rows / fc2 classes per workgroup
constexpr int THREADS = 768;
constexpr int NT_H = HR / 8;           // terms of a chain over h: 112
constexpr int NT_A = HF / 8;           // terms of a chain over a: 32

// Which instantiations exchange h_t / a_t as 4-byte words (ar_shared.h: xd_word_h / xd_word_a) instead of 8-byte {tag, value} granules:
// bit BXT of the two masks (the exchanges are independent: either can be built alone).  h_t: four slots per XCD do; one and two
// slots keep the granules until they have been measured under the same rule.  a_t: none -- at four slots it measured 0.1 us per
// step slower than the granules (profiles/r15_ab_exchange_words.txt); the code stays for the next look at it.
// -DXD_WORDS_H=7 -DXD_WORDS_A=7 builds all three on words, 0 none.  Candidates are granules either way.
#ifndef XD_WORDS_H
#define XD_WORDS_H 4
#endif
#ifndef XD_WORDS_A
#define XD_WORDS_A 0
#endif
__host__ __device__ constexpr bool xd_words_h(int bxt) { return (XD_WORDS_H & bxt) != 0; }
__host__ __device__ constexpr bool xd_words_a(int bxt) { return (XD_WORDS_A & bxt) != 0; }
// exchange area of one XCD, in 8-byte units (a granule, or two words)
__host__ __device__ constexpr int xg_h(int bxt) { return NW * bxt * (xd_words_h(bxt) ? 16 : 32); }   // [rank][slot][32] (28 used): granules two whole lines, words one
__host__ __device__ constexpr int xg_a(int bxt) { return bxt * NW * FPB / (xd_words_a(bxt) ? 2 : 1); }   // [slot][rank][8]: a slot's 256 are one run of 2 KB (granules) or 1 KB (words)
__host__ __device__ constexpr int xg_c() { return NW * 16; }                      // [slot < 16][rank]: a slot's 32 candidates are contiguous
__host__ __device__ constexpr int xg_region(int bxt) { return xg_h(bxt) + xg_a(bxt) + xg_c(); }
constexpr int CTL_WORDS = 64;          // u32: arrivals per XCC [0..7], total [8]
// byte offset of a_t row `row` (0..7) of worker `rank`, slot `slot`, in the a_t region
__device__ __forceinline__ unsigned xg_a_off(unsigned rank, unsigned row, unsigned slot) { return (((slot * NW + rank) << 3) + row) * 8u; }
// the same for words; and the byte offset of h_t chunk q (units 4 q .. 4 q + 3, q < 7) of (rank, slot) in the h_t region of words
__device__ __forceinline__ unsigned xg_a_off_w(unsigned rank, unsigned row, unsigned slot) { return (((slot * NW + rank) << 3) + row) * 4u; }
__device__ __forceinline__ unsigned xg_h_off_w(unsigned rank, unsigned slot, unsigned bxt, unsigned unit) { return (((rank * bxt + slot) << 5) + unit) * 4u; }
// one fc1 row of step `tag` - 1 goes out, as a word or as a granule
template <bool WORDS>
__device__ __forceinline__ void xd_put_a(u64 *ga, unsigned rank, unsigned row, unsigned slot, float v, unsigned tag, int agent) {
    if constexpr (WORDS) xd_put_word(ga, xg_a_off_w(rank, row, slot), xd_word_a(v, tag & 1u), agent);
    else xd_put(ga, xg_a_off(rank, row, slot), ((u64)tag << 32) | __float_as_uint(v), agent);
}

// Placement, run by ONE thread per workgroup: which XCD am I on (xid), which of its workers am I (rank, a ticket)?  Waits, bounded, until
// the whole grid has taken its tickets; false unless every XCD was dealt exactly `nw` workgroups (STATUS_MISPLACED is then set).  The
// control words are the first CTL_WORDS of the exchange area, zeroed by the launcher.
__device__ __forceinline__ bool xd_place(const XdParams &p, int nw, unsigned &xid, unsigned &rank) {
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xid));
    xid &= 7u;
    if (p.dbg_misplace && blockIdx.x == 0) xid = (xid + 1u) & 7u;      // tests: one workgroup reports the wrong XCD
    unsigned *ctl = (unsigned *)p.xg;
    rank = __hip_atomic_fetch_add(ctl + xid, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(ctl + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool ok = true;
    const u64 t0 = __builtin_amdgcn_s_memrealtime();
    for (unsigned spins = 0; __hip_atomic_load(ctl + 8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < gridDim.x; ++spins) {
        if ((spins & 63) == 63 && (__builtin_amdgcn_s_memrealtime() - t0 > (u64)p.timeout_ticks ||
                                   __hip_atomic_load(p.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u)) { ok = false; break; }
        __builtin_amdgcn_s_sleep(2);
    }
    if (ok)
        for (int x = 0; x < 8; ++x)
            if (__hip_atomic_load(ctl + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (unsigned)nw) ok = false;
    if (!ok) __hip_atomic_store(p.status, p.status_tag | STATUS_MISPLACED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return ok;
}

// Granule traffic is addressed as (uniform 64-bit base in SGPRs) + (32-bit byte offset in a VGPR) + immediate: a 64-bit
// address per lane and granule costs two VGPRs each, and the chain waves have none to spare.  The loads are sc1 (served by
// L2, not by this CU's L1); each helper issues its loads together and returns when they have landed (hipcc does not count
// the memory operations of an asm statement, so the wait is part of it; nor does it pad the hazard between a VALU write of
// the base SGPRs (v_readfirstlane) and a vector-memory instruction inside the statement reading them: every statement
// opens with the five wait states itself -- without them the stamped build and the 2-slot instantiation faulted).
template <int STEP>
__device__ __forceinline__ void gran_load1(u64 (&v)[1], const u64 *base, unsigned off) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %1, %2 sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v[0]) : "v"(off), "s"(base) : "memory");
}
template <int STEP>
__device__ __forceinline__ void gran_load2(u64 (&v)[2], const u64 *base, unsigned off) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %2, %3 sc1\n\tglobal_load_dwordx2 %1, %2, %3 offset:%4 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"(off), "s"(base), "i"(STEP) : "memory");
}
template <int STEP>
__device__ __forceinline__ void gran_load4(u64 (&v)[4], const u64 *base, unsigned off) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %4, %5 sc1\n\tglobal_load_dwordx2 %1, %4, %5 offset:%6 sc1\n\t"
                 "global_load_dwordx2 %2, %4, %5 offset:%7 sc1\n\tglobal_load_dwordx2 %3, %4, %5 offset:%8 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(off), "s"(base), "i"(STEP), "i"(2 * STEP), "i"(3 * STEP) : "memory");
}
// Two 16-byte chunks 1 KB apart, each TWO neighbouring granules, each granule validated by its own tag as ever (its publisher wrote it
// with one 8-byte store): from L2 an 8-byte sc1 access moves 0.54..0.70 of what a 16-byte one does.
typedef xd_u32x4 u32x4;
__device__ __forceinline__ void gran_chunks2(u32x4 (&v)[2], const u64 *base, unsigned off) {
    asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %2, %3 sc1\n\tglobal_load_dwordx4 %1, %2, %3 offset:1024 sc1\n\ts_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]) : "v"(off), "s"(base) : "memory");
}
// 16-byte chunks of four WORDS (ar_shared.h), one global_load_dwordx4 each: one chunk, or two in flight together.  A lane whose
// offset is XD_NO_CHUNK (its chunk belongs to a slot this XCD does not run, or it has none) does not load and keeps what `v` held: the
// statement narrows exec to the other lanes around the load and puts it back.
constexpr unsigned XD_NO_CHUNK = 0xFFFFFFFFu;
__device__ __forceinline__ void gran_load(u32x4 &v, const u64 *base, unsigned off) {
    u64 ex;
    asm volatile("s_nop 4\n\tv_cmp_ne_u32 vcc, -1, %2\n\ts_and_saveexec_b64 %1, vcc\n\tglobal_load_dwordx4 %0, %2, %3 sc1\n\t"
                 "s_mov_b64 exec, %1\n\ts_waitcnt vmcnt(0)"
                 : "+v"(v), "=&s"(ex) : "v"(off), "s"(base) : "memory", "vcc");
}
__device__ __forceinline__ void gran_load_pair(u32x4 &a, u32x4 &b, const u64 *base, unsigned off, unsigned off2) {
    u64 ex;
    asm volatile("s_nop 4\n\tv_cmp_ne_u32 vcc, -1, %3\n\ts_and_saveexec_b64 %2, vcc\n\tglobal_load_dwordx4 %0, %3, %5 sc1\n\t"
                 "s_mov_b64 exec, %2\n\tv_cmp_ne_u32 vcc, -1, %4\n\ts_and_saveexec_b64 %2, vcc\n\tglobal_load_dwordx4 %1, %4, %5 sc1\n\t"
                 "s_mov_b64 exec, %2\n\ts_waitcnt vmcnt(0)"
                 : "+v"(a), "+v"(b), "=&s"(ex) : "v"(off), "v"(off2), "s"(base) : "memory", "vcc");
}
// 2 N granules: N at `off` + i STEP and N at `off2` + i STEP, all in flight together
template <int N, int STEP>
__device__ __forceinline__ void gran_load_pair(u64 (&a)[N], u64 (&b)[N], const u64 *base, unsigned off, unsigned off2) {
    if constexpr (N == 1)
        asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %2, %4 sc1\n\tglobal_load_dwordx2 %1, %3, %4 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(a[0]), "=&v"(b[0]) : "v"(off), "v"(off2), "s"(base) : "memory");
    if constexpr (N == 2)
        asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %4, %6 sc1\n\tglobal_load_dwordx2 %1, %4, %6 offset:%7 sc1\n\t"
                     "global_load_dwordx2 %2, %5, %6 sc1\n\tglobal_load_dwordx2 %3, %5, %6 offset:%7 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(a[0]), "=&v"(a[1]), "=&v"(b[0]), "=&v"(b[1]) : "v"(off), "v"(off2), "s"(base), "i"(STEP) : "memory");
    if constexpr (N == 4)
        asm volatile("s_nop 4\n\tglobal_load_dwordx2 %0, %8, %10 sc1\n\tglobal_load_dwordx2 %1, %8, %10 offset:%11 sc1\n\t"
                     "global_load_dwordx2 %2, %8, %10 offset:%12 sc1\n\tglobal_load_dwordx2 %3, %8, %10 offset:%13 sc1\n\t"
                     "global_load_dwordx2 %4, %9, %10 sc1\n\tglobal_load_dwordx2 %5, %9, %10 offset:%11 sc1\n\t"
                     "global_load_dwordx2 %6, %9, %10 offset:%12 sc1\n\tglobal_load_dwordx2 %7, %9, %10 offset:%13 sc1\n\ts_waitcnt vmcnt(0)"
                     : "=&v"(a[0]), "=&v"(a[1]), "=&v"(a[2]), "=&v"(a[3]), "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                     : "v"(off), "v"(off2), "s"(base), "i"(STEP), "i"(2 * STEP), "i"(3 * STEP) : "memory");
}
template <int N, int STEP>
__device__ __forceinline__ void gran_load(u64 (&v)[N], const u64 *base, unsigned off) {
    if constexpr (N == 1) gran_load1<STEP>(v, base, off);
    if constexpr (N == 2) gran_load2<STEP>(v, base, off);
    if constexpr (N == 4) gran_load4<STEP>(v, base, off);
}

// acc += (value of `h` in lane J of this lane's quad) * w -- one fp32 fma, as the MFMA chain does it.  Eight (four)
// consecutive terms of a chain go into ONE asm statement: hipcc pads every asm statement with an s_nop, which at one
// fmac per statement doubled the instruction count of a chain (13 cycles per term measured; the terms of one statement
// need no padding among themselves: the accumulator is an ordinary operand, the DPP operand comes from LDS loads).
#define XD_QP(J) "quad_perm:[" #J "," #J "," #J "," #J "] row_mask:0xf bank_mask:0xf"
#define XD_FMAC8(J)                                                                                                      \
    asm("v_fmac_f32_dpp %0, %1, %9 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, %2, %10 " XD_QP(J) "\n\t"                        \
        "v_fmac_f32_dpp %0, %3, %11 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, %4, %12 " XD_QP(J) "\n\t"                       \
        "v_fmac_f32_dpp %0, %5, %13 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, %6, %14 " XD_QP(J) "\n\t"                       \
        "v_fmac_f32_dpp %0, %7, %15 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, %8, %16 " XD_QP(J)                              \
        : "+v"(acc)                                                                                                      \
        : "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]), "v"(h[5]), "v"(h[6]), "v"(h[7]),                       \
          "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]))
// the same on |h|: a_t exchange words carry the step's parity in their sign bit (ar_shared.h), and a_t = max(0, .) has none of its own
#define XD_FMAC8A(J)                                                                                                     \
    asm("v_fmac_f32_dpp %0, |%1|, %9 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, |%2|, %10 " XD_QP(J) "\n\t"                    \
        "v_fmac_f32_dpp %0, |%3|, %11 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, |%4|, %12 " XD_QP(J) "\n\t"                   \
        "v_fmac_f32_dpp %0, |%5|, %13 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, |%6|, %14 " XD_QP(J) "\n\t"                   \
        "v_fmac_f32_dpp %0, |%7|, %15 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, |%8|, %16 " XD_QP(J)                          \
        : "+v"(acc)                                                                                                      \
        : "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(h[4]), "v"(h[5]), "v"(h[6]), "v"(h[7]),                       \
          "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]), "v"(w[4]), "v"(w[5]), "v"(w[6]), "v"(w[7]))
#define XD_FMAC4(J)                                                                                                      \
    asm("v_fmac_f32_dpp %0, %1, %5 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, %2, %6 " XD_QP(J) "\n\t"                         \
        "v_fmac_f32_dpp %0, %3, %7 " XD_QP(J) "\n\tv_fmac_f32_dpp %0, %4, %8 " XD_QP(J)                                \
        : "+v"(acc)                                                                                                      \
        : "v"(h[0]), "v"(h[1]), "v"(h[2]), "v"(h[3]), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]))
// terms 8 J .. 8 J + 7 of a 32-term phase: operands h[0..7] as held by quad lane J, weights w[0..7]
template <int J, bool ABS = false>
__device__ __forceinline__ void fmac8(float &acc, const float *h, const float *w) {
    if constexpr (ABS) {
        if constexpr (J == 0) XD_FMAC8A(0);
        if constexpr (J == 1) XD_FMAC8A(1);
        if constexpr (J == 2) XD_FMAC8A(2);
        if constexpr (J == 3) XD_FMAC8A(3);
    } else {
        if constexpr (J == 0) XD_FMAC8(0);
        if constexpr (J == 1) XD_FMAC8(1);
        if constexpr (J == 2) XD_FMAC8(2);
        if constexpr (J == 3) XD_FMAC8(3);
    }
}
template <int J>
__device__ __forceinline__ void fmac4(float &acc, const float *h, const float *w) {
    if constexpr (J == 0) XD_FMAC4(0);
    if constexpr (J == 1) XD_FMAC4(1);
    if constexpr (J == 2) XD_FMAC4(2);
    if constexpr (J == 3) XD_FMAC4(3);
}
// one phase: len = 32 (8 terms per quad lane) or 16 (4 per lane); w = the phase's weights in term order
template <int LEN>
__device__ __forceinline__ void chain_phase(float &acc, const float (&hv)[8], const float *w) {
    if constexpr (LEN == 32) { fmac8<0>(acc, hv, w); fmac8<1>(acc, hv, w + 8); fmac8<2>(acc, hv, w + 16); fmac8<3>(acc, hv, w + 24); }
    else { fmac4<0>(acc, hv, w); fmac4<1>(acc, hv, w + 4); fmac4<2>(acc, hv, w + 8); fmac4<3>(acc, hv, w + 12); }
}

// Lane layout of a chain wave: lane = 16 R + 4 kw + j; R = 2 rq + c0.  The quad (j = 0..3) holds chain (kw, c0) of rows
// 4 rq + j.  Operand values of a chain sit in LDS chain by chain ([cid = 2 kw + c0][...]); they are used in PHASES of 32
// terms: in phase ph quad lane j holds terms 32 ph + 8 j .. + 7 (two 16-byte LDS words), so term n comes from quad lane
// (n % 32) / 8, register n % 8 -- 8 operand registers per phase instead of NT / 4 for the whole chain.  A last phase of 16
// terms (NT = 112) gives every lane 4.
// LDS order inside a phase: the four lanes' FIRST words, then their SECOND words (term 32 ph + 8 j + r sits at 32 ph + 16 (r / 4)
// + 4 j + r % 4), so that one ds_read_b128 of a quad covers 16 contiguous floats and the four chains of a 16-lane group (chain
// stride 112 or 48 floats = 48 mod 64 banks) cover all 64 banks: with the terms in plain order (lane j at 8 j) a quad's read had
// holes and chains cid / cid + 4 shared banks -- rocprofv3 counted 59 % of the LDS cycles of ar_xcd_kernel<4> as bank conflicts
// (profiles/r04_pmc_sq_xcd32.json, round 4's first pass).
// (the 16-term last phase of a 112-term chain keeps its plain order: lane j's one word at 4 j)
template <int NT>
__device__ __forceinline__ int phase_pos_t(int n) { return (NT % 32 != 0 && n >= NT - NT % 32) ? n : ((n & ~31) + ((n >> 2) & 1) * 16 + ((n >> 3) & 3) * 4 + (n & 3)); }
template <int NT>
__device__ __forceinline__ float chain_regs(const float *w, const float *opnd) {
    float acc = 0.f;
    constexpr int NPH = (NT + 31) / 32;
    float4 cur[2], nxt[2];                              // opnd = base + cid * stride + 4 j: this lane's first word of phase 0
    cur[0] = *(const float4 *)opnd; cur[1] = *(const float4 *)(opnd + 16);
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
        const int len = NT - 32 * ph < 32 ? NT - 32 * ph : 32;          // 32, or 16 in the last phase of 112
        if (ph + 1 < NPH) {
            const int nlen = NT - 32 * (ph + 1) < 32 ? NT - 32 * (ph + 1) : 32;
            nxt[0] = *(const float4 *)(opnd + 32 * (ph + 1));
            // a 16-term phase: lane j holds terms 4 j .. 4 j + 3 = its first word; there is no second
            nxt[1] = nlen == 32 ? *(const float4 *)(opnd + 32 * (ph + 1) + 16) : nxt[0];
        }
        const float hv[8] = {cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y, cur[1].z, cur[1].w};
        if (len == 32) chain_phase<32>(acc, hv, w + 32 * ph);
        else chain_phase<16>(acc, hv, w + 32 * ph);
        cur[0] = nxt[0]; cur[1] = nxt[1];
    }
    return acc;
}
// The same chain for ONE or TWO operand vectors (two decode slots) with its weights streamed from LDS a phase ahead of their use: a
// service wave must not hold 112 weights next to everything else it keeps (four slots, fc1 on wave 0: 112 pinned weights spill even
// with a loop of its own, and the fits of up to 9 pinned groups run slower than this -- profiles/r05_fc1_pin_sweep.txt).  The weights of a lane's chain are NT / 4 16-byte words,
// word i at wp[i * WS]: the words of the WS lane-chains of a wave are interleaved ([word][lane-chain]), so that a wave's read of word
// i is one contiguous run -- with a lane's chain contiguous ([lane-chain][NT], 448 bytes apart) the sixteen lanes of a read group hit
// four bank windows four ways each.  w0 = the weights of phase 0, already in registers (requested before the barrier the chain waits
// behind).
__device__ __forceinline__ void load_phase(const float *opnd, int ph, int nlen, float4 (&d)[2]) {
    d[0] = *(const float4 *)(opnd + 32 * ph);
    d[1] = nlen == 32 ? *(const float4 *)(opnd + 32 * ph + 16) : d[0];     // 16-term phase: lane j holds terms 4 j .. 4 j + 3 = the first word
}
template <int NT, int WS>
__device__ __forceinline__ void chain_lds2(const float4 *wp, const float4 (&w0)[8], const float *opA, const float *opB, bool two,
                                           float &accA, float &accB) {
    constexpr int NPH = (NT + 31) / 32;
    float4 curA[2], nxtA[2], curB[2], nxtB[2], wc[8], wn[8];
    load_phase(opA, 0, NT < 32 ? NT : 32, curA);
    if (two) load_phase(opB, 0, NT < 32 ? NT : 32, curB);
    else { curB[0] = curA[0]; curB[1] = curA[1]; }
#pragma unroll
    for (int i = 0; i < 8; ++i) wc[i] = w0[i];
    accA = 0.f; accB = 0.f;
#pragma unroll
    for (int ph = 0; ph < NPH; ++ph) {
        const int len = NT - 32 * ph < 32 ? NT - 32 * ph : 32;
        if (ph + 1 < NPH) {
            const int nlen = NT - 32 * (ph + 1) < 32 ? NT - 32 * (ph + 1) : 32;
            load_phase(opA, ph + 1, nlen, nxtA);
            if (two) load_phase(opB, ph + 1, nlen, nxtB);
#pragma unroll
            for (int i = 0; i < nlen / 4; ++i) wn[i] = wp[(8 * (ph + 1) + i) * WS];
        }
        __builtin_amdgcn_sched_barrier(0);
        float wv[32];
#pragma unroll
        for (int i = 0; i < 8; ++i) { wv[4 * i] = wc[i].x; wv[4 * i + 1] = wc[i].y; wv[4 * i + 2] = wc[i].z; wv[4 * i + 3] = wc[i].w; }
        {
            const float hv[8] = {curA[0].x, curA[0].y, curA[0].z, curA[0].w, curA[1].x, curA[1].y, curA[1].z, curA[1].w};
            if (len == 32) chain_phase<32>(accA, hv, wv);
            else chain_phase<16>(accA, hv, wv);
        }
        if (two) {
            const float hv[8] = {curB[0].x, curB[0].y, curB[0].z, curB[0].w, curB[1].x, curB[1].y, curB[1].z, curB[1].w};
            if (len == 32) chain_phase<32>(accB, hv, wv);
            else chain_phase<16>(accB, hv, wv);
        }
        __builtin_amdgcn_sched_barrier(0);
        curA[0] = nxtA[0]; curA[1] = nxtA[1]; curB[0] = nxtB[0]; curB[1] = nxtB[1];
#pragma unroll
        for (int i = 0; i < 8; ++i) wc[i] = wn[i];
    }
}

// the lane of a chain wave that holds chain cc (= 2 kw + c0) of the wave's row rr (0..7): inverse of the lane layout above
__device__ __forceinline__ unsigned xd_lane_of(unsigned rr, unsigned cc) { return 16u * (2u * (rr >> 2) + (cc & 1u)) + 4u * (cc >> 1) + (rr & 3u); }

// Row sum from the 8 chain lanes of a row: a0 + a1 across the two 16-lane rows of an rq pair (lane ^ 16), then
// ((q0 + q1) + q2) + q3 along the K quarters (lane + 4, + 8, + 12 inside the row) -- the order of the MFMA kernels.
// Meaningful in lanes with kw == 0 of the c0 = 0 rows (lanes 0..3 and 32..35: sum_lane).  The partner row comes through
// v_permlane16_swap_b32 (gfx950: the second operand's rows 0 and 2 receive the first operand's rows 1 and 3), not ds_swizzle: a
// swizzle is an LDS round trip, ~0.1 us behind the other waves' reads -- and four in a row, one per accumulator of a matrix-pipe
// chain, were 0.4 us of the step's critical path (fc1 -> a_t).
__device__ __forceinline__ float chain_combine(float acc) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc), __float_as_uint(acc), false, false);
    const float o = __uint_as_float(sw[1]);                                                        // rows 0 and 2: lane + 16
    const float q = acc + o;
    // ((q + q1) + q2) + q3, q_k = q of lane + 4 k: three v_add_f32_dpp (the shifted operand read in place) instead of three dpp moves and
    // three adds; s_nop 1: the two wait states between the add that wrote q and its first dpp read (hipcc does not look into the statement)
    float s;                                            // early clobber: q must stay what the second and third add shift
    asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %1 row_shl:4 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %1, %0 row_shl:8 row_mask:0xf bank_mask:0xf\n\t"
        "v_add_f32_dpp %0, %1, %0 row_shl:12 row_mask:0xf bank_mask:0xf" : "=&v"(s) : "v"(q));
    return s;
}

// position of operand column k in the LDS copy (inverse of chain_col): chain cid = 2 kw + c0 at cid * stride, term n at phase_pos(n)
template <int NS>
__device__ __forceinline__ int chain_pos(int k, int stride) {
    const int S = k >> 4, kw = S / NS, s = S - kw * NS;
    const int q = (k >> 2) & 3, c0 = k & 1, ci = (k >> 1) & 1;
    return (2 * kw + c0) * stride + phase_pos_t<8 * NS>(8 * s + 4 * ci + q);
}

// ---- the same chains on the matrix pipe, for the FOUR slots of an XCD at once (ar_xcd_kernel<4>).  v_mfma_f32_4x4x1_16B_f32 is
// sixteen independent 4x4 outer products, one per quad: lane 4 b + i supplies A_b[i], lane 4 b + j supplies B_b[j], and
// D_b[i][j] += A_b[i] * B_b[j] (one rounding: bit for bit fmaf -- tools/microbench_mfma4x4.hip) lands in register i of lane
// 4 b + j.  With the chain waves' lane layout (quad = chain (kw, c0) of rows 4 rq + 0..3) A is the lane's pinned weight of term
// n -- exactly what v_fmac_f32_dpp used -- and B is term n's operand of slot j = lane & 3: one instruction advances the chains of
// 4 rows x 4 slots, where the vector ALU needed 4 (one per slot).  Why: with three waves per SIMD a wave's 112-term dpp chain
// costs the SIMD 0.27 us whoever waits for it (tools/microbench_chain.hip: 0.80 us per pass for the last of three waves), the
// twelve passes of a 4-slot step 3.3 us -- the step was vector-ALU bound behind barrier A (tools/xcd_barriers.py: the youngest
// wave of every SIMD reaches barrier B 3.6 us after A, with or without the exchange waits); the matrix pipe does the four
// slots' chains of three waves in 1.5 us and leaves the vector ALU to the serial work.
// Operands: the lane reads ITS slot's copy of the chain itself, terms in plain order: hc[j * HS4 + cid * NT_H + n] -- 14
// ds_read_b128 per step, each half of the wave one word of a group's two (below; the dpp form reads 4 x 7).  Slot stride
// HS4 = HR + 4: the four lanes of a quad start one 16-byte unit apart, the four quads of a ds_read_b128 lane group (chains
// {0,6,3,5} or {2,4,1,7}, 28 units apart) 4 units apart -- 64 banks.
typedef float v4f __attribute__((ext_vector_type(4)));
constexpr int HS4 = HR + 4;
constexpr int NG_H = NT_H / 8;         // groups of 8 terms (two 16-byte operand words)
template <int NS>
__device__ __forceinline__ int chain_pos_plain(int k, int stride) {
    const int S = k >> 4, kw = S / NS, s = S - kw * NS;
    const int q = (k >> 2) & 3, c0 = k & 1, ci = (k >> 1) & 1;
    return (2 * kw + c0) * stride + 8 * s + 4 * ci + q;
}
// chain_combine of the FOUR accumulators of fc1's matrix-pipe chain at once, in ONE statement: the same adds in the same order per
// accumulator, interleaved -- the four are independent, so each fills the others' wait states and no s_nop is left between them.
// Hazards inside the statement, which hipcc does not pad: the matrix instruction that wrote `a` -> its first VALU read (four states
// for this two-pass instruction: s_nop 3); VALU write -> v_permlane16_swap or DPP read of the same register (two states; three
// instructions lie between each pair).  The swap takes the accumulator itself as its first operand: rows 0 and 2 of it, where the sum
// lanes and the lanes they shift in are, stay what they were; rows 1 and 3 are not used afterwards.
// fc1's epilogue rides along: s[i] = max(0, row sum i + b[i]), the v_add_f32 / v_max_f32 pair hipcc emits for `v += b; v = v > 0.f ? v : 0.f`
// (left to hipcc behind the statement they became packed adds, compare / select pairs with their own wait states, or a canonicalising
// v_max_f32 v, v, v in front of each ReLU).
__device__ __forceinline__ void fc1_finish4(const v4f &a, const float (&b)[4], float (&s)[4]) {
    float a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3], q0, q1, q2, q3;
#define XD_SHL(N) " row_shl:" #N " row_mask:0xf bank_mask:0xf\n\t"
    asm("s_nop 3\n\t"
        "v_mov_b32 %4, %8\n\tv_mov_b32 %5, %9\n\tv_mov_b32 %6, %10\n\tv_mov_b32 %7, %11\n\t"
        "v_permlane16_swap_b32 %8, %4\n\tv_permlane16_swap_b32 %9, %5\n\tv_permlane16_swap_b32 %10, %6\n\tv_permlane16_swap_b32 %11, %7\n\t"
        "v_add_f32 %4, %8, %4\n\tv_add_f32 %5, %9, %5\n\tv_add_f32 %6, %10, %6\n\tv_add_f32 %7, %11, %7\n\t"
        "v_add_f32_dpp %0, %4, %4" XD_SHL(4) "v_add_f32_dpp %1, %5, %5" XD_SHL(4) "v_add_f32_dpp %2, %6, %6" XD_SHL(4) "v_add_f32_dpp %3, %7, %7" XD_SHL(4)
        "v_add_f32_dpp %0, %4, %0" XD_SHL(8) "v_add_f32_dpp %1, %5, %1" XD_SHL(8) "v_add_f32_dpp %2, %6, %2" XD_SHL(8) "v_add_f32_dpp %3, %7, %3" XD_SHL(8)
        "v_add_f32_dpp %0, %4, %0" XD_SHL(12) "v_add_f32_dpp %1, %5, %1" XD_SHL(12) "v_add_f32_dpp %2, %6, %2" XD_SHL(12) "v_add_f32_dpp %3, %7, %3" XD_SHL(12)
        "v_add_f32 %0, %0, %12\n\tv_add_f32 %1, %1, %13\n\tv_add_f32 %2, %2, %14\n\tv_add_f32 %3, %3, %15\n\t"
        "v_max_f32 %0, 0, %0\n\tv_max_f32 %1, 0, %1\n\tv_max_f32 %2, 0, %2\n\tv_max_f32 %3, 0, %3"
        : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3]), "=&v"(q0), "=&v"(q1), "=&v"(q2), "=&v"(q3), "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3)
        : "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));
#undef XD_SHL
}

// ONE operand word per lane and group of 8 terms, not two.  A lane's operand depends on (kw, c0, j) and not on rq: lanes 32..63 would
// read exactly what lanes 0..31 read.  So the halves read DIFFERENT words -- lanes 0..31 terms 8 g .. 8 g + 3, lanes 32..63 terms
// 8 g + 4 .. 8 g + 7 (`op` carries the half's offset, 4 rq floats) -- and the instruction's B lane-group pattern picks the half that
// holds the term: pattern 1 = both halves take B from lanes 0..31, pattern 2 = both take it from lanes 32..63; the other half's
// register is ignored, whatever it holds (tools/microbench_mfma4x4.hip).  A stays per lane.  Same bits: every accumulator still sees
// fmaf(w[n], h[n], acc) for n = 0 .. 111 in order, with the values it saw before -- only the register the value comes from differs.
// 14 operand reads per wave and step instead of 28; inside each 16-lane group of a ds_read_b128 all lanes moved by the same 16 bytes,
// so the bank picture above holds.
__device__ __forceinline__ void mfma_group8(v4f &acc, const float *w, const float4 &h) {
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[0], h.x, acc, 0, 0, 1);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[1], h.y, acc, 0, 0, 1);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[2], h.z, acc, 0, 0, 1);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[3], h.w, acc, 0, 0, 1);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[4], h.x, acc, 0, 0, 2);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[5], h.y, acc, 0, 0, 2);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[6], h.z, acc, 0, 0, 2);
    acc = __builtin_amdgcn_mfma_f32_4x4x1f32(w[7], h.w, acc, 0, 0, 2);
}
// groups [G0, G1) of the chain, weights pinned (w[n] = term n); cur = this half's operand word of group G0, already requested (it
// leaves with that of group G1: a chain can pause between two calls without losing its prefetch)
template <int G0, int G1>
__device__ __forceinline__ void chain_mfma_regs(v4f &acc, const float *w, const float *op, float4 &cur) {
#pragma unroll
    for (int g = G0; g < G1; ++g) {
        float4 nxt = cur;
        __builtin_amdgcn_sched_barrier(0);
        mfma_group8(acc, w + 8 * g, cur);
        // the next group's operands are requested BEHIND this group's terms (in front of them: 3.73 instead of 3.69 us per step at 32
        // utterances): three waves share the pipe, the read comes back while the other two run their groups
        if (g + 1 < NG_H) nxt = *(const float4 *)(op + 8 * (g + 1));
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
    }
}
// the whole chain with its weights streamed from the word-interleaved LDS copy (word i of the lane's chain at wp[i * WS]), D groups
// ahead of their use -- weights AND operands: behind barrier A a ds_read_b128 comes back after ~300 cycles (twelve waves read), a
// group's 8 dependent matrix instructions take ~140, and with one group of prefetch the chain ran at the LDS latency (fc1, the first
// thing on the step's critical path: 1.9 us; profiles/r04_mfma_chains.txt).  wpre = words 0 .. 2 D - 1, requested before the barrier
// the chain waits behind.  A group is THREE reads -- the half's operand word (mfma_group8) and the lane's two weight words: A is not
// shared between the halves (WS = 32, rows 80..83: both halves read lane & 31's chain and run the same products) -- so five groups
// fit under the 4-bit lgkmcnt counter where four reads per group allowed three.
template <int WS, int D>
__device__ __forceinline__ v4f chain_mfma_lds(const float4 *wp, const float4 *wpre, const float *op) {
    static_assert(3 * D <= 15, "reads in flight: lgkmcnt counts to 15");
    v4f acc = {0.f, 0.f, 0.f, 0.f};
    float4 hb[D], wb[D][2];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        hb[d] = *(const float4 *)(op + 8 * d);
        wb[d][0] = wpre[2 * d]; wb[d][1] = wpre[2 * d + 1];
    }
#pragma unroll
    for (int g = 0; g < NG_H; ++g) {
        const int s = g % D;
        __builtin_amdgcn_sched_barrier(0);
        const float wv[8] = {wb[s][0].x, wb[s][0].y, wb[s][0].z, wb[s][0].w, wb[s][1].x, wb[s][1].y, wb[s][1].z, wb[s][1].w};
        mfma_group8(acc, wv, hb[s]);
        __builtin_amdgcn_sched_barrier(0);
        if (g + D < NG_H) {                                     // refill the buffer just used with group g + D
            hb[s] = *(const float4 *)(op + 8 * (g + D));
            wb[s][0] = wp[(2 * (g + D)) * WS]; wb[s][1] = wp[(2 * (g + D) + 1) * WS];
        }
    }
    return acc;
}

}  // namespace
