// encoder.hip -- the kernels of Encoder.encode / Encoder.forward on gfx950 (reference: model.py:43-155); the handle and the
// vqcpc_encoder_* entry points are in encoder_host.hip, the layered schedule's GEMM in gemm_chain.hip.
//
// Every kernel here reproduces the rounding sequence of the reference's PyTorch-CPU path
// (oracle/vqcpc_oracle.c documents each order and tests pin it against the reference):
//   * contractions are fp32 MFMA chains (v_mfma_f32_16x16x4_f32 == a k-ordered fmaf chain),
//     restarted at the K-block boundaries the reference's MKL / oneDNN kernels use;
//   * LayerNorm moments follow ATen's 8-lane Welford cascade;
//   * |x|^2 follows ATen's cascade_sum order; the VQ distance is one fma per (row, code).
// Build with -ffp-contract=off: every fused multiply-add below is written explicitly.
#include "encoder_internal.h"
#include <math.h>

// ------------------------------------------------------------------------------------------
// LayerNorm(512) + optional ReLU, ATen CPU order (see oracle orc_ln_moments).
// One half-wave (32 lanes) per row: lane = chunk*8 + l runs the Welford chain of vector lane
// l over chunk `chunk` (16 vectors of 8), merges by shuffles, then all lanes normalise.
// ------------------------------------------------------------------------------------------
// (mean, rstd) of the 512-float row x (global or LDS) on the calling thread's half-wave; every lane of it returns them.
// (The half-wave and the lane in it are taken from threadIdx here: handed in as arguments, the same values cost ln512_kernel
// 15 instructions and enc_fused_kernel 4 VGPRs -- and with them its third wave per SIMD.)
__device__ __forceinline__ float2 ln512_moments(const float *x, const LnConst &k, float eps) {
    const int lane = threadIdx.x & 63, half = lane >> 5, ll = lane & 31;
    const int chunk = ll >> 3, l = ll & 7;
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float xv = x[(chunk * 16 + j) * 8 + l];
        const float d = xv - m1;
        m1 = __builtin_fmaf(d, k.inv[j], m1);
        m2 = __builtin_fmaf(d, xv - m1, m2);
    }
    // chunk 1 -> chunk 0, chunk 3 -> chunk 2   (AddMomentsVec, 16 + 16 vectors, c = 1/2)
    float a1 = __shfl_down(m1, 8), a2 = __shfl_down(m2, 8);
    {
        const float delta = a1 - m1;
        const float n1 = __builtin_fmaf(0.5f, delta, m1);
        m2 = __builtin_fmaf((0.5f * 16.0f) * delta, delta, m2 + a2);
        m1 = n1;
    }
    // (chunks 2,3) -> (chunks 0,1)              (32 + 32 vectors)
    a1 = __shfl_down(m1, 16); a2 = __shfl_down(m2, 16);
    {
        const float delta = a1 - m1;
        const float n1 = __builtin_fmaf(0.5f, delta, m1);
        m2 = __builtin_fmaf((0.5f * 32.0f) * delta, delta, m2 + a2);
        m1 = n1;
    }
    // the 8 vector lanes, serially (AddMoments, scalar)
    float M1 = 0.f, M2 = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float s1 = __shfl(m1, half * 32 + q), s2 = __shfl(m2, half * 32 + q);
        const float delta = s1 - M1;
        M1 = __builtin_fmaf(k.sc[q], delta, M1);
        M2 = M2 + __builtin_fmaf((delta * delta) * k.sc[q], (float)(64 * q), s2);
    }
    const float var = M2 / 512.0f;
    // 1 / sqrt(var + eps), both correctly rounded in fp32 (via fp64: innocuous double rounding)
    const float sd = (float)sqrt((double)(var + eps));
    return make_float2(M1, (float)(1.0 / (double)sd));
}

__global__ __launch_bounds__(256) void ln512_kernel(const float *__restrict__ X, const float *__restrict__ g,
                                                    const float *__restrict__ b, float *__restrict__ Y, int M,
                                                    float eps, int relu, LnConst k, float *__restrict__ stat) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, ll = lane & 31;
    const int row = (blockIdx.x * 4 + wave) * 2 + half;
    const int rr = row < M ? row : M - 1;
    const float *x = X + (size_t)rr * 512;
    const float2 mr = ln512_moments(x, k, eps);
    const float mean = mr.x, rstd = mr.y;
    if (row < M) {
        if (stat && ll == 0) { stat[2 * (size_t)row] = mean; stat[2 * (size_t)row + 1] = rstd; }   // kept for the backward (front_grad.hip)
        float *y = Y + (size_t)row * 512;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = q * 128 + ll * 4;
            const float4 xv = *(const float4 *)(x + e);
            const float4 gv = *(const float4 *)(g + e);
            const float4 bv = *(const float4 *)(b + e);
            float4 o;
            o.x = __builtin_fmaf((xv.x - mean) * rstd, gv.x, bv.x);
            o.y = __builtin_fmaf((xv.y - mean) * rstd, gv.y, bv.y);
            o.z = __builtin_fmaf((xv.z - mean) * rstd, gv.z, bv.z);
            o.w = __builtin_fmaf((xv.w - mean) * rstd, gv.w, bv.w);
            if (relu) {
                o.x = o.x < 0.f ? 0.f : o.x; o.y = o.y < 0.f ? 0.f : o.y;
                o.z = o.z < 0.f ? 0.f : o.z; o.w = o.w < 0.f ? 0.f : o.w;
            }
            *(float4 *)(y + e) = o;
        }
    }
}

// ------------------------------------------------------------------------------------------
// torch.sum(v**2, dim=1) over 64 floats, ATen cascade order (oracle orc_sumsq64).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float sumsq64(const float *v) {
    float sq[64];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 t = *(const float4 *)(v + 4 * i);
        sq[4 * i + 0] = t.x * t.x; sq[4 * i + 1] = t.y * t.y; sq[4 * i + 2] = t.z * t.z; sq[4 * i + 3] = t.w * t.w;
    }
    float acc = 0.f;
#pragma unroll
    for (int l = 0; l < 8; ++l) {
        const float q0 = sq[l] + sq[32 + l], q1 = sq[8 + l] + sq[40 + l];
        const float q2 = sq[16 + l] + sq[48 + l], q3 = sq[24 + l] + sq[56 + l];
        acc += ((q0 + q1) + q2) + q3;
    }
    return acc;
}
__global__ void rowsumsq64_kernel(const float *__restrict__ X, float *__restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sumsq64(X + (size_t)i * 64);
}

// ------------------------------------------------------------------------------------------
// VQEmbeddingEMA.encode (model.py:103-115) in one kernel: |x|^2, the distance matrix row block,
// first-index argmin and the F.embedding gather.  One 256-thread workgroup per 16 rows; each wave owns a
// quarter of the codes and runs them as 16x16 tiles on v_mfma_f32_16x16x4_f32 with ONE accumulator per
// tile, so a dot product is the k-ascending fmaf chain of the reference's addmm (K = 64 is a single MKL
// block); two tiles are interleaved to cover the MFMA's dependent latency.
// Codebook fragments: Ef[(t*4 + q)*64 + lane] (float4) = E[16t + (lane&15)][16q + 4c + (lane>>4)], c = .x.y.z.w
// ------------------------------------------------------------------------------------------
__global__ void vq_build_frag_kernel(const float *__restrict__ E, float4 *__restrict__ Ef, int n_emb) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= n_emb * 16) return;
    const int lane = id & 63, q = (id >> 6) & 3, t = id >> 8;
    const float *r = E + (size_t)(16 * t + (lane & 15)) * 64 + 16 * q + (lane >> 4);
    Ef[id] = make_float4(r[0], r[4], r[8], r[12]);
}

__device__ __forceinline__ void vq_load_tile(const float4 *__restrict__ Ef, int t, int lane, float4 (&f)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) f[q] = Ef[(size_t)(t * 4 + q) * 64 + lane];
}
__device__ __forceinline__ void vq_take(const f32x4 &acc, int code, float e2, const float (&x2)[4], float (&bd)[4], int (&bj)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float d = __builtin_fmaf(-2.0f, acc[r], e2 + x2[r]);
        if (d < bd[r]) { bd[r] = d; bj[r] = code; }
    }
}

// Waves of a 512-thread workgroup that search: all 8 when the 16-code tiles divide among them, else 4 (vq_encode_kernel has 4).
__device__ __forceinline__ int vq_search_waves(int n_emb) { return n_emb % 128 == 0 ? 8 : 4; }
// The first two codebook tiles of a searching wave, requested ahead of the rows (vq_rows16 takes them as f0_in / f1_in): a wave
// owns n_emb / (16 nwv) consecutive tiles, and one with a single tile gets it twice.
__device__ __forceinline__ void vq_first_tiles(const float4 *__restrict__ Ef, int n_emb, int nwv, int wave, int lane, float4 (&f0)[4],
                                               float4 (&f1)[4]) {
    const int tpw = n_emb / (16 * nwv), t0 = wave * tpw;
#pragma unroll
    for (int q = 0; q < 4; ++q) f0[q] = f1[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (wave < nwv) {
        vq_load_tile(Ef, t0, lane, f0);
        vq_load_tile(Ef, tpw > 1 ? t0 + 1 : t0, lane, f1);
    }
}

// Shared tail of the VQ search: xs / x2s hold the 16 rows (and their |x|^2) of the block starting at row r0.
struct VqSmem {
    float xs[16][68];
    float x2s[16];
    float cd[8][16];
    int cj[8][16];
    int best[16];
};
__device__ __forceinline__ void vq_rows16(VqSmem &sm, int r0, int N, const float4 *__restrict__ Ef, const float *__restrict__ E,
                                          const float *__restrict__ e2, int n_emb, int64_t *__restrict__ idx,
                                          float *__restrict__ zq, int tid, const float4 (&f0_in)[4], const float4 (&f1_in)[4],
                                          int nwv = 4) {
    // nwv = waves that search (4, or 8 of a 512-thread workgroup when the tiles divide); waves beyond only keep the two
    // barriers company
    const bool active = (tid >> 6) < nwv;                              // wave-uniform
    const int lane = tid & 63, wave = active ? tid >> 6 : 0;
    const int tpw = active ? n_emb / (16 * nwv) : 0, t0 = wave * tpw;  // 16-code tiles per wave, this wave's first
    float4 f0[4], f1[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { f0[q] = f0_in[q]; f1[q] = f1_in[q]; }
    float a[16], x2[4], bd[4];
    int bj[4];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = sm.xs[lane & 15][4 * j + (lane >> 4)];
#pragma unroll
    for (int r = 0; r < 4; ++r) { x2[r] = sm.x2s[4 * (lane >> 4) + r]; bd[r] = __builtin_inff(); bj[r] = 0; }

    int tt = 0;
    for (; tt + 1 < tpw; tt += 2) {
        const int t = t0 + tt, c0 = 16 * t + (lane & 15);
        const float ea = e2[c0], eb = e2[c0 + 16];
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 0], f0[q].x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 0], f1[q].x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 1], f0[q].y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 1], f1[q].y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 2], f0[q].z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 2], f1[q].z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 3], f0[q].w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 3], f1[q].w, acc1, 0, 0, 0);
        }
        if (tt + 2 < tpw) vq_load_tile(Ef, t + 2, lane, f0);           // next pair streams in under the compares
        if (tt + 3 < tpw) vq_load_tile(Ef, t + 3, lane, f1);
        vq_take(acc0, c0, ea, x2, bd, bj);
        vq_take(acc1, c0 + 16, eb, x2, bd, bj);
    }
    if (tt < tpw) {                                                    // odd tile count: last tile alone
        const int c0 = 16 * (t0 + tt) + (lane & 15);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 0], f0[q].x, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 1], f0[q].y, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 2], f0[q].z, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * q + 3], f0[q].w, acc0, 0, 0, 0);
        }
        vq_take(acc0, c0, e2[c0], x2, bd, bj);
    }
    // first-index argmin: over the 16 codes of a lane group, then over the four waves (ascending codes).  The lexicographic
    // (distance, index) minimum is idempotent, so four DPP exchanges inside the row of 16 lanes (pairs, quads, the mirrored
    // half, the mirrored row) leave it in every lane -- no ds_bpermute round trips.
#define VQ_DPP_MIN(ctrl)                                                                                        \
    {                                                                                                           \
        const float od = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(bd[r]), (ctrl), 0xF, 0xF, false)); \
        const int oj = __builtin_amdgcn_update_dpp(0, bj[r], (ctrl), 0xF, 0xF, false);                          \
        if (od < bd[r] || (od == bd[r] && oj < bj[r])) { bd[r] = od; bj[r] = oj; }                              \
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        VQ_DPP_MIN(0xB1)            // quad_perm [1,0,3,2]
        VQ_DPP_MIN(0x4E)            // quad_perm [2,3,0,1]
        VQ_DPP_MIN(0x141)           // row_half_mirror
        VQ_DPP_MIN(0x140)           // row_mirror
        if (active && (lane & 15) == 0) { sm.cd[wave][4 * (lane >> 4) + r] = bd[r]; sm.cj[wave][4 * (lane >> 4) + r] = bj[r]; }
    }
#undef VQ_DPP_MIN
    __syncthreads();
    if (tid < 16) {
        float d = sm.cd[0][tid];
        int j = sm.cj[0][tid];
        for (int w = 1; w < nwv; ++w)
            if (sm.cd[w][tid] < d) { d = sm.cd[w][tid]; j = sm.cj[w][tid]; }
        sm.best[tid] = j;
        if (r0 + tid < N) idx[r0 + tid] = j;
    }
    __syncthreads();
    if (tid < 256) {
        const int row = tid >> 4, c4 = tid & 15;                       // F.embedding gather (model.py:113)
        if (r0 + row < N) ((float4 *)zq)[(size_t)(r0 + row) * 16 + c4] = ((const float4 *)E)[(size_t)sm.best[row] * 16 + c4];
    }
}

__global__ __launch_bounds__(256) void vq_encode_kernel(const float *__restrict__ X, int N, const float4 *__restrict__ Ef,
                                                        const float *__restrict__ E, const float *__restrict__ e2, int n_emb,
                                                        int64_t *__restrict__ idx, float *__restrict__ zq) {
    __shared__ VqSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r0 = blockIdx.x * 16;
    {
        const int row = tid >> 4, c4 = tid & 15;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + row < N) v = ((const float4 *)X)[(size_t)(r0 + row) * 16 + c4];
        sm.xs[row][4 * c4 + 0] = v.x; sm.xs[row][4 * c4 + 1] = v.y; sm.xs[row][4 * c4 + 2] = v.z; sm.xs[row][4 * c4 + 3] = v.w;
    }
    if (tid < 16) sm.x2s[tid] = r0 + tid < N ? sumsq64(X + (size_t)(r0 + tid) * 64) : 0.f;
    float4 f0[4], f1[4];
    vq_first_tiles(Ef, n_emb, 4, wave, lane, f0, f1);
    __syncthreads();
    vq_rows16(sm, r0, N, Ef, E, e2, n_emb, idx, zq, tid, f0, f1);
}

// encoder.14's tail for a 512-thread workgroup whose wave ct + 4 kh holds chain kh (k < 256, k >= 256) of column tile ct in zt:
// the reference's fold is (bias + c0) + c1, so c1 is handed over through the LDS scratch `part` (element [ct][row][col] at
// ct * TS + row * RS + col), the kh = 0 waves write z to sm.xs (and z_pre), and the VQ search runs on all of it (model.py:103-115).
// stop_at_z: z_pre is all the caller wants.
template <int TS, int RS>
__device__ __forceinline__ void rows16_finish_z(const FusedP &p, VqSmem &sm, float *part, const f32x4 &zt, int ct, int kh, int r0,
                                                int tid, const float4 (&f0)[4], const float4 (&f1)[4], int nwv, bool stop_at_z) {
    const int lane = tid & 63;
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[ct * TS + (4 * (lane >> 4) + r) * RS + (lane & 15)] = zt[r];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 4 * (lane >> 4) + r, col = 16 * ct + (lane & 15);
            const float z = zt[r] + part[ct * TS + row * RS + (lane & 15)];
            sm.xs[row][col] = z;
            if (p.z_pre && r0 + row < p.N) p.z_pre[(size_t)(r0 + row) * 64 + col] = z;
        }
    }
    __syncthreads();
    if (stop_at_z) return;
    if (tid < 16) sm.x2s[tid] = r0 + tid < p.N ? sumsq64(&sm.xs[tid][0]) : 0.f;
    __syncthreads();
    vq_rows16(sm, r0, p.N, p.Ef, p.E, p.e2, p.n_emb, p.idx, p.z_q, tid, f0, f1, nwv);
}

// ------------------------------------------------------------------------------------------
// Fused front end: conv -> LN/ReLU -> 4 x (FC -> LN/ReLU) -> FC 512->64 -> VQ in ONE launch, 16 rows per workgroup.
//
// The layered path above moves every activation through HBM ten times and spends 22 % of a C2 call in stand-alone
// LayerNorm passes (DESIGN "Encoder").  Here a 256-thread workgroup owns 16 whole rows: the activation tile
// (16 x 512 fp32) lives in LDS from the im2col gather to the VQ search, LayerNorm runs on it in place (the same
// half-wave-per-row Welford cascade as ln512_kernel, so the same bits), and each wave multiplies it with 128 output
// columns at a time on v_mfma_f32_16x16x4_f32: weights are pre-arranged in fragment order
//   Wf[(ct * K/16 + q) * 64 + lane] (float4) = W[16 ct + (lane & 15)][16 q + 4 c + (lane >> 4)], c = .x .y .z .w
// and go from L2 straight to registers (16 B per lane per 4 MFMAs, requested 3 q-steps ahead); one MFMA covers 4
// consecutive k, one accumulator per 16 x 16 tile, so a dot product is the same k-ascending fmaf chain -- restarted at
// the reference's K-block boundaries -- that gemm_chain_kernel runs on 32x32x2 tiles.  Same bits, one launch, no
// activation traffic; per workgroup the stream is all 5 MB of weights (L2-resident: every workgroup reads the same).
// ------------------------------------------------------------------------------------------
#define FE_LD 514                       // LDS row stride of the activation tile: bank = 2 row + k, conflict-free A reads
#define FE_WIN_C 128                    // channels of the staged mel window (the fused schedule runs for 4 C <= 512)

__global__ void frag16_build_kernel(const float *__restrict__ W, int N, int K, float4 *__restrict__ Wf) {
    const int nq = K / 16;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)(N / 16) * nq * 64) return;
    const int lane = (int)(id & 63);
    const int q = (int)((id >> 6) % nq), ct = (int)((id >> 6) / nq);
    const float *r = W + (size_t)(16 * ct + (lane & 15)) * K + 16 * q + (lane >> 4);
    Wf[id] = make_float4(r[0], r[4], r[8], r[12]);
}

// One GEMM stage for this wave: tile (LDS, 16 rows x K) x NT column tiles starting at ct0.  tot = fold over K blocks of
// kcq q-steps (16 k each) of zero-started chains: first block (bias ? bias + chain : chain), later blocks tot + chain.
// The first D-1 q-steps' fragments of a stage, requested ahead of time (under the previous stage's epilogue and
// LayerNorm, when the MFMA pipe would otherwise wait for the first bytes of the next weight matrix).
// D = depth of the fragment ring (a power of two): fragments are requested D-1 q-steps (of 0.43 us of MFMAs at NT = 8)
// before their MFMAs.  The weight stream is latency x bytes-in-flight bound: with D = 4 a wave has 24 KB in flight and
// a workgroup pulls 44 GB/s -- alone on the chip as well as among 255 others -- against the 75 GB/s its MFMAs consume.
// q_off / nq_all: the stage covers q-steps [q_off, q_off + nq) of a fragment array holding nq_all per column tile (0: nq).
template <int NT, int D>
__device__ __forceinline__ void rows16_prefetch(const float4 *__restrict__ Wf, int ct0, int nq, float4 (&fr)[D][NT], int lane,
                                                int q_off = 0, int nq_all = 0) {
    const int qs = nq_all ? nq_all : nq;
#pragma unroll
    for (int u = 0; u < D - 1; ++u)
#pragma unroll
        for (int j = 0; j < NT; ++j) fr[u][j] = Wf[(((size_t)(ct0 + j) * qs) + q_off + (u < nq ? u : nq - 1)) * 64 + lane];
}

template <int NT, int D>
__device__ __forceinline__ void rows16_gemm(const float *tile, const float4 *__restrict__ Wf, int ct0, int nq, int kcq,
                                            const float *__restrict__ bias, f32x4 (&tot)[NT], int lane, float4 (&fr)[D][NT],
                                            int q_off = 0, int nq_all = 0) {
    const float4 *wp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) wp[j] = Wf + ((size_t)(ct0 + j) * (nq_all ? nq_all : nq) + q_off) * 64 + lane;
    const float *arow = tile + (lane & 15) * FE_LD + (lane >> 4) + 16 * q_off;
    float an[4] = {arow[0], arow[4], arow[8], arow[12]};
    f32x4 acc[NT];
    float bv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        tot[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        bv[j] = bias ? bias[16 * (ct0 + j) + (lane & 15)] : 0.f;
    }
    bool first = true;
    for (int q0 = 0; q0 < nq; q0 += D) {                             // nq is a multiple of 4; D = 8 walks it in halves
#pragma unroll
        for (int u = 0; u < D; ++u) {
            const int q = q0 + u;
            if (D > 4 && q >= nq) break;                             // wave-uniform
            const int qp = q + D - 1 < nq ? q + D - 1 : nq - 1;
#pragma unroll
            for (int j = 0; j < NT; ++j) fr[(u + D - 1) & (D - 1)][j] = wp[j][(size_t)qp * 64];
            const float a0 = an[0], a1 = an[1], a2 = an[2], a3 = an[3];
            const int qn = q + 1 < nq ? q + 1 : q;
            an[0] = arow[16 * qn]; an[1] = arow[16 * qn + 4]; an[2] = arow[16 * qn + 8]; an[3] = arow[16 * qn + 12];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, fr[u][j].x, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, fr[u][j].y, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, fr[u][j].z, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, fr[u][j].w, acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if ((u & 3) == 3 && (q + 1) % kcq == 0) {                // end of a K block (kcq is a multiple of 4)
#pragma unroll
                for (int j = 0; j < NT; ++j) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        tot[j][r] = first ? (bias ? bv[j] + acc[j][r] : acc[j][r]) : tot[j][r] + acc[j][r];
                        acc[j][r] = 0.f;
                    }
                }
                first = false;
            }
        }
    }
}

// D layout of the 16x16x4 MFMA: register r of a lane = row 4 (lane >> 4) + r, column lane & 15.
template <int NT>
__device__ __forceinline__ void rows16_store(float *tile, const f32x4 (&tot)[NT], int ct0, int lane) {
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(4 * (lane >> 4) + r) * FE_LD + 16 * (ct0 + j) + (lane & 15)] = tot[j][r];
}

// LayerNorm(512) + ReLU of the tile in place, a half-wave per row as ln512_kernel (512 threads: 16 half-waves, 16 rows).
__device__ __forceinline__ void rows16_layernorm(float *tile, const float *__restrict__ g, const float *__restrict__ b,
                                                 float eps, const LnConst &k, int tid) {
    const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, ll = lane & 31;
    float *x = tile + (wave * 2 + half) * FE_LD;
    const float2 mr = ln512_moments(x, k, eps);
    const float mean = mr.x, rstd = mr.y;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int e = q * 64 + ll * 2;                                  // 8-byte LDS accesses (the row stride is 8 mod 16)
        const float2 gv = *(const float2 *)(g + e);
        const float2 bb = *(const float2 *)(b + e);
        const float2 xv = *(const float2 *)(x + e);
        float2 o;
        o.x = __builtin_fmaf((xv.x - mean) * rstd, gv.x, bb.x);
        o.y = __builtin_fmaf((xv.y - mean) * rstd, gv.y, bb.y);
        o.x = o.x < 0.f ? 0.f : o.x;
        o.y = o.y < 0.f ? 0.f : o.y;
        *(float2 *)(x + e) = o;
    }
}

__device__ __forceinline__ bool rows16_dump(const FusedP &p, const float *tile, int stage, int r0, int tid) {
    if (p.stage != stage) return false;
    for (int e = tid; e < 16 * 512; e += (int)blockDim.x) {
        const int row = e >> 9, col = e & 511;
        if (r0 + row < p.N) p.stage_out[(size_t)(r0 + row) * 512 + col] = tile[row * FE_LD + col];
    }
    return true;
}

// 512 threads: eight waves of four column tiles, TWO per SIMD.  With one wave per SIMD (256 threads x eight tiles) the MFMA
// pipe idles while that wave requests the next fragments, reads its A operands and folds K blocks -- each Linear took 18.5 us
// for 13.7 us of MFMAs (tools/encoder_stage_times.py); a second wave fills those gaps, and LayerNorm has a half-wave per row.
__global__ __launch_bounds__(512) void enc_fused_kernel(FusedP p) {
    __shared__ __attribute__((aligned(16))) float tile[16 * FE_LD];
    __shared__ VqSmem sm;
    __shared__ float mel_win[FE_WIN_C * 36];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r0 = blockIdx.x * 16;
    const int K0 = 4 * p.C;
    constexpr int NT = 4, RD = 4;                        // column tiles per wave; fragment ring: 3 q-steps ahead (a ring of 8 --
    f32x4 tot[NT];                                       // 7 ahead -- measured the same: the stream is not what the MFMAs wait for)
    float4 fr[RD][NT];
    rows16_prefetch<NT, RD>(p.conv_f, NT * wave, K0 / 16, fr, lane);      // the first conv fragments fly under the gather

    // ---- im2col of the 16 rows (model.py:65), k order of the reference back end (im2col_ct).  When the 16 rows are consecutive
    // frames of ONE utterance (always at configs[1]: 64 frames per utterance) their taps are a window of 34 mel frames per
    // channel: it is loaded ONCE, coalesced along T (136 contiguous bytes per channel instead of 16 x 4 scalar loads 8 bytes
    // apart), into LDS and the tile is built from there.  A tile that straddles two utterances (or the end) gathers from global.
    const int b0 = r0 / p.To, tt0 = r0 - b0 * p.To;
    const bool one_utt = r0 + 15 < p.N && tt0 + 15 < p.To && p.C <= FE_WIN_C;
    if (one_utt) {
        float *win = mel_win;                                 // [C][36]: frames 2 tt0 - 1 ... 2 tt0 + 32 (zero outside the utterance)
        const float *src = p.mel + (size_t)b0 * p.C * p.T;
        const int ti0 = 2 * tt0 - 1;
        for (int e = tid; e < p.C * 36; e += 512) {
            const int c = e / 36, o = e - c * 36, ti = ti0 + o;
            win[e] = (o < 34 && ti >= 0 && ti < p.T) ? src[(size_t)c * p.T + ti] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < 16 * K0; e += 512) {
            const int i = e & 15, kidx = e >> 4;
            int c, tap;
            im2col_ct(p.conv_mode, kidx, c, tap);
            tile[i * FE_LD + kidx] = win[c * 36 + 2 * i + tap];
        }
    } else {
        for (int e = tid; e < 16 * K0; e += 512) {
            const int i = e & 15, kidx = e >> 4;
            tile[i * FE_LD + kidx] = im2col_at(p.mel, p.C, p.T, p.To, p.N, r0 + i, kidx, p.conv_mode);
        }
    }
    __syncthreads();

    rows16_gemm<NT, RD>(tile, p.conv_f, NT * wave, K0 / 16, p.conv_mode == 1 ? K0 / 16 : 4, nullptr, tot, lane, fr);
    if (p.stage != 0) rows16_prefetch<NT, RD>(p.fc_f[0], NT * wave, 32, fr, lane);    // under the store + LayerNorm below
    __syncthreads();                                     // every wave has read its A operands
    rows16_store<NT>(tile, tot, NT * wave, lane);
    __syncthreads();
    if (rows16_dump(p, tile, 0, r0, tid)) return;

    // ---- seg-FC stack (model.py:46-55)
    rows16_layernorm(tile, p.ln_g[0], p.ln_b[0], p.eps, p.lnc, tid);
    __syncthreads();
    if (rows16_dump(p, tile, 1, r0, tid)) return;
    for (int l = 0; l < 4; ++l) {
        rows16_gemm<NT, RD>(tile, p.fc_f[l], NT * wave, 32, 16, nullptr, tot, lane, fr);
        if (l < 3) rows16_prefetch<NT, RD>(p.fc_f[l + 1], NT * wave, 32, fr, lane);
        __syncthreads();
        rows16_store<NT>(tile, tot, NT * wave, lane);
        __syncthreads();
        if (rows16_dump(p, tile, 2 + 2 * l, r0, tid)) return;
        rows16_layernorm(tile, p.ln_g[l + 1], p.ln_b[l + 1], p.eps, p.lnc, tid);
        __syncthreads();
        if (rows16_dump(p, tile, 3 + 2 * l, r0, tid)) return;
    }

    // ---- encoder.14: 512 -> 64 with bias: four 16-column tiles.  The reference's fold (bias + c0) + c1 has two independent
    // zero-started chains (k < 256, k >= 256): wave w runs c0 of tile w, wave w + 4 runs c1 -- half the dependent MFMA chain
    // each -- and hands it over through LDS.  The VQ codebook tiles stream in underneath.
    const int ctw = wave & 3, kh = wave >> 2;
    const int nwv = vq_search_waves(p.n_emb);
    float4 f0[4], f1[4];
    vq_first_tiles(p.Ef, p.n_emb, nwv, wave, lane, f0, f1);
    f32x4 zt[1];
    float4 fr1[4][1];
    rows16_prefetch<1, 4>(p.out_f, ctw, 16, fr1, lane, 16 * kh, 32);
    rows16_gemm<1, 4>(tile, p.out_f, ctw, 16, 16, kh == 0 ? p.out_b : nullptr, zt, lane, fr1, 16 * kh, 32);
    __syncthreads();                                     // the activation tile is dead once every wave is past its chain:
    rows16_finish_z<16, 68>(p, sm, tile, zt[0], ctw, kh, r0, tid, f0, f1, nwv, p.stage == 10);   // c1 goes through it as [16][68]
}

// ------------------------------------------------------------------------------------------
// Small calls (a single utterance: BASELINE configs[0], encode.py:44-46): too few 16-row tiles to fill the chip with
// whole-row workgroups, and each of those would still stream all 5 MB of weights.  Here the columns are split over
// several workgroups per row tile and one launch covers one Linear:
//   launch 0: im2col + conv (8 column groups: 4 waves x one 16-column tile)                     -> raw rows
//   launch l = 1..4: LayerNorm_{l-1} + ReLU of the raw rows ON LOAD (every column workgroup repeats it for its 16 rows:
//                    16 x 512 elements, nothing next to the launch boundary it saves) + Linear_l, 16 column groups of
//                    2 column tiles x the 2 K halves of the chain fold                          -> raw rows
//   launch 5: LayerNorm_4 + ReLU on load + encoder.14 + VQ search (one workgroup per row tile, as the fused tail)
// Six launches instead of fourteen, same chains, same bits.  The K blocks of a chain fold are independent
// zero-started chains, so a wave runs them interleaved (NBLK accumulators) instead of one dependent MFMA sequence.
// ------------------------------------------------------------------------------------------
// A wave's whole weight slice (one 16-column tile, NQ q-steps) is requested up front -- 4 NQ registers -- so that the
// loads fly under the A-tile load and the LayerNorm, and the MFMAs then run back to back (a 1-deep prefetch left every
// step waiting ~0.3 us on L2: 10.4 us per launch, rocprofv3).
template <int NQ>
__device__ __forceinline__ void rows16_load_w(const float4 *__restrict__ Wf, int ct, int lane, float4 (&wf)[NQ]) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) wf[q] = Wf[((size_t)ct * NQ + q) * 64 + lane];
}
template <int NBLK, int KCQ>
__device__ __forceinline__ f32x4 rows16_gemm_pre(const float *tile, const float4 (&wf)[NBLK * KCQ], int ct,
                                                 const float *__restrict__ bias, int lane) {
    const float *arow = tile + (lane & 15) * FE_LD + (lane >> 4);
    f32x4 acc[NBLK];
#pragma unroll
    for (int b = 0; b < NBLK; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KCQ; ++s) {
        float a[NBLK][4];
#pragma unroll
        for (int b = 0; b < NBLK; ++b)
#pragma unroll
            for (int c = 0; c < 4; ++c) a[b][c] = arow[16 * (b * KCQ + s) + 4 * c];
#pragma unroll
        for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b][0], wf[b * KCQ + s].x, acc[b], 0, 0, 0);
#pragma unroll
        for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b][1], wf[b * KCQ + s].y, acc[b], 0, 0, 0);
#pragma unroll
        for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b][2], wf[b * KCQ + s].z, acc[b], 0, 0, 0);
#pragma unroll
        for (int b = 0; b < NBLK; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[b][3], wf[b * KCQ + s].w, acc[b], 0, 0, 0);
    }
    const float bv = bias ? bias[16 * ct + (lane & 15)] : 0.f;
    f32x4 tot;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        tot[r] = bias ? bv + acc[0][r] : acc[0][r];
#pragma unroll
        for (int b = 1; b < NBLK; ++b) tot[r] = tot[r] + acc[b][r];
    }
    return tot;
}

// Prologue of a 512-thread launch that takes raw rows: rows r0 .. r0 + 15 of `in` (N x 512, zero past N) into the LDS tile, then
// LayerNorm + ReLU in place.  vmcnt retires in order, so the rows' loads are issued FIRST and `issue_weights` -- the caller's
// loads of its weight slice -- behind them: waiting for the rows then leaves the weights in flight under the LayerNorm.
template <class F>
__device__ __forceinline__ void rows16_load_ln(const float *__restrict__ in, int r0, int N, float *tile, const float *__restrict__ g,
                                               const float *__restrict__ b, float eps, const LnConst &k, int tid, F issue_weights) {
    float4 av[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = tid + 512 * n, row = e >> 7, c4 = e & 127;
        av[n] = r0 + row < N ? ((const float4 *)in)[(size_t)(r0 + row) * 128 + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    issue_weights();
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int e = tid + 512 * n, row = e >> 7, c4 = e & 127;
        float *d = tile + row * FE_LD + 4 * c4;
        *(float2 *)d = make_float2(av[n].x, av[n].y);
        *(float2 *)(d + 2) = make_float2(av[n].z, av[n].w);
    }
    __syncthreads();
    rows16_layernorm(tile, g, b, eps, k, tid);
    __syncthreads();
}

// The three layer kinds of the split schedule for column group `cg` of the row tile at r0 (bodies of the enc_split_*_kernel launches):
// conv (layer 0), Linear l = 1..4 (LayerNorm l-1 on load); encoder.14 + VQ (LayerNorm 4 on load) has a launch shape of its own.
__device__ __forceinline__ void split_conv(const FusedP &p, float *__restrict__ out, int cg, int r0, float *tile) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K0 = 4 * p.C;
    const int ct = 4 * cg + wave, nq = K0 / 16;
    // vmcnt retires in order: the gather's loads go FIRST, the weight slice behind them, so that waiting for the
    // gather leaves the weights in flight
    float gv[20];
#pragma unroll
    for (int n = 0; n < 20; ++n) {
        const int e = tid + 256 * n;
        gv[n] = e < 16 * K0 ? im2col_at(p.mel, p.C, p.T, p.To, p.N, r0 + (e & 15), e >> 4, p.conv_mode) : 0.f;
    }
    float4 wc[20];
    if (nq == 20) rows16_load_w<20>(p.conv_f, ct, lane, wc);          // C = 80 (the reference): whole slice up front
#pragma unroll
    for (int n = 0; n < 20; ++n) {
        const int e = tid + 256 * n;
        if (e < 16 * K0) tile[(e & 15) * FE_LD + (e >> 4)] = gv[n];
    }
    for (int e = tid + 256 * 20; e < 16 * K0; e += 256) {             // more than 80 channels: the rest, plainly
        tile[(e & 15) * FE_LD + (e >> 4)] = im2col_at(p.mel, p.C, p.T, p.To, p.N, r0 + (e & 15), e >> 4, p.conv_mode);
    }
    __syncthreads();
    f32x4 tot;
    if (nq == 20 && p.conv_mode == 1) tot = rows16_gemm_pre<1, 20>(tile, wc, ct, nullptr, lane);
    else if (nq == 20) tot = rows16_gemm_pre<5, 4>(tile, wc, ct, nullptr, lane);
    else {                                                            // other channel counts: the generic fold
        f32x4 t1[1];
        float4 fr1[4][1];
        rows16_prefetch<1, 4>(p.conv_f, ct, nq, fr1, lane);
        rows16_gemm<1, 4>(tile, p.conv_f, ct, nq, p.conv_mode == 1 ? nq : 4, nullptr, t1, lane, fr1);
        tot = t1[0];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = r0 + 4 * (lane >> 4) + r;
        if (m < p.N) out[(size_t)m * 512 + 16 * ct + (lane & 15)] = tot[r];
    }
}

// 512 threads: 8 column groups per row tile; a workgroup = 4 column tiles x the 2 K halves of the chain fold (they are
// independent zero-started chains: tot = c0 + c1), so a wave streams 16 KB of weights and issues 64 MFMAs; every column
// workgroup repeats the LayerNorm of its row tile, a half-wave per row.
__device__ __forceinline__ void split_fc(const FusedP &p, int layer, const float *__restrict__ in, float *__restrict__ out, int cg,
                                         int r0, float *tile, float (*part)[16][17]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cl = wave & 3, ct = 4 * cg + cl, kh = wave >> 2;
    float4 wh[16];
    rows16_load_ln(in, r0, p.N, tile, p.ln_g[layer - 1], p.ln_b[layer - 1], p.eps, p.lnc, tid,
                   [&] { rows16_load_w<16>(p.fc_f[layer - 1], 2 * ct + kh, lane, wh); });
    const f32x4 acc = rows16_gemm_pre<1, 16>(tile + 256 * kh, wh, ct, nullptr, lane);      // k in [256 kh, 256 kh + 256)
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) part[cl][4 * (lane >> 4) + r][lane & 15] = acc[r];
    }
    __syncthreads();
    if (kh == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = r0 + 4 * (lane >> 4) + r;
            if (m < p.N) out[(size_t)m * 512 + 16 * ct + (lane & 15)] = acc[r] + part[cl][4 * (lane >> 4) + r][lane & 15];
        }
    }
}

// The last launch, one 512-thread workgroup per row tile: LayerNorm 4 + ReLU on load (a half-wave per row), encoder.14 with
// its two K-block chains on wave pairs (as the fused launch's tail), VQ search on 8 waves.
__global__ __launch_bounds__(512) void enc_split_tail_kernel(FusedP p, const float *__restrict__ in) {
    __shared__ __attribute__((aligned(16))) float tile[16 * FE_LD];
    __shared__ VqSmem sm;
    __shared__ float part[4][16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r0 = blockIdx.y * 16;
    const int ct = wave & 3, kh = wave >> 2;
    float4 wh[16];
    rows16_load_ln(in, r0, p.N, tile, p.ln_g[4], p.ln_b[4], p.eps, p.lnc, tid,
                   [&] { rows16_load_w<16>(p.out_f, 2 * ct + kh, lane, wh); });
    const int nwv = vq_search_waves(p.n_emb);
    float4 f0[4], f1[4];
    vq_first_tiles(p.Ef, p.n_emb, nwv, wave, lane, f0, f1);
    // (bias + c0) + c1: wave w < 4 runs c0 of column tile w, wave w + 4 runs c1
    const f32x4 zt = rows16_gemm_pre<1, 16>(tile + 256 * kh, wh, ct, kh == 0 ? p.out_b : nullptr, lane);
    rows16_finish_z<16 * 17, 17>(p, sm, &part[0][0][0], zt, ct, kh, r0, tid, f0, f1, nwv, false);
}

__global__ __launch_bounds__(256) void enc_split_conv_kernel(FusedP p, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[16 * FE_LD];
    split_conv(p, out, blockIdx.x, blockIdx.y * 16, tile);
}
__global__ __launch_bounds__(512) void enc_split_fc_kernel(FusedP p, int layer, const float *__restrict__ in, float *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) float tile[16 * FE_LD];
    __shared__ float part[4][16][17];
    split_fc(p, layer, in, out, blockIdx.x, blockIdx.y * 16, tile, part);
}

// (A resident one-launch form of this schedule -- the 16 column workgroups of a row tile on one XCD, handing the rows over
// in-kernel through that XCD's L2 -- was built and measured slower, 62 vs 50.5 us: profiles/r02_encoder_resident_timeline.txt.)

// Eval-branch statistics of VQEmbeddingEMA.forward (model.py:147-153): deterministic two-level
// reductions (per-block partials, then one block in fixed order).
__global__ __launch_bounds__(256) void vq_stats_partial_kernel(const float *__restrict__ x, const float *__restrict__ q,
                                                               const int64_t *__restrict__ idx, int n_rows,
                                                               float *__restrict__ zst, double *__restrict__ part_se,
                                                               unsigned *__restrict__ hist) {
    __shared__ double red[256];
    const size_t n = (size_t)n_rows * 64;
    double se = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float xv = x[i], qv = q[i];
        const float d = xv - qv;
        se += (double)d * (double)d;
        if (zst) zst[i] = xv + (qv - xv);
    }
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n_rows; r += gridDim.x * 256) atomicAdd(&hist[idx[r]], 1u);
    red[threadIdx.x] = se;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) part_se[blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void vq_stats_final_kernel(const double *__restrict__ part_se, int nparts,
                                                             const unsigned *__restrict__ hist, int n_emb, int n_rows,
                                                             float *__restrict__ loss, float *__restrict__ ppl) {
    __shared__ double red[256];
    double ent = 0.0;
    for (int j = threadIdx.x; j < n_emb; j += 256) {
        const float p = (float)((double)hist[j] / (double)n_rows);
        ent += (double)(p * logf(p + 1e-10f));
    }
    red[threadIdx.x] = ent;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double se = 0.0;
        for (int i = 0; i < nparts; ++i) se += part_se[i];
        *loss = (float)(0.25 * se / ((double)n_rows * 64.0));
        *ppl = expf((float)-red[0]);
    }
}

// conv.weight (O, C, 4) -> GEMM operand (O, 4C) in the k order of each reference back-end.
__global__ void conv_weight_permute_kernel(const float *__restrict__ w, float *__restrict__ w1,
                                           float *__restrict__ w2, int O, int C) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int K = 4 * C;
    if (i >= O * K) return;
    const int o = i / K, kidx = i - o * K;
    w1[i] = w[i];                                          // mode 1: kidx = c*4 + tap (native layout)
    int c, tap;
    im2col_ct(2, kidx, c, tap);
    w2[i] = w[((size_t)o * C + c) * 4 + tap];              // mode 2: [block of 16 c][tap][c in block]
}

// ------------------------------------------------------------------------------------------
// launches (encoder_internal.h)
// ------------------------------------------------------------------------------------------
void launch_ln512(const float *X, const float *g, const float *b, float *Y, int M, float eps, int relu, const LnConst &k, hipStream_t s,
                  float *stat) {
    hipLaunchKernelGGL(ln512_kernel, dim3((M + 7) / 8), dim3(256), 0, s, X, g, b, Y, M, eps, relu, k, stat);
}
void launch_vq_encode(const float *X, int N, const float4 *Ef, const float *E, const float *e2, int n_emb, int64_t *idx, float *zq, hipStream_t s) {
    hipLaunchKernelGGL(vq_encode_kernel, dim3((N + 15) / 16), dim3(256), 0, s, X, N, Ef, E, e2, n_emb, idx, zq);
}
void launch_enc_fused(const FusedP &p, hipStream_t s) {
    hipLaunchKernelGGL(enc_fused_kernel, dim3((p.N + 15) / 16), dim3(512), 0, s, p);
}
void launch_enc_split(const FusedP &p, float *a, float *b, hipStream_t s) {
    const int ntiles = (p.N + 15) / 16;
    hipLaunchKernelGGL(enc_split_conv_kernel, dim3(8, ntiles), dim3(256), 0, s, p, a);
    for (int l = 1; l <= 4; ++l) {
        hipLaunchKernelGGL(enc_split_fc_kernel, dim3(8, ntiles), dim3(512), 0, s, p, l, (const float *)a, b);
        float *t = a; a = b; b = t;
    }
    hipLaunchKernelGGL(enc_split_tail_kernel, dim3(1, ntiles), dim3(512), 0, s, p, (const float *)a);
}
void launch_vq_stats(const float *x, const float *q, const int64_t *idx, int n_rows, float *zst, double *part, int nparts, unsigned *hist,
                     int n_emb, float *loss, float *ppl, hipStream_t s) {
    hipLaunchKernelGGL(vq_stats_partial_kernel, dim3(nparts), dim3(256), 0, s, x, q, idx, n_rows, zst, part, hist);
    hipLaunchKernelGGL(vq_stats_final_kernel, dim3(1), dim3(256), 0, s, part, nparts, hist, n_emb, n_rows, loss, ppl);
}
void launch_conv_weight_permute(const float *w, float *w1, float *w2, int O, int C, hipStream_t s) {
    hipLaunchKernelGGL(conv_weight_permute_kernel, dim3((unsigned)(((size_t)O * C * 4 + 255) / 256)), dim3(256), 0, s, w, w1, w2, O, C);
}
void launch_rowsumsq64(const float *X, float *out, int n, hipStream_t s) {
    hipLaunchKernelGGL(rowsumsq64_kernel, dim3((n + 63) / 64), dim3(64), 0, s, X, out, n);
}
void launch_vq_build_frag(const float *E, float4 *Ef, int n_emb, hipStream_t s) {
    hipLaunchKernelGGL(vq_build_frag_kernel, dim3((n_emb * 16 + 255) / 256), dim3(256), 0, s, E, Ef, n_emb);
}
void launch_frag16_build(const float *W, int N, int K, float4 *Wf) {
    const size_t n4 = (size_t)(N / 16) * (K / 16) * 64;
    hipLaunchKernelGGL(frag16_build_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, 0, W, N, K, Wf);
}
