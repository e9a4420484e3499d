// Vocoder scoring head (K9): after a chunk of the teacher-forced scan has left h_t of every step in `hall`, ONE kernel
// finishes the chunk -- fc1 + ReLU, fc2, log-sum-exp, target gather, first-argmax -- without writing the fc1 outputs or the
// energies to memory.  What leaves the kernel is one fp32 nll per scored sample (optional) and one {sum, scored, correct}
// record per (utterance, workgroup); tf_nll_finish_kernel adds the records of a chunk to the call's per-utterance totals in
// a fixed order.  No atomics touch a sum: equal inputs give equal bits.
//
// Tile.  A 256-thread workgroup owns 64 consecutive steps of ONE utterance (grid = (ceil(CH / 64), B)), so every record
// belongs to one utterance.  Both GEMMs run on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 out): wave w owns output columns
// [64 w, 64 w + 64) of all 64 rows = 4 x 4 tiles of 16 x 16 = 64 accumulator registers.  The weights are the plain
// (rows, K) copies of the handle: a lane reads 16 bytes of a row (4 consecutive k) per 16-k step, straight from L2 into
// registers, NLL_D - 1 steps ahead; the h rows travel the same way (fc1) or come out of LDS (fc2: the ReLU'd fc1 tile,
// 64 x 256 fp32, row stride 260 floats: bank = 4 row + k, conflict-free 16-byte reads).  MFMA s of a 16-k step multiplies
// the columns k = 16 q + 4 g + s (g = lane >> 4): each dot product is one zero-started fp32 fma chain over a fixed
// permutation of k, then bias + chain -- the same number of roundings as the chunk GEMMs of Vocoder.forward, in another order.
#include "common.h"
#include "ar_shared.h"
#include "nll.h"

#define NLL_ROWS 64
#define NLL_LD 260                      // LDS row stride of the fc1 tile (floats)
#define NLL_D 4                         // depth of the operand ring: operands are requested NLL_D - 1 steps ahead

struct NllLds {
    float a[NLL_ROWS * NLL_LD];         // relu(W1 h + b1)
    float wm[4][NLL_ROWS];              // per wave: row maximum over its 64 classes, its first class,
    int wi[4][NLL_ROWS];
    float ws[4][NLL_ROWS];              // and sum of exp(e - m)
    float et[NLL_ROWS];                 // the target's energy
    float out[NLL_ROWS];                // nll per row (0 for a row that is not scored)
    int tgt[NLL_ROWS];                  // target class, -1 = the row is not scored
    int ok[NLL_ROWS];                   // the target was the first maximum
};

// One GEMM stage of a wave: 64 rows x 64 columns x K.  A: 4 row-tile pointers (this lane's row, + 4 g), global or LDS;
// W: 4 column-tile pointers (this lane's weight row, + 4 g).  nq = K / 16, a multiple of NLL_D.
__device__ __forceinline__ void nll_gemm(const float *const (&ap)[4], const float *const (&wp)[4], int nq, f32x4 (&acc)[4][4]) {
    f32x4 fa[NLL_D][4], fw[NLL_D][4];             // native vectors: one 16-byte load each (a float4 struct is split per field)
#pragma unroll
    for (int u = 0; u < NLL_D - 1; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            fa[u][j] = *(const f32x4 *)(ap[j] + 16 * u);
            fw[u][j] = *(const f32x4 *)(wp[j] + 16 * u);
        }
    for (int q0 = 0; q0 < nq; q0 += NLL_D) {
#pragma unroll
        for (int u = 0; u < NLL_D; ++u) {
            const int q = q0 + u;
            const int qp = q + NLL_D - 1 < nq ? q + NLL_D - 1 : nq - 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                fa[(u + NLL_D - 1) & (NLL_D - 1)][j] = *(const f32x4 *)(ap[j] + 16 * qp);
                fw[(u + NLL_D - 1) & (NLL_D - 1)][j] = *(const f32x4 *)(wp[j] + 16 * qp);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][i][0], fw[u][j][0], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][i][1], fw[u][j][1], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][i][2], fw[u][j][2], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[u][i][3], fw[u][j][3], acc[i][j], 0, 0, 0);
        }
    }
}

__global__ __launch_bounds__(256, 2) void tf_nll_kernel(NllHead p) {
    extern __shared__ __align__(16) unsigned char nll_lds_raw[];
    NllLds &S = *(NllLds *)nll_lds_raw;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
    const int b = blockIdx.y, tt0 = blockIdx.x * NLL_ROWS, tiles = gridDim.x;
    const int slen = p.slen[b];                                   // scored steps of this utterance
    NllPart *part = p.part + (size_t)b * tiles + blockIdx.x;
    if (p.t0 + tt0 >= slen) {                                     // nothing of this tile is scored (workgroup-uniform)
        if (tid == 0) *part = NllPart{0.0, 0, 0};
        return;
    }
    // targets of the tile's rows; a class outside [0, n_cls) in a scored position (input or target) is reported, not read past
    if (tid < NLL_ROWS) {
        const int tt = tt0 + tid, t = p.t0 + tt;
        int tg = -1;
        if (tt < p.CH && t < slen) {
            const long long x = p.audio[(size_t)b * p.L + t], y = p.audio[(size_t)b * p.L + t + 1];
            if (x < 0 || x >= NLL_CLS || y < 0 || y >= NLL_CLS) {
                if (p.status) __hip_atomic_fetch_or(p.status, p.status_tag | STATUS_BAD_INDEX, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                tg = NLL_CLS;                                     // scored, matches no class
            } else tg = (int)y;
        }
        S.tgt[tid] = tg;
        S.et[tid] = 0.f;
    }

    f32x4 acc[4][4];
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // ---- fc1: a = relu(b1 + W1 h), K = Hr.  Rows past the chunk re-read its last row (masked below).
    {
        const float *ap[4], *wp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int tt = tt0 + 16 * i + c;
            tt = tt < p.CH ? tt : p.CH - 1;
            ap[i] = p.hall + ((size_t)b * p.CH + tt) * p.Hr + 4 * g;
            wp[i] = p.w1 + (size_t)(64 * wave + 16 * i + c) * p.Hr + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = zero;
        }
        nll_gemm(ap, wp, p.Hr / 16, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 64 * wave + 16 * j + c;
            const float bv = p.b1[col];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = bv + acc[i][j][r];
                    S.a[(16 * i + 4 * g + r) * NLL_LD + col] = v < 0.f ? 0.f : v;
                }
        }
    }
    __syncthreads();
    // ---- fc2: e = b2 + W2 a, K = 256, A from LDS
    {
        const float *ap[4], *wp[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ap[i] = S.a + (16 * i + c) * NLL_LD + 4 * g;
            wp[i] = p.w2 + (size_t)(64 * wave + 16 * i + c) * NLL_HF + 4 * g;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = zero;
        }
        nll_gemm(ap, wp, NLL_HF / 16, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float bv = p.b2[64 * wave + 16 * j + c];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = bv + acc[i][j][r];
        }
    }
    // ---- per row: maximum and its first class.  A lane holds classes 64 w + 16 j + c (j = 0..3) of row 16 i + 4 g + r; the 16
    // lanes of a group share the row (butterfly over c), the 4 waves combine through LDS in wave = class order.
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * i + 4 * g + r;
            float m = acc[i][0][r];
            int k = 64 * wave + c;
#pragma unroll
            for (int j = 1; j < 4; ++j) if (acc[i][j][r] > m) { m = acc[i][j][r]; k = 64 * wave + 16 * j + c; }
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const float om = __shfl_xor(m, d, 64);
                const int ok = __shfl_xor(k, d, 64);
                if (om > m || (om == m && ok < k)) { m = om; k = ok; }
            }
            if (c == 0) { S.wm[wave][row] = m; S.wi[wave][row] = k; }
            const int tg = S.tgt[row];
#pragma unroll
            for (int j = 0; j < 4; ++j) if (tg == 64 * wave + 16 * j + c) S.et[row] = acc[i][j][r];
        }
    __syncthreads();
    // ---- sum of exp(e - m) as a fixed tree: (x0 + x1) + (x2 + x3) in the lane, four butterfly levels over the 16 lanes of the
    // group, (s0 + s1) + (s2 + s3) over the waves: 8 roundings on every path
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * i + 4 * g + r;
            float m = S.wm[0][row];
#pragma unroll
            for (int w = 1; w < 4; ++w) m = S.wm[w][row] > m ? S.wm[w][row] : m;
            const float x0 = expf(acc[i][0][r] - m), x1 = expf(acc[i][1][r] - m);
            const float x2 = expf(acc[i][2][r] - m), x3 = expf(acc[i][3][r] - m);
            float s = (x0 + x1) + (x2 + x3);
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) s = s + __shfl_xor(s, d, 64);
            if (c == 0) S.ws[wave][row] = s;
        }
    __syncthreads();
    if (tid < NLL_ROWS) {
        const int row = tid, tg = S.tgt[row];
        float m = S.wm[0][row];
        int k = S.wi[0][row];
#pragma unroll
        for (int w = 1; w < 4; ++w) if (S.wm[w][row] > m) { m = S.wm[w][row]; k = S.wi[w][row]; }
        const float s = (S.ws[0][row] + S.ws[1][row]) + (S.ws[2][row] + S.ws[3][row]);
        const float lse = m + logf(s);
        const float v = lse - S.et[row];
        const bool scored = tg >= 0;
        S.out[row] = scored ? v : 0.f;
        S.ok[row] = scored && k == tg;
        if (scored && p.nll) p.nll[(size_t)b * (p.L - 1) + p.t0 + tt0 + row] = v;
    }
    __syncthreads();
    if (tid == 0) {                                               // the tile's record: double sum in step order
        double sum = 0.0;
        int n = 0, ok = 0;
        for (int row = 0; row < NLL_ROWS; ++row) {
            if (S.tgt[row] < 0) continue;
            sum += (double)S.out[row]; n += 1; ok += S.ok[row];
        }
        *part = NllPart{sum, n, ok};
    }
}

// Per utterance: the chunk's records in tile order onto the call's totals (chunks arrive in step order on one stream).
__global__ void tf_nll_finish_kernel(const NllPart *__restrict__ part, int B, int tiles, double *nll_sum, int64_t *n_scored,
                                     int64_t *n_correct) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double sum = nll_sum[b];
    long long n = n_scored[b], ok = n_correct[b];
    for (int j = 0; j < tiles; ++j) {
        const NllPart q = part[(size_t)b * tiles + j];
        sum += q.sum; n += q.n; ok += q.ok;
    }
    nll_sum[b] = sum; n_scored[b] = n; n_correct[b] = ok;
}

// tf_nll_kernel needs more than the default 64 KiB of dynamic LDS: set per device, once per handle (vqcpc_vocoder_create).
int vq_tf_nll_prepare() {
    HIP_TRY(hipFuncSetAttribute((const void *)tf_nll_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(NllLds)));
    return VQCPC_OK;
}

int vq_tf_nll_tiles(int CH) { return (CH + NLL_ROWS - 1) / NLL_ROWS; }

int vq_tf_nll_chunk(const NllHead &p, double *nll_sum, int64_t *n_scored, int64_t *n_correct, hipStream_t s) {
    VQ_REQUIRE(p.Hr % (16 * NLL_D) == 0 && p.CH > 0 && p.B > 0 && p.L >= 2, "vocoder.nll: unsupported shape Hr=%d CH=%d B=%d L=%d",
               p.Hr, p.CH, p.B, p.L);
    VQ_REQUIRE(((uintptr_t)p.hall & 15) == 0 && ((uintptr_t)p.w1 & 15) == 0 && ((uintptr_t)p.w2 & 15) == 0,
               "vocoder.nll: operands must be 16-byte aligned");
    const int tiles = vq_tf_nll_tiles(p.CH);
    hipLaunchKernelGGL(tf_nll_kernel, dim3(tiles, p.B), dim3(256), sizeof(NllLds), s, p);
    hipLaunchKernelGGL(tf_nll_finish_kernel, dim3((p.B + 63) / 64), dim3(64), 0, s, (const NllPart *)p.part, p.B, tiles, nll_sum,
                       n_scored, n_correct);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
