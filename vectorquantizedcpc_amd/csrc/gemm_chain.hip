// gemm_chain.hip -- the exact-chain fp32 GEMM of the library: the encoder's layered schedule, the mel front end, the
// recurrent scans' hoisted input projections and the vocoder's batched fc1 / fc2 all run on it.  A dot product is a
// k-ascending fmaf chain (v_mfma_f32_32x32x2_f32), restarted at the K-block boundaries the reference's MKL / oneDNN kernels
// use and folded in their order (oracle/vqcpc_oracle.c).  Build with -ffp-contract=off.
#include "encoder_internal.h"

// ------------------------------------------------------------------------------------------
// Exact-chain GEMM: 64x64 output tile per 256-thread workgroup, 4 waves as 2x2 of 32x32,
// one v_mfma_f32_32x32x2_f32 per two k.  LDS tiles are k-major ([k][row], stride 65) so the
// MFMA operand reads are conflict-free row-contiguous b32 reads.
// ------------------------------------------------------------------------------------------
#define GT_BM 64
#define GT_BN 64
#define GT_BK 32
#define GT_LD 65

struct GemmP {
    const float *A; int lda;
    const float *W;            // (N, K) row-major
    const float *bias;         // (N) or null
    float *Y; int ldy;
    int M, N, K, KC;
    // im2col source (AMODE 1/2): mel (B, C, T)
    const float *x; int C, T, To;
    // epilogue extras (vq_gemm_chain_ex): ReLU; output row m -> (m / ydiv) * ystride + yoff + m % ydiv, rows whose
    // yoff + m % ydiv >= ylim are not stored (ydiv == 0: row m)
    int relu, ydiv, ystride, yoff, ylim;
};

template <int AMODE>
__device__ __forceinline__ void fetch_a(const GemmP &p, int m0, int k0, int tid, float (&v)[8]) {
    const int row = tid >> 2, kq = (tid & 3) * 8;
    const int m = m0 + row;
    if (AMODE == 0) {
        if (m < p.M) {
            const float4 *src = (const float4 *)(p.A + (size_t)m * p.lda + k0 + kq);
            float4 a = src[0], b = src[1];
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = 0.f;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = im2col_at(p.x, p.C, p.T, p.To, p.M, m, k0 + kq + i, AMODE);
    }
}
__device__ __forceinline__ void fetch_w(const GemmP &p, int n0, int k0, int tid, float (&v)[8]) {
    const int row = tid >> 2, kq = (tid & 3) * 8;
    const float4 *src = (const float4 *)(p.W + (size_t)(n0 + row) * p.K + k0 + kq);
    float4 a = src[0], b = src[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void stage(float (*T)[GT_LD], int tid, const float (&v)[8]) {
    const int row = tid >> 2, kq = (tid & 3) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) T[kq + i][row] = v[i];
}

__device__ __forceinline__ void gemm_epilogue(const GemmP &p, const f32x16 &tot, int m0, int wm, int half, int col) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (m >= p.M) continue;
        size_t row = (size_t)m;
        if (p.ydiv > 0) {
            const int q = m / p.ydiv, t = p.yoff + (m - q * p.ydiv);
            if (t >= p.ylim) continue;
            row = (size_t)q * p.ystride + t;
        }
        const float v = tot[r];
        p.Y[row * p.ldy + col] = (p.relu && v < 0.f) ? 0.f : v;
    }
}

// Software pipeline.  A loop that does, per k tile, {wait for global loads, 16 LDS stores, barrier, 32 LDS
// operand reads} and then its 16 MFMAs pays for both halves: measured on MI355X, 17 us of MFMA + 16 us of
// LDS work for a 4096 x 512 x 512 layer that ran 28.6 us (tools/microbench_mfma.hip).  Here the
// LDS tiles are double-buffered and every MFMA gap carries its share of the other work, in program order
// (pinned with sched_barrier): MFMAs 0-7 of tile k are interleaved with the LDS stores of tile k+1, then the
// global loads of tile k+2 are requested, one barrier, and MFMAs 8-15 are interleaved with the operand
// reads of tile k+1 into a second register set.  22.5 us for the same layer, same k order, same bits.
template <int AMODE, int C>
__device__ __forceinline__ void pipe_body(const GemmP &p, float (*As)[GT_BK][GT_LD], float (*Ws)[GT_BK][GT_LD], int tid,
                                          int m0, int n0, int k2, float (&va)[8], float (&vw)[8], float (&oa)[2][16],
                                          float (&ob)[2][16], f32x16 &acc, int acol, int bcol, int half) {
    const int row = tid >> 2, kq = (tid & 3) * 8;
    float (*An)[GT_LD] = As[C ^ 1];
    float (*Wn)[GT_LD] = Ws[C ^ 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(oa[C][j], ob[C][j], acc, 0, 0, 0);
        An[kq + j][row] = va[j];
        Wn[kq + j][row] = vw[j];
        __builtin_amdgcn_sched_barrier(0);
    }
    fetch_a<AMODE>(p, m0, k2, tid, va);
    fetch_w(p, n0, k2, tid, vw);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(oa[C][8 + j], ob[C][8 + j], acc, 0, 0, 0);
        oa[C ^ 1][2 * j] = An[4 * j + half][acol];
        oa[C ^ 1][2 * j + 1] = An[4 * j + 2 + half][acol];
        ob[C ^ 1][2 * j] = Wn[4 * j + half][bcol];
        ob[C ^ 1][2 * j + 1] = Wn[4 * j + 2 + half][bcol];
        __builtin_amdgcn_sched_barrier(0);
    }
}

__device__ __forceinline__ void fold_chain(const GemmP &p, f32x16 &acc, f32x16 &tot, bool &first, float bv) {
    if (first) {
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = p.bias ? bv + acc[r] : acc[r];
        first = false;
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[r] = tot[r] + acc[r];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
}

template <int AMODE>
__global__ __launch_bounds__(256) void gemm_chain_kernel(GemmP p) {
    __shared__ float As[2][GT_BK][GT_LD];
    __shared__ float Ws[2][GT_BK][GT_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, half = lane >> 5, li = lane & 31;
    const int n0 = blockIdx.x * GT_BN, m0 = blockIdx.y * GT_BM;
    const int col = n0 + wn * 32 + li, acol = wm * 32 + li, bcol = wn * 32 + li;
    const int nt = p.K / GT_BK, tpb = p.KC / GT_BK;

    f32x16 acc, tot;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.f; tot[r] = 0.f; }
    bool first = true;
    const float bv = p.bias ? p.bias[col] : 0.f;

    float va[8], vw[8], oa[2][16], ob[2][16];
    fetch_a<AMODE>(p, m0, 0, tid, va);
    fetch_w(p, n0, 0, tid, vw);
    stage(As[0], tid, va);
    stage(Ws[0], tid, vw);
    const int k1 = nt > 1 ? GT_BK : 0;
    fetch_a<AMODE>(p, m0, k1, tid, va);
    fetch_w(p, n0, k1, tid, vw);
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
        oa[0][kk] = As[0][2 * kk + half][acol];
        ob[0][kk] = Ws[0][2 * kk + half][bcol];
    }

    int k = 0;
    for (; k + 2 < nt; k += 2) {
        pipe_body<AMODE, 0>(p, As, Ws, tid, m0, n0, (k + 2) * GT_BK, va, vw, oa, ob, acc, acol, bcol, half);
        if ((k + 1) % tpb == 0) fold_chain(p, acc, tot, first, bv);
        pipe_body<AMODE, 1>(p, As, Ws, tid, m0, n0, (k + 3 < nt ? k + 3 : nt - 1) * GT_BK, va, vw, oa, ob, acc, acol, bcol, half);
        if ((k + 2) % tpb == 0) fold_chain(p, acc, tot, first, bv);
    }
    if (k + 1 < nt) {                                                 // two tiles left
        pipe_body<AMODE, 0>(p, As, Ws, tid, m0, n0, (nt - 1) * GT_BK, va, vw, oa, ob, acc, acol, bcol, half);
        if ((k + 1) % tpb == 0) fold_chain(p, acc, tot, first, bv);
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(oa[1][kk], ob[1][kk], acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(oa[0][kk], ob[0][kk], acc, 0, 0, 0);
    }
    fold_chain(p, acc, tot, first, bv);

    gemm_epilogue(p, tot, m0, wm, half, col);
}

template <int AMODE>
static int launch_gemm(const GemmP &p, hipStream_t s) {
    VQ_REQUIRE(p.N % GT_BN == 0 && p.K % GT_BK == 0 && p.KC % GT_BK == 0 && p.M > 0,
               "gemm_chain: unsupported shape M=%d N=%d K=%d KC=%d", p.M, p.N, p.K, p.KC);
    dim3 grid(p.N / GT_BN, (p.M + GT_BM - 1) / GT_BM);
    hipLaunchKernelGGL((gemm_chain_kernel<AMODE>), grid, dim3(256), 0, s, p);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

int vq_gemm_chain(const float *A, int lda, const float *W, const float *bias, float *Y, int ldy,
                  int M, int N, int K, int KC, hipStream_t s) {
    return vq_gemm_chain_ex(A, lda, W, bias, Y, ldy, M, N, K, KC, 0, 0, 0, 0, 0, s);
}

int vq_gemm_chain_ex(const float *A, int lda, const float *W, const float *bias, float *Y, int ldy,
                     int M, int N, int K, int KC, int relu, int ydiv, int ystride, int yoff, int ylim, hipStream_t s) {
    VQ_REQUIRE(lda % 4 == 0 && ((uintptr_t)A & 15) == 0 && ((uintptr_t)W & 15) == 0,
               "gemm_chain: operands must be 16-byte aligned");
    GemmP p{};
    p.A = A; p.lda = lda; p.W = W; p.bias = bias; p.Y = Y; p.ldy = ldy;
    p.M = M; p.N = N; p.K = K; p.KC = KC;
    p.relu = relu; p.ydiv = ydiv; p.ystride = ystride; p.yoff = yoff; p.ylim = ylim;
    return launch_gemm<0>(p, s);
}

int vq_gemm_chain_im2col(const float *mel, int C, int T, int To, const float *W, float *Y, int M, int N, int KC, int mode, hipStream_t s) {
    GemmP p{};
    p.W = W; p.Y = Y; p.ldy = N; p.M = M; p.N = N; p.K = 4 * C; p.KC = KC;
    p.x = mel; p.C = C; p.T = T; p.To = To;
    return mode == VQCPC_CONV_IM2COL ? launch_gemm<1>(p, s) : launch_gemm<2>(p, s);
}
