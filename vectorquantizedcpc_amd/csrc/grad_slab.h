// Fixed-order sums over rows.  Slabs: the split-K weight gradients of cpc_grad.hip (dW, db) and context_grad.hip (dW_ih, dW_hh, db)
// run slab_mfma_tile / slab_column_sum, each with its own row maps; a finish kernel then adds the slab partials in slab order.  Whole
// sums in one workgroup: the kernel bodies behind grad_rows.hip, vocoder_grad.hip and prenet_grad.hip.
#pragma once
#include "ar_shared.h"

constexpr int GRAD_SLAB = 1024;      // consecutive rows per slab
constexpr int GRAD_AHEAD = 4;        // MFMA steps of a wave whose operand loads are issued together

// NA x NB tiles of 16 x 16 of A^T B over the rows [r0, r0 + GRAD_SLAB) below R on v_mfma_f32_16x16x4_f32.  a(r, ia), b(r, ib): this
// lane's element of row r of A (row lane & 15 of A's tile ia) and of B (column lane & 15 of B's tile ib); ks = lane >> 4.  Every
// tile is summed on its own, in one order: MFMA (s, q) takes rows r0 + 16 s + 4 kslot + q, kslot 0 .. 3 summed inside the
// instruction; q even goes to accumulator 0, q odd to accumulator 1, s ascending, the two added once at the end.  Rows past R add
// exact zeros.  out[ia][ib]: row 4 ks + r of the tile, column lane & 15.  More than one tile per wave shares the operand loads
// among them (NA + NB loads for NA NB MFMAs) and changes no sum.
template <int NA, int NB, class FA, class FB>
__device__ __forceinline__ void slab_mfma_block(int R, int r0, int ks, FA a, FB b, f32x4 (&out)[NA][NB]) {
    f32x4 a0[NA][NB], a1[NA][NB];
#pragma unroll
    for (int ia = 0; ia < NA; ++ia)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) a0[ia][ib] = a1[ia][ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < GRAD_SLAB / 16 && r0 + 16 * s0 < R; s0 += GRAD_AHEAD) {
        float av[GRAD_AHEAD][NA][4], bv[GRAD_AHEAD][NB][4];
#pragma unroll
        for (int u = 0; u < GRAD_AHEAD; ++u) {           // the loads of GRAD_AHEAD steps in flight together, then their MFMAs in order
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * (s0 + u) + 4 * ks + q;
#pragma unroll
                for (int ia = 0; ia < NA; ++ia) av[u][ia][q] = r < R ? a(r, ia) : 0.f;
#pragma unroll
                for (int ib = 0; ib < NB; ++ib) bv[u][ib][q] = r < R ? b(r, ib) : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < GRAD_AHEAD; ++u)
#pragma unroll
            for (int ia = 0; ia < NA; ++ia)
#pragma unroll
                for (int ib = 0; ib < NB; ++ib)
                    mfma_k4(a0[ia][ib], a1[ia][ib], make_float4(av[u][ia][0], av[u][ia][1], av[u][ia][2], av[u][ia][3]),
                            make_float4(bv[u][ib][0], bv[u][ib][1], bv[u][ib][2], bv[u][ib][3]));
    }
#pragma unroll
    for (int ia = 0; ia < NA; ++ia)
#pragma unroll
        for (int ib = 0; ib < NB; ++ib) out[ia][ib] = a0[ia][ib] + a1[ia][ib];
}

// One such tile: a(r), b(r).
template <class FA, class FB>
__device__ __forceinline__ f32x4 slab_mfma_tile(int R, int r0, int ks, FA a, FB b) {
    f32x4 out[1][1];
    slab_mfma_block<1, 1>(R, r0, ks, [&](int r, int) { return a(r); }, [&](int r, int) { return b(r); }, out);
    return out[0][0];
}

// ---- The sums over ALL rows below p.R as kernels.  P is a struct of the operands with their row maps: grad_rows.hip has the plain
// ones (vq_grad_atb, vq_grad_colsum, vq_grad_rows_w), vocoder_grad.hip and prenet_grad.hip instantiate the same bodies with theirs.

// A^T B, one 16 x 16 tile per wave: every slab in slab order from 0 (slab_mfma_tile), the slabs' sums added in that order from +0.
// grid (column tiles of B, ceil(columns of A / 64)): wave w of workgroup (x, y) owns the output rows 64 y + 16 w .. + 15, columns
// 16 x .. + 15.  P: R, a(r, m), b(r, c), put(m, c, sum).
template <class P>
__global__ __launch_bounds__(256) void grad_atb_kernel(P p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, ks = lane >> 4;
    const int m0 = blockIdx.y * 64 + wave * 16, c = blockIdx.x * 16 + i;
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    for (int r0 = 0; r0 < p.R; r0 += GRAD_SLAB)
        sum = sum + slab_mfma_tile(p.R, r0, ks, [&](int r) { return p.a(r, m0 + i); }, [&](int r) { return p.b(r, c); });
#pragma unroll
    for (int e = 0; e < 4; ++e) p.put(m0 + ks * 4 + e, c, sum[e]);     // row 4 ks + e of the tile, column i
}

// Column sums, out[m] += sum_r a(r, m), 64 columns per workgroup: thread (column, row group g = 0 .. 3) adds rows g + 4 i, i
// ascending, into four accumulators (i mod 4) combined (a0 + a1) + (a2 + a3); the four row groups are combined the same way.
// grid (columns / 64).  P: R, a(r, m), out.
template <class P>
__global__ __launch_bounds__(256) void grad_colsum_kernel(P p) {
    __shared__ float red[4][64];
    const int d = threadIdx.x & 63, rg = threadIdx.x >> 6, m = blockIdx.x * 64 + d;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; rg + 4 * i < p.R; i += 4) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = rg + 4 * (i + e);
            a[e] += r < p.R ? p.a(r, m) : 0.f;
        }
    }
    red[rg][d] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    if (rg == 0) p.out[m] = p.out[m] + ((red[0][d] + red[1][d]) + (red[2][d] + red[3][d]));
}

// out (R, N) = A W for A (rows of K) and W (K rows of ldw, columns [0, N)), one 16 x 16 tile per workgroup; K % 64 == 0, N % 16 == 0.
// Wave w takes k in [w K / 4, (w + 1) K / 4) in super-steps S of 16; MFMA c (c = 0 .. 3) takes k = 16 S + 4 q + c, q = 0 .. 3 summed
// in that order inside the instruction; c even goes to accumulator 0, c odd to accumulator 1, S ascending (mfma_k4); the wave's sum
// is a0 + a1 and the four waves are combined ((w0 + w1) + w2) + w3 (reduce4).  grid (ceil(R / 16), N / 16).
// P: src(r) = A's row that output row r reads, or -1: the row is masked -- exact zeros enter, nothing is read and nothing stored;
// value(r, c, v) = what is stored for the product v.
template <class P>
__global__ __launch_bounds__(256) void grad_rows_w_kernel(const float *__restrict__ A, const float *__restrict__ W, int ldw,
                                                          float *__restrict__ out, int R, int K, int N, P p) {
    __shared__ float red[4][16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, kq = lane >> 4;
    const int r0 = blockIdx.x * 16, c0 = blockIdx.y * 16, NS = K / 64;
    const long long src = r0 + i < R ? p.src(r0 + i) : -1;
    const float4 *ap = (const float4 *)(A + (size_t)(src < 0 ? 0 : src) * K) + (size_t)wave * NS * 4 + kq;
    const float *wp = W + ((size_t)wave * NS * 16 + 4 * kq) * ldw + c0 + i;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < NS; ++s) {
        float4 av = make_float4(0.f, 0.f, 0.f, 0.f);
        if (src >= 0) av = ap[4 * s];
        const float *w = wp + (size_t)16 * s * ldw;
        mfma_k4(a0, a1, av, make_float4(w[0], w[ldw], w[2 * (size_t)ldw], w[3 * (size_t)ldw]));
    }
    const float v = reduce4(red, a0 + a1, wave, lane, tid);            // row r0 + (tid >> 4), column c0 + (tid & 15)
    const int r = r0 + (tid >> 4), c = c0 + (tid & 15);
    if (r < R && p.src(r) >= 0) out[(size_t)r * N + c] = p.value(r, c, v);
}

// Column sums of the same slab on the vector ALU, 256 threads = (column d = tid & 63, row group rg = tid >> 6): the thread adds
// rows r0 + rg + 4 i of `col` (stride floats apart), i ascending, into four accumulators (i mod 4) combined (a0 + a1) + (a2 + a3);
// the four row groups are combined the same way (through `red`; every thread returns its column's sum).  Sixteen short chains and a
// tree: the terms of a bias gradient largely share a sign, so a long chain's rounding errors would add up where a weight gradient's cancel.
__device__ __forceinline__ float slab_column_sum(const float *col, size_t stride, long long R, long long r0, int rg, int d, float (*red)[64]) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < GRAD_SLAB / 4 && r0 + 4 * i < R; i += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long long r = r0 + rg + 4 * (i + q);
            a[q] += r < R ? col[(size_t)r * stride] : 0.f;             // rows past R add exact zeros
        }
    }
    red[rg][d] = (a[0] + a[1]) + (a[2] + a[3]);
    __syncthreads();
    return (red[0][d] + red[1][d]) + (red[2][d] + red[3][d]);
}
