// Fixed-order sums over slabs of rows: the split-K weight gradients of cpc_grad.hip (dW, db) and context_grad.hip (dW_ih, dW_hh,
// db) run these statements, each with its own row maps; a finish kernel then adds the slab partials in slab order.
#pragma once
#include "ar_shared.h"

constexpr int GRAD_SLAB = 1024;      // consecutive rows per slab
constexpr int GRAD_AHEAD = 4;        // MFMA steps of a wave whose operand loads are issued together

// One 16 x 16 tile of A^T B over the rows [r0, r0 + GRAD_SLAB) below R on v_mfma_f32_16x16x4_f32.  a(r), b(r): this lane's element of
// row r of A (the tile's row lane & 15) and of B (the tile's column lane & 15); ks = lane >> 4.  MFMA (s, q) takes rows
// r0 + 16 s + 4 kslot + q, kslot 0 .. 3 summed inside the instruction; q even goes to accumulator 0, q odd to accumulator 1, s
// ascending, the two added once at the end.  Rows past R add exact zeros.  Result: row 4 ks + r of the tile, column lane & 15.
template <class FA, class FB>
__device__ __forceinline__ f32x4 slab_mfma_tile(int R, int r0, int ks, FA a, FB b) {
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < GRAD_SLAB / 16 && r0 + 16 * s0 < R; s0 += GRAD_AHEAD) {
        float av[GRAD_AHEAD][4], bv[GRAD_AHEAD][4];
#pragma unroll
        for (int u = 0; u < GRAD_AHEAD; ++u) {           // the loads of GRAD_AHEAD steps in flight together, then their MFMAs in order
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int r = r0 + 16 * (s0 + u) + 4 * ks + q;
                av[u][q] = bv[u][q] = 0.f;
                if (r < R) { av[u][q] = a(r); bv[u][q] = b(r); }
            }
        }
#pragma unroll
        for (int u = 0; u < GRAD_AHEAD; ++u)
            mfma_k4(a0, a1, make_float4(av[u][0], av[u][1], av[u][2], av[u][3]), make_float4(bv[u][0], bv[u][1], bv[u][2], bv[u][3]));
    }
    return a0 + a1;
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
