// Fixed-order sums over slabs of rows: the split-K weight gradients of cpc_grad.hip (dW, db) and context_grad.hip (dW_ih, dW_hh,
// db) run these statements, each with its own row maps; a finish kernel then adds the slab partials in slab order.
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
