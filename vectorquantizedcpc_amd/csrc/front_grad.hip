// Gradients of the encoder's front end, Encoder.conv + Encoder.encoder (model.py:43-55, :65-67), and of the VQ step's
// straight-through estimator (model.py:147-150): a forward that keeps what the backward reads again, and the backward -- what
// loss.backward() does below z in train_cpc.py:116-124.  Entry points: include/vqcpc.h (encoder_host.hip).
// B utterances of T mel frames, To = T / 2 output frames, rows r = b To + tt, R = B To; C = in_channels; layers l = 0 .. 4:
//   x_0 = conv(mel), a_l = ReLU(LN_l(x_l)), x_{l+1} = a_l W_l^T (l < 4), z_pre = a_4 W_out^T + b_out.
// Every sum has ONE order, fixed by the code and independent of the grid's timing: no floating-point read-modify-write on global
// memory, no wait on another workgroup; launch boundaries order the passes.  Equal inputs give equal bits.  Every operation below
// is one separately rounded fp32 operation (-ffp-contract=off); every accumulator starts from +0.
//
// Forward (vq_front_fwd): vq_front_chain of encoder_host.hip, the function that IS the layered schedule of vqcpc_encoder_stage,
//   called with the views of `saved` as its destinations, so z_pre has the bits of vqcpc_encoder_stage(10).  saved = x_0 .. x_4
//   (R, 512 each), a_0 .. a_4 (R, 512 each), then (mean, rstd) of every row of LN_0 .. LN_4 (R, 2 each) as ln512_kernel computed
//   them.  A caller's conv.weight is first brought into the two k orders (launch_conv_weight_permute), in stream order.
//
// Backward (vq_front_bwd), from the top; G = dLoss / dz_pre (R, 64); a pass whose products nobody asked for is not launched:
//   dW_out = G^T a_4, dW_l = dy_{l+1}^T a_l, dW_conv = dy_0^T im2col(mel): front_grad_w_kernel, grid (column pairs of tiles of 16,
//     output rows / 128 (/ 64 for the out layer), slabs); a wave holds 2 x 2 (1 x 2) tiles that share their operand loads, each
//     tile summed on its own.  A slab is GRAD_SLAB = 1024 consecutive rows; inside a slab slab_mfma_block (grad_slab.h, the statements
//     of ctx_grad_w_kernel and cpc_grad_w_kernel): MFMA (s, c) takes rows r0 + 16 s + 4 q + c, q = 0 .. 3 summed inside the
//     instruction, c even to accumulator 0, c odd to accumulator 1, s ascending, the two added once at the end.  The conv reads its
//     operand through im2col_at in the layout of conv.weight (k = 4 c + tap): zeros at utterance edges and for the frame an odd T
//     leaves over; no im2col matrix is stored.  front_sum_parts_kernel adds the slab partials in slab order.
//   db_out = column sums of G: front_grad_bias_kernel, the same slabs through slab_column_sum (grad_slab.h), finished in slab order.
//   da_4 = G W_out, da_{l-1} = dy_l W_{l-1}: vq_gemm_chain on a transpose of the weight made in stream order
//     (transpose_kernel); k ascending, the chain restarted every 64 k and the blocks folded in ascending order.
//   LayerNorm + ReLU backward: front_ln_bwd_kernel, one wave per row, a workgroup of four waves per tile of 16 rows, wave w takes
//     rows 16 tile + 4 w + j, j ascending.  Lane n holds columns 256 h + 4 n + k (h = 0, 1; k = 0 .. 3).  Per element
//       xhat = (x - mean) * rstd   dn = a > 0 ? da : 0   dxh = dn * gamma
//     the lane adds its eight dxh, and its eight dxh * xhat, in the order (h, k) ascending; the 64 lane sums are combined by a
//     butterfly over lane distances 1, 2, 4, 8, 16, 32 in that order (every lane ends with the same bits); the sums times 1 / 512 are
//     the two means m1, m2, and
//       dy = rstd * ((dxh - m1) - xhat * m2)
//     overwrites da.  The mask is the saved a > 0, never recomputed from x.  In the same pass the wave adds dn (for dbeta) and
//     dn * xhat (for dgamma) of its four rows per column, j ascending; the four waves are combined ((w0 + w1) + w2) + w3 into
//     the tile's partial.  Rows >= R of the last tile are skipped: they contribute nothing.  front_ln_slab_kernel: per column
//     and slab, the slab's 64 tiles t go to four accumulators (t mod 4), t ascending, combined (a0 + a1) + (a2 + a3);
//     front_sum_parts_kernel adds the slab sums in slab order.
//   vq_bwd_kernel: the element-wise statements vqcpc.h gives.
//
// Dirt: every partial that a finish kernel reads was written by the same call (the grids cover exactly the tiles and slabs
// below R); the (R, 512) buffers are written for every row below R before they are read.  Nothing is zero-filled.
#include "encoder_internal.h"
#include "grad_slab.h"

namespace {

constexpr int CH = 512, ZD = 64, LN_TILE = 16;

// part (slabs, M, K) = per slab dy^T act.  A wave owns NA x 2 tiles of 16 x 16: output units m0 + 16 NA wave + 16 ia + (0 .. 15),
// columns 32 ct + 16 ib + (0 .. 15); the workgroup 64 NA units.  NA = 2 where M allows it (four tiles share four operand loads).
template <bool CONV, int NA>
__global__ __launch_bounds__(256) void front_grad_w_kernel(const float *__restrict__ dy, int M, const float *__restrict__ act, int K,
                                                           const float *__restrict__ mel, int C, int T, int To,
                                                           float *__restrict__ part, int R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, ks = lane >> 4;
    const int slab = blockIdx.z, r0 = slab * GRAD_SLAB;
    const int m = blockIdx.y * 64 * NA + wave * 16 * NA + i, col = blockIdx.x * 32 + i;
    const auto a = [&](int r, int ia) { return dy[(size_t)r * M + m + 16 * ia]; };
    f32x4 acc[NA][2];
    if (CONV) slab_mfma_block<NA, 2>(R, r0, ks, a, [&](int r, int ib) { return im2col_at(mel, C, T, To, R, r, col + 16 * ib, 1); }, acc);
    else slab_mfma_block<NA, 2>(R, r0, ks, a, [&](int r, int ib) { return act[(size_t)r * K + col + 16 * ib]; }, acc);
#pragma unroll
    for (int ia = 0; ia < NA; ++ia)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
            for (int r = 0; r < 4; ++r)                  // row = the tile's unit 4 ks + r, column = the tile's column i
                part[((size_t)slab * M + (m - i) + 16 * ia + ks * 4 + r) * K + col + 16 * ib] = acc[ia][ib][r];
}

// part (slabs, 64): column sums of G (R, 64) per slab.
__global__ __launch_bounds__(256) void front_grad_bias_kernel(const float *__restrict__ G, float *__restrict__ part, int R) {
    __shared__ float red[4][64];
    const int d = threadIdx.x & 63, rg = threadIdx.x >> 6, slab = blockIdx.x;
    const float sum = slab_column_sum(G + d, ZD, R, (long long)slab * GRAD_SLAB, rg, d, red);
    if (rg == 0) part[(size_t)slab * ZD + d] = sum;
}

// out[e] = part[0][e] + part[1][e] + ... in slab order, e < n; the slabs are `stride` floats apart.
__global__ __launch_bounds__(256) void front_sum_parts_kernel(const float *__restrict__ part, float *__restrict__ out, int S, size_t n,
                                                              size_t stride) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += part[(size_t)s * stride + e];
    out[e] = sum;
}

// out (cols, rows) = in (rows, cols)^T
__global__ __launch_bounds__(256) void transpose_kernel(const float *__restrict__ in, float *__restrict__ out, int rows, int cols) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= rows * cols) return;
    const int c = e / rows, r = e - c * rows;
    out[e] = in[(size_t)r * cols + c];
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = v + __shfl_xor(v, d);
    return v;
}

// d (R, 512): da in, dy out.  colpart (tiles, 2, 512): [0] the tile's column sums of dn, [1] of dn * xhat; null = not wanted.
__global__ __launch_bounds__(256) void front_ln_bwd_kernel(float *__restrict__ d, const float *__restrict__ x, const float *__restrict__ a,
                                                           const float *__restrict__ stat, const float *__restrict__ gamma,
                                                           float *__restrict__ colpart, int R) {
    __shared__ __attribute__((aligned(16))) float red[4][2][CH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tile = blockIdx.x;
    float4 g[2];
    float sb[2][4], sg[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        g[h] = *(const float4 *)(gamma + 256 * h + 4 * lane);
#pragma unroll
        for (int k = 0; k < 4; ++k) sb[h][k] = sg[h][k] = 0.f;
    }
    for (int j = 0; j < 4; ++j) {
        const int r = tile * LN_TILE + wave * 4 + j;
        if (r >= R) break;                               // uniform over the wave
        const size_t at = (size_t)r * CH + 4 * lane;
        const float mean = stat[2 * (size_t)r], rstd = stat[2 * (size_t)r + 1];
        float xh[2][4], dxh[2][4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 dv = *(const float4 *)(d + at + 256 * h), xv = *(const float4 *)(x + at + 256 * h);
            const float4 av = *(const float4 *)(a + at + 256 * h);
            const float da[4] = {dv.x, dv.y, dv.z, dv.w}, xs[4] = {xv.x, xv.y, xv.z, xv.w}, as[4] = {av.x, av.y, av.z, av.w};
            const float gs[4] = {g[h].x, g[h].y, g[h].z, g[h].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                xh[h][k] = (xs[k] - mean) * rstd;
                const float dn = as[k] > 0.f ? da[k] : 0.f;
                dxh[h][k] = dn * gs[k];
                s1 = s1 + dxh[h][k];
                s2 = s2 + dxh[h][k] * xh[h][k];
                sb[h][k] = sb[h][k] + dn;
                sg[h][k] = sg[h][k] + dn * xh[h][k];
            }
        }
        const float m1 = wave_sum(s1) * (1.0f / 512.0f), m2 = wave_sum(s2) * (1.0f / 512.0f);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float4 o;
            o.x = rstd * ((dxh[h][0] - m1) - xh[h][0] * m2);
            o.y = rstd * ((dxh[h][1] - m1) - xh[h][1] * m2);
            o.z = rstd * ((dxh[h][2] - m1) - xh[h][2] * m2);
            o.w = rstd * ((dxh[h][3] - m1) - xh[h][3] * m2);
            *(float4 *)(d + at + 256 * h) = o;
        }
    }
    if (!colpart) return;                                // uniform over the grid
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        *(float4 *)&red[wave][0][256 * h + 4 * lane] = make_float4(sb[h][0], sb[h][1], sb[h][2], sb[h][3]);
        *(float4 *)&red[wave][1][256 * h + 4 * lane] = make_float4(sg[h][0], sg[h][1], sg[h][2], sg[h][3]);
    }
    __syncthreads();
#pragma unroll
    for (int e = threadIdx.x; e < 2 * CH; e += 256) {
        const int which = e >> 9, c = e & (CH - 1);
        colpart[((size_t)tile * 2 + which) * CH + c] = ((red[0][which][c] + red[1][which][c]) + red[2][which][c]) + red[3][which][c];
    }
}

// slabpart (slabs, 2, 512): the slab's sums of the tile partials.  Grid (slabs, 2 * 512 / 64); thread (column tid & 63, accumulator
// q = tid >> 6) adds tiles t0 + q + 4 i, i ascending; the four accumulators are combined (a0 + a1) + (a2 + a3).
__global__ __launch_bounds__(256) void front_ln_slab_kernel(const float *__restrict__ colpart, float *__restrict__ slabpart, int tiles) {
    __shared__ float red[4][64];
    constexpr int TPS = GRAD_SLAB / LN_TILE;             // tiles per slab
    const int d = threadIdx.x & 63, q = threadIdx.x >> 6, slab = blockIdx.x;
    const int e = blockIdx.y * 64 + d, which = e >> 9, c = e & (CH - 1);
    float acc = 0.f;
    for (int t = slab * TPS + q; t < (slab + 1) * TPS && t < tiles; t += 4) acc += colpart[((size_t)t * 2 + which) * CH + c];
    red[q][d] = acc;
    __syncthreads();
    if (q == 0) slabpart[((size_t)slab * 2 + which) * CH + c] = (red[0][d] + red[1][d]) + (red[2][d] + red[3][d]);
}

__global__ __launch_bounds__(256) void vq_bwd_kernel(const float *__restrict__ z_pre, const float *__restrict__ z_q, size_t n, float scale,
                                                     const float *__restrict__ grad_z_st, const float *__restrict__ grad_loss,
                                                     float *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (!grad_loss) { out[e] = grad_z_st[e]; return; }
    const float d = z_pre[e] - z_q[e];
    const float s = grad_loss[0] * scale;
    const float t = s * d;
    out[e] = grad_z_st ? grad_z_st[e] + t : t;
}

// `saved` as the layered schedule's destinations: every layer's rows and statistics in a place of their own.
FrontDst saved_view(const float *saved, size_t R, float *z_pre = nullptr) {
    float *s = const_cast<float *>(saved);
    FrontDst v;
    for (int l = 0; l < 5; ++l) { v.x[l] = s + l * R * CH; v.a[l] = s + (5 + l) * R * CH; v.stat[l] = s + 10 * R * CH + l * 2 * R; }
    v.z_pre = z_pre;
    return v;
}

}  // namespace

size_t vq_front_saved_bytes(int B, int To) { return (size_t)B * To * (10 * CH + 10) * sizeof(float); }

void launch_vq_bwd(const float *z_pre, const float *z_q, size_t n, float scale, const float *grad_z_st, const float *grad_loss,
                   float *grad_z_pre, hipStream_t s) {
    hipLaunchKernelGGL(vq_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z_pre, z_q, n, scale, grad_z_st, grad_loss, grad_z_pre);
}

int vq_front_fwd(FrontGradWork &k, FrontW w, const LnConst &lnc, const float *mel, int B, int C, int T, int conv_mode, float *z_pre,
                 float *saved, hipStream_t s) {
    if (!w.conv_w1) {                                    // a caller's conv.weight: the two k orders, in stream order
        const size_t nconv = (size_t)CH * C * 4;
        TRY(k.convw.reserve(2 * nconv * sizeof(float)));
        float *w1 = k.convw.as<float>(), *w2 = w1 + nconv;
        launch_conv_weight_permute(w.t.conv_weight, w1, w2, CH, C, s);
        w.conv_w1 = w1; w.conv_w2 = w2;
    }
    const float *unused = nullptr;
    return vq_front_chain(w, lnc, mel, B, C, T, conv_mode, 10, saved_view(saved, (size_t)B * ((T - 2) / 2 + 1), z_pre), &unused, s);
}

int vq_front_bwd(FrontGradWork &k, const FrontW &w, const float *mel, int B, int C, int T, const float *saved, const float *grad_z_pre,
                 const FrontG &g, hipStream_t s) {
    const int To = (T - 2) / 2 + 1, R = B * To;
    const int slabs = (R + GRAD_SLAB - 1) / GRAD_SLAB, tiles = (R + LN_TILE - 1) / LN_TILE;
    const FrontDst v = saved_view(saved, (size_t)R);
    // how far down the chain goes: da_l is needed for LN_l's own gradients and for dy_l; dy_l for the weight below it and for da_{l-1}
    bool need_da[5], need_dy[5];
    for (int l = 0; l < 5; ++l) {
        need_dy[l] = l == 0 ? g.conv_weight != nullptr : (g.fc_weight[l - 1] != nullptr || need_da[l - 1]);
        need_da[l] = g.ln_weight[l] || g.ln_bias[l] || need_dy[l];
    }
    bool any_w = g.conv_weight || g.out_weight || g.out_bias, any_ln = false;
    for (int l = 0; l < 4; ++l) any_w = any_w || g.fc_weight[l];
    for (int l = 0; l < 5; ++l) any_ln = any_ln || g.ln_weight[l] || g.ln_bias[l];
    const int kmax = g.conv_weight && 4 * C > CH ? 4 * C : CH;
    if (any_w) TRY(k.part.reserve(up256((size_t)slabs * CH * kmax * sizeof(float))));
    if (any_ln) TRY(k.colpart.reserve(up256((size_t)(tiles + slabs) * 2 * CH * sizeof(float))));      // tile partials, then slab sums
    if (need_da[4]) {
        TRY(k.wT.reserve((size_t)CH * CH * sizeof(float)));
        TRY(k.d0.reserve(up256((size_t)R * CH * sizeof(float))));
        TRY(k.d1.reserve(up256((size_t)R * CH * sizeof(float))));
    }
    float *part = k.part.as<float>(), *wT = k.wT.as<float>();
    const dim3 blk(256);
    const auto finish = [&](float *out, size_t n) {
        hipLaunchKernelGGL(front_sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), blk, 0, s, (const float *)part, out, slabs, n, n);
    };
    const auto transpose = [&](const float *W, int rows, int cols) {
        hipLaunchKernelGGL(transpose_kernel, dim3((rows * cols + 255) / 256), blk, 0, s, W, wT, rows, cols);
    };

    // the out layer (model.py:55)
    if (g.out_weight) {
        hipLaunchKernelGGL((front_grad_w_kernel<false, 1>), dim3(CH / 32, ZD / 64, slabs), blk, 0, s, grad_z_pre, ZD, (const float *)v.a[4], CH,
                           nullptr, 0, 0, 0, part, R);
        finish(g.out_weight, (size_t)ZD * CH);
    }
    if (g.out_bias) {
        hipLaunchKernelGGL(front_grad_bias_kernel, dim3(slabs), blk, 0, s, grad_z_pre, part, R);
        finish(g.out_bias, ZD);
    }
    float *d = k.d0.as<float>(), *dn = k.d1.as<float>();
    if (need_da[4]) {
        transpose(w.t.out_weight, ZD, CH);                                    // (512, 64): da_4 = G W_out
        TRY(vq_gemm_chain(grad_z_pre, ZD, wT, nullptr, d, CH, R, CH, ZD, 64, s));
    }
    for (int l = 4; l >= 0 && need_da[l]; --l) {
        const bool ln = g.ln_weight[l] || g.ln_bias[l];
        hipLaunchKernelGGL(front_ln_bwd_kernel, dim3(tiles), blk, 0, s, d, (const float *)v.x[l], (const float *)v.a[l],
                           (const float *)v.stat[l], w.t.ln_weight[l], ln ? k.colpart.as<float>() : nullptr, R);
        if (ln) {                                                             // the tile partials by slab, then the slabs in order
            const float *slabpart = k.colpart.as<float>() + (size_t)tiles * 2 * CH;
            hipLaunchKernelGGL(front_ln_slab_kernel, dim3(slabs, 2 * CH / 64), blk, 0, s, (const float *)k.colpart.as<float>(),
                               k.colpart.as<float>() + (size_t)tiles * 2 * CH, tiles);
            if (g.ln_bias[l]) hipLaunchKernelGGL(front_sum_parts_kernel, dim3(CH / 256), blk, 0, s, slabpart, g.ln_bias[l], slabs, (size_t)CH, (size_t)2 * CH);
            if (g.ln_weight[l]) hipLaunchKernelGGL(front_sum_parts_kernel, dim3(CH / 256), blk, 0, s, slabpart + CH, g.ln_weight[l], slabs, (size_t)CH, (size_t)2 * CH);
        }
        if (l == 0) {
            if (g.conv_weight) {                                              // dW_conv in the layout of conv.weight: k = 4 c + tap
                hipLaunchKernelGGL((front_grad_w_kernel<true, 2>), dim3(4 * C / 32, CH / 128, slabs), blk, 0, s, (const float *)d, CH, nullptr,
                                   4 * C, mel, C, T, To, part, R);
                finish(g.conv_weight, (size_t)CH * 4 * C);
            }
            break;
        }
        if (g.fc_weight[l - 1]) {
            hipLaunchKernelGGL((front_grad_w_kernel<false, 2>), dim3(CH / 32, CH / 128, slabs), blk, 0, s, (const float *)d, CH,
                               (const float *)v.a[l - 1], CH, nullptr, 0, 0, 0, part, R);
            finish(g.fc_weight[l - 1], (size_t)CH * CH);
        }
        if (need_da[l - 1]) {
            transpose(w.t.fc_weight[l - 1], CH, CH);
            TRY(vq_gemm_chain(d, CH, wT, nullptr, dn, CH, R, CH, CH, 64, s));
            float *t = d; d = dn; dn = t;
        }
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
