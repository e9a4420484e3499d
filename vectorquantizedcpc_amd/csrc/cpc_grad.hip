// CPC gradients: the backward of CPCLoss (model.py:191-316) for loss = mean_k mean_{n,t} (lse_j f - f_0), upstream gradient 1.
// With g[k,n,j,t] = (softmax_j f - delta_j0) / (K N L):
//     dWc[k,n,t,:] = (1/8) sum_j g_j zrow_j        db_k = sum_{n,t} dWc        dW_k = sum_{n,t} dWc[k,n,t,:]^T c[n,t,:]
//     dc[n,t,:]    = sum_k dWc[k,n,t,:] W_k  (t < L; zero for t >= L)
//     dz[row,:]    = (1/8) sum g Wc[k,n,t,:] over every (k,n,j,t) whose row j is `row`
// Every sum has ONE order, fixed by the code and independent of the grid's timing: there is no floating-point read-modify-write
// on global memory, no wait on another workgroup; launch boundaries order the passes.  Equal inputs give equal bits.
//
// Launches (a pass whose only products nobody asked for is skipped) and the summation order of each gradient:
//   cpc_grad_tile_kernel, grid (ceil(L / 16), N, n_steps) -- the grid of cpc_score_kernel.  Forward by the statements of
//     cpc_tile.h (the loss partials are those of vqcpc_cpc_score; cpc_finish_kernel follows), then per pair
//     g = (expf(f - m) / e - delta_j0) / (K N L) with m, e of the position's log-sum-exp, then
//     dWc[t, d] = 0.125 * chain_j fmaf(g_j, zrow_j[d], .) from 0, j = 0 (the positive), 1 .. Neg ascending.
//     Stores dWc (K, N, L, 64) and, when grad_z is wanted, Wc (K, N, L, 64), g (K, N, J, L) and the negatives' indices u
//     (K, Utt, Neg), s (K, N, Neg, L) as int32: the dz pass repeats no Philox draw.
//   dW: cpc_grad_w_kernel, grid (C / 16, slabs, n_steps): a split-K GEMM on v_mfma_f32_16x16x4_f32, A = dWc^T, B = c.  A slab is
//     GRAD_SLAB = 1024 consecutive rows r = n L + t.  Inside a slab MFMA (s, q) takes rows r0 + 16 s + 4 kslot + q, kslot 0 .. 3
//     summed inside the instruction; q even goes to accumulator 0, q odd to accumulator 1, s ascending, the two added once at
//     the end.  cpc_grad_w_finish_kernel adds the slab partials in slab order.
//   db: cpc_grad_b_kernel, grid (slabs, n_steps), the same slabs: thread (feature d, row group rg) adds rows r0 + rg + 4 i, i
//     ascending, into four accumulators (i mod 4) combined (a0 + a1) + (a2 + a3); the four row groups are combined the same way.
//     Sixteen short chains and a tree, on the vector ALU: the terms of db largely share a sign, so a long chain's rounding
//     errors would add up where dW's cancel.  The slab partials go through cpc_grad_w_finish_kernel as a column of their own.
//   dc: cpc_grad_c_kernel, grid (ceil(T / 16), N, C / 64), one MFMA chain per 16 x 16 output tile: k ascending, inside a step
//     MFMA (s, q) takes features 16 s + 4 kslot + q, accumulators as above.  Rows t >= L are stored as exact zeros.
//   dz: cpc_grad_z_kernel, grid (ceil(L / 64), N, n_steps): workgroup (tile, n' = (spk, u'), k) owns 64 destination positions
//     s of utterance n' in LDS (never a whole utterance: T is not limited), wave w the 16 of them from 16 w, lane d feature d.
//     Position s starts from the positive g[k,n',0,s] Wc[k,n',s,:], then the negatives that drew (u', s), walked as
//     (utt, j, t) ascending, each fmaf(g, Wc[d], .); times 0.125; stored as the step's partial (K, N, L, 64).
//     cpc_grad_z_sum_kernel: dz[n, tau, :] = sum of the partials [k][n][tau - k] for k = 1 .. n_steps ascending (those with
//     0 <= tau - k < L), from 0: row 0 has no term and is an exact zero.
#include "cpc_tile.h"
#include "grad_slab.h"

namespace {

constexpr int GZ_ROWS = 64;          // destination positions per dz workgroup
constexpr int GZ_FLIGHT = 8;         // contribution rows a dz wave loads before it adds them

struct CpcGradArgs {
    CpcArgs f;
    float *dWc, *Wc, *g;             // work space; Wc, g, u_out, s_out null unless grad_z is wanted
    int *u_out, *s_out;
    float count;                     // K N L
};

__global__ __launch_bounds__(256) void cpc_grad_tile_kernel(CpcGradArgs ga) {
    __shared__ __attribute__((aligned(16))) float wc[CPC_TT][CPC_WCS];
    __shared__ float sc[CPC_MAXJ][CPC_TT];
    __shared__ int rows[CPC_MAXJ][CPC_TT];
    __shared__ float pos_loss[CPC_TT], pos_m[CPC_TT], pos_e[CPC_TT];
    __shared__ int pos_correct[CPC_TT];

    const CpcArgs &a = ga.f;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, n = blockIdx.y, k = blockIdx.z + 1;
    const int t0 = tile * CPC_TT, N = a.Spk * a.Utt, L = a.L, J = 1 + a.Neg;

    // ---- forward: the statements of cpc_score_kernel
    cpc_wc_tile(a, wc, lane, wave, n, k, t0);
    __syncthreads();
    cpc_score_pairs(a, wc, sc, tid, tile, n, k, rows, ga.u_out, ga.s_out);
    __syncthreads();
    if (tid < CPC_TT) cpc_position(a, sc, pos_loss, pos_correct, tid, t0, n, k, pos_m, pos_e);
    __syncthreads();
    if (tid == 0) cpc_tile_partial(a, pos_loss, pos_correct, tile, n, k);

    // ---- 4. g replaces f, pair by pair (a pair's thread touches its own element only)
    for (int p = tid; p < J * CPC_TT; p += 256) {
        const int j = p >> 4, tl = p & 15;
        const float pj = expf(sc[j][tl] - pos_m[tl]) / pos_e[tl];
        const float g = (j == 0 ? pj - 1.f : pj) / ga.count;
        sc[j][tl] = g;
        if (ga.g && t0 + tl < L) ga.g[(((size_t)(k - 1) * N + n) * J + j) * L + t0 + tl] = g;
    }
    __syncthreads();

    // ---- 5. dWc: thread (anchor tid >> 4, features 4 (tid & 15) .. + 3), one chain over j
    {
        const int tl = tid >> 4, d4 = tid & 15;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < J; ++j) {
            const float g = sc[j][tl];
            const float4 zv = ((const float4 *)(a.z + (size_t)rows[j][tl] * CPC_D))[d4];
            acc.x = fmaf(g, zv.x, acc.x);
            acc.y = fmaf(g, zv.y, acc.y);
            acc.z = fmaf(g, zv.z, acc.z);
            acc.w = fmaf(g, zv.w, acc.w);
        }
        if (t0 + tl < L) {
            const size_t o = (((size_t)(k - 1) * N + n) * L + t0 + tl) * (CPC_D / 4) + d4;
            ((float4 *)ga.dWc)[o] = make_float4(acc.x * 0.125f, acc.y * 0.125f, acc.z * 0.125f, acc.w * 0.125f);
            if (ga.Wc) ((float4 *)ga.Wc)[o] = *(const float4 *)&wc[tl][4 * d4];
        }
    }
}

// part (n_steps, slabs, 64, C + 16): column C of a row is the bias partial of cpc_grad_b_kernel (C + 1 .. C + 15 pad the row).
__global__ __launch_bounds__(256) void cpc_grad_w_kernel(const float *dWc, const float *c, float *part, int N, int L, int T, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, ks = lane >> 4;
    const int ct = blockIdx.x, slab = blockIdx.y, k = blockIdx.z, S = gridDim.y;
    const int R = N * L;                                 // N L < 2^31 (the entry checks it)
    const f32x4 acc = slab_mfma_tile(R, slab * GRAD_SLAB, ks,
        [&](int r) { return dWc[((size_t)k * R + r) * CPC_D + wave * 16 + i]; },
        [&](int r) { const int n = r / L, t = r - n * L; return c[((size_t)n * T + t) * C + ct * 16 + i]; });
#pragma unroll
    for (int r = 0; r < 4; ++r)                          // row = feature 16 wave + 4 ks + r, column = ct * 16 + i
        part[(((size_t)k * S + slab) * CPC_D + wave * 16 + ks * 4 + r) * (C + 16) + ct * 16 + i] = acc[r];
}

__global__ __launch_bounds__(256) void cpc_grad_b_kernel(const float *dWc, float *part, int N, int L, int C) {
    __shared__ float red[4][CPC_D];
    const int d = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int slab = blockIdx.x, k = blockIdx.y, S = gridDim.x;
    const long long R = (long long)N * L;
    const float sum = slab_column_sum(dWc + (size_t)k * R * CPC_D + d, CPC_D, R, (long long)slab * GRAD_SLAB, rg, d, red);
    if (rg == 0) part[(((size_t)k * S + slab) * CPC_D + d) * (C + 16) + C] = sum;
}

__global__ __launch_bounds__(256) void cpc_grad_w_finish_kernel(const float *part, float *dW, float *db, int K, int S, int C) {
    const int ld = C + 16;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;           // (k, d, col), col <= C
    if (e >= (size_t)K * CPC_D * (C + 1)) return;
    const int col = (int)(e % (C + 1));
    const size_t kd = e / (C + 1);
    const int k = (int)(kd / CPC_D), d = (int)(kd % CPC_D);
    if (col < C ? dW == nullptr : db == nullptr) return;
    float sum = 0.f;
    for (int s = 0; s < S; ++s) sum += part[(((size_t)k * S + s) * CPC_D + d) * ld + col];
    if (col < C) dW[kd * C + col] = sum; else db[kd] = sum;
}

__global__ __launch_bounds__(256) void cpc_grad_c_kernel(const float *dWc, const float *W, float *dc, int K, int N, int L, int T, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, ks = lane >> 4;
    const int t0 = blockIdx.x * 16, n = blockIdx.y, c0 = (blockIdx.z * 4 + wave) * 16;
    const int t = t0 + i;
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
    if (t0 < L) {
        for (int k = 0; k < K; ++k) {
            const float4 *ap = (const float4 *)(dWc + (((size_t)k * N + n) * L + min(t, L - 1)) * CPC_D) + ks;
            const float *wp = W + ((size_t)k * CPC_D + 4 * ks) * C + c0 + i;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float4 av = ap[4 * s];
                if (t >= L) av = make_float4(0.f, 0.f, 0.f, 0.f);
                const float *w = wp + (size_t)16 * s * C;
                mfma_k4(a0, a1, av, make_float4(w[0], w[C], w[2 * (size_t)C], w[3 * (size_t)C]));
            }
        }
    }
    const f32x4 acc = a0 + a1;                           // row = anchor t0 + 4 ks + r, column = c0 + i
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int to = t0 + 4 * ks + r;
        if (to < T) dc[((size_t)n * T + to) * C + c0 + i] = to < L ? acc[r] : 0.f;
    }
}

__global__ __launch_bounds__(256) void cpc_grad_z_kernel(const float *Wc, const float *g, const int *u_in, const int *s_in, float *dzk,
                                                         int Utt, int Neg, int L) {
    __shared__ float acc[GZ_ROWS][CPC_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nd = blockIdx.y, k = blockIdx.z, N = gridDim.y, J = 1 + Neg;
    const int spk = nd / Utt, ud = nd - spk * Utt;
    const int lo = blockIdx.x * GZ_ROWS + 16 * wave;     // this wave's destination positions lo .. lo + 15
    for (int r = 0; r < 16; ++r) {                       // the positive: anchor (nd, s) itself
        const int s = lo + r;
        float v = 0.f;
        if (s < L) v = g[(((size_t)k * N + nd) * J) * L + s] * Wc[(((size_t)k * N + nd) * L + s) * CPC_D + lane];
        acc[16 * wave + r][lane] = v;
    }
    for (int utt = 0; utt < Utt; ++utt) {
        const int n = spk * Utt + utt;
        for (int j = 1; j <= Neg; ++j) {
            if (u_in[((size_t)k * Utt + utt) * Neg + j - 1] != ud) continue;
            const int *sp = s_in + (((size_t)k * N + n) * Neg + j - 1) * L;
            const float *gp = g + (((size_t)k * N + n) * J + j) * L;
            const float *wp = Wc + (((size_t)k * N + n) * L) * CPC_D + lane;
            for (int tc = 0; tc < L; tc += 64) {
                const int s = tc + lane < L ? sp[tc + lane] : -1;
                for (unsigned long long hits = __ballot(s >= lo && s < lo + 16); hits;) {
                    int sb[GZ_FLIGHT];
                    float gv[GZ_FLIGHT], wv[GZ_FLIGHT];
                    bool live[GZ_FLIGHT];
#pragma unroll
                    for (int q = 0; q < GZ_FLIGHT; ++q) {            // the next anchors in t order, their loads in flight together
                        live[q] = hits != 0;
                        const int b = live[q] ? __builtin_ctzll(hits) : 0;       // a dead slot re-reads anchor tc and adds nothing
                        hits &= hits - 1;
                        sb[q] = __shfl(s, b);
                        gv[q] = gp[tc + b];
                        wv[q] = wp[(size_t)(tc + b) * CPC_D];
                    }
#pragma unroll
                    for (int q = 0; q < GZ_FLIGHT; ++q) {            // added one after the other, in that order
                        if (!live[q]) continue;
                        float *dst = &acc[sb[q] - lo + 16 * wave][lane];
                        *dst = fmaf(gv[q], wv[q], *dst);
                    }
                }
            }
        }
    }
    for (int r = 0; r < 16; ++r) {
        const int s = lo + r;
        if (s < L) dzk[(((size_t)k * N + nd) * L + s) * CPC_D + lane] = acc[16 * wave + r][lane] * 0.125f;
    }
}

__global__ __launch_bounds__(256) void cpc_grad_z_sum_kernel(const float *dzk, float *dz, int K, int N, int L, int T) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;           // (n, tau, d)
    if (e >= (size_t)N * T * CPC_D) return;
    const int d = (int)(e % CPC_D);
    const size_t nt = e / CPC_D;
    const int n = (int)(nt / T), tau = (int)(nt % T);
    float sum = 0.f;
    for (int k = 1; k <= K; ++k) {
        const int s = tau - k;
        if (s >= 0 && s < L) sum += dzk[((((size_t)(k - 1)) * N + n) * L + s) * CPC_D + d];
    }
    dz[e] = sum;
}

}  // namespace

extern "C" int vqcpc_cpc_grad(vqcpc_cpc *cpc, const float *z, const float *c, int T, const float *W, const float *bias,
                              const int64_t *utt_index, const int64_t *seq_index, uint64_t seed, uint32_t stream_id, float *loss,
                              float *step_loss, float *accuracy, float *grad_z, float *grad_c, float *grad_W, float *grad_bias,
                              void *stream) {
    VQ_REQUIRE(cpc && z && c && loss && step_loss && accuracy, "vqcpc_cpc_grad: null argument");
    VQ_REQUIRE((W == nullptr) == (bias == nullptr), "vqcpc_cpc_grad: give W and bias together, or neither (the handle's copies)");
    CpcGradArgs ga;
    CpcArgs &a = ga.f;
    size_t P = 0;
    TRY(cpc_begin(cpc, "vqcpc_cpc_grad", z, c, T, W, bias, utt_index, seq_index, seed, stream_id, a, P));
    const int K = cpc->n_steps, L = a.L, N = a.Spk * a.Utt, C = a.C, J = 1 + a.Neg, tiles = a.tiles;
    VQ_REQUIRE((long long)N * T < (1ll << 31), "vqcpc_cpc_grad: Spk * Utt * T = %lld rows do not fit a 32-bit row index", (long long)N * T);
    const int slabs = (int)(((long long)N * L + GRAD_SLAB - 1) / GRAD_SLAB);
    VQ_REQUIRE(slabs <= 65535, "vqcpc_cpc_grad: Spk * Utt * L = %lld rows, more than 65535 slabs of %d", (long long)N * L, GRAD_SLAB);
    const bool want_w = grad_W || grad_bias;
    // work space: dWc | Wc, g, s, u, dz partials (grad_z) | dW slab partials (grad_W, grad_bias)
    const size_t b_rows = up256((size_t)K * N * L * CPC_D * sizeof(float)), b_g = up256((size_t)K * N * J * L * sizeof(float));
    const size_t b_s = up256((size_t)K * N * cpc->Neg * L * sizeof(int)), b_u = up256((size_t)K * cpc->Utt * cpc->Neg * sizeof(int));
    const size_t b_part = up256((size_t)K * slabs * CPC_D * (C + 16) * sizeof(float));
    TRY(cpc->grad_work.reserve(b_rows + (grad_z ? 2 * b_rows + b_g + b_s + b_u : 0) + (want_w ? b_part : 0)));
    char *w = cpc->grad_work.as<char>();
    float *dWc = (float *)w; w += b_rows;
    float *Wc = nullptr, *g = nullptr, *dzk = nullptr, *part = nullptr;
    int *s_buf = nullptr, *u_buf = nullptr;
    if (grad_z) {
        Wc = (float *)w; w += b_rows;
        dzk = (float *)w; w += b_rows;
        g = (float *)w; w += b_g;
        s_buf = (int *)w; w += b_s;
        u_buf = (int *)w; w += b_u;
    }
    if (want_w) part = (float *)w;
    ga.dWc = dWc; ga.Wc = Wc; ga.g = g; ga.u_out = u_buf; ga.s_out = s_buf;
    ga.count = (float)((double)K * N * L);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cpc_grad_tile_kernel, dim3(tiles, N, K), dim3(256), 0, s, ga);
    hipLaunchKernelGGL(cpc_finish_kernel, dim3(1), dim3(256), 0, s, a.part_loss, a.part_correct, K, (int)P, N * L, loss, step_loss,
                       accuracy);
    if (want_w) {
        if (grad_W) hipLaunchKernelGGL(cpc_grad_w_kernel, dim3(C / 16, slabs, K), dim3(256), 0, s, dWc, c, part, N, L, T, C);
        if (grad_bias) hipLaunchKernelGGL(cpc_grad_b_kernel, dim3(slabs, K), dim3(256), 0, s, dWc, part, N, L, C);
        const size_t outs = (size_t)K * CPC_D * (C + 1);
        hipLaunchKernelGGL(cpc_grad_w_finish_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, part, grad_W, grad_bias, K,
                           slabs, C);
    }
    if (grad_c)
        hipLaunchKernelGGL(cpc_grad_c_kernel, dim3((T + 15) / 16, N, C / 64), dim3(256), 0, s, dWc, a.W, grad_c, K, N, L, T, C);
    if (grad_z) {
        hipLaunchKernelGGL(cpc_grad_z_kernel, dim3((L + GZ_ROWS - 1) / GZ_ROWS, N, K), dim3(256), 0, s, Wc, g, u_buf, s_buf, dzk, cpc->Utt,
                           cpc->Neg, L);
        const size_t outs = (size_t)N * T * CPC_D;
        hipLaunchKernelGGL(cpc_grad_z_sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, s, dzk, grad_z, K, N, L, T);
    }
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
