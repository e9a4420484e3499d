// codebook.hip -- codebook adaptation: the EMA update of VQEmbeddingEMA.forward in training mode (model.py:136-145), after the
// eval-branch kernels of encoder.hip have produced the indices, the histogram, the loss and the perplexity from the OLD codebook.
// Two launches; every step is a separately rounded fp32 operation (-ffp-contract=off), divisions are IEEE.
//   ema_prep_kernel    indices narrowed to 16 bits (n_emb <= 4096); count = decay * ema_count + omd * hist into work space, so that
//                      the update below may overwrite ema_count while other workgroups still sum the counts.
//   ema_update_kernel  one workgroup per code, lane = dimension: n = sum(count) in the fixed order, the Laplace-smoothed count, the
//                      per-code row sum dw in the chunk-tree order (eight waves, an eighth of the chunks each), ema_weight and
//                      embedding.  No float atomics, no one-hot, no per-chunk array in memory; no workgroup waits for another.
#include "encoder_internal.h"

__global__ __launch_bounds__(256) void ema_prep_kernel(const int64_t *__restrict__ idx, int n_rows, const unsigned *__restrict__ hist,
                                                       const float *__restrict__ ema_count, int n_emb, float decay, float omd,
                                                       uint16_t *__restrict__ idx16, float *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_rows) idx16[i] = (uint16_t)idx[i];
    if (i < n_emb) {
        const float a = decay * ema_count[i], b = omd * (float)hist[i];        // hist <= 2^24: exact in fp32
        cnt[i] = a + b;
    }
}

// Chunk partials are combined by the adjacent-pair tree -- (0+1), (2+3), ..., an odd last one carried up, until one remains.  A
// carried-up partial equals that partial plus an exact zero, so the tree equals, value for value, the full binary tree over the
// chunk indices padded with empty chunks to a power of two.  One workgroup per code splits that tree among its eight waves: wave w
// owns the aligned block of S chunks from w * S (S a power of two, 8 S >= chunks), i.e. one subtree three levels below the root,
// and sums it with a binary counter -- after chunk c the partial of every complete, not yet paired aligned block of 2^l chunks
// sits in st[l] -- and the root is ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)).  2^24 rows = 2^18 chunks: 19 levels.
// A code that owns most rows is the critical path (one workgroup gathers them all): eight waves with 16 row loads in flight each.
#define EMA_LEVELS 19
#define EMA_UNROLL 8                      // chunks whose index loads are in flight together
#define EMA_ROWS 16                       // row loads in flight
#define EMA_WAVES 8

__global__ __launch_bounds__(64 * EMA_WAVES) void ema_update_kernel(EmaP p) {
    __shared__ float part8[EMA_WAVES][64];
    __shared__ float total;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = blockIdx.x;
    const int nchunks = (p.n_rows + 63) / 64;
    int S = 1;
    while (EMA_WAVES * S < nchunks) S *= 2;
    const int first = w * S, mine = min(S, nchunks - first);         // wave-uniform; mine <= 0: nothing, an exact zero

    if (w == EMA_WAVES - 1) {                                        // its block is the ragged end: it also sums the counts
        // n = sum(count): part[l] = count[l] + count[64 + l] + ... in sequence, then the upper half onto the lower, 32, 16, ... 1
        float part = p.cnt[lane];
        for (int j = 1; j < p.n_emb / 64; ++j) part = part + p.cnt[64 * j + lane];
#pragma unroll
        for (int h = 32; h > 0; h >>= 1) part = part + __shfl_down(part, h, 64);
        if (lane == 0) total = part;
    }

    // this wave's share of dw[m][lane]: rows of a chunk in ascending order, chunks by the counter
    float st[EMA_LEVELS];
#pragma unroll
    for (int l = 0; l < EMA_LEVELS; ++l) st[l] = 0.f;
    for (int c0 = 0; c0 < mine; c0 += EMA_UNROLL) {
        int code[EMA_UNROLL];
#pragma unroll
        for (int k = 0; k < EMA_UNROLL; ++k) {
            const int r = (first + c0 + k) * 64 + lane;
            code[k] = (c0 + k < mine && r < p.n_rows) ? (int)p.idx16[r] : 0xFFFF;     // 0xFFFF: no code (n_emb <= 4096)
        }
#pragma unroll
        for (int k = 0; k < EMA_UNROLL; ++k) {
            const int c = c0 + k;                                    // chunk index inside this wave's block
            if (c >= mine) break;
            unsigned long long mask = __builtin_amdgcn_ballot_w64(code[k] == m);
            const float *rows = p.x + (size_t)(first + c) * 64 * 64 + lane;
            float acc = 0.f;
            while (mask) {                                           // EMA_ROWS row loads in flight, added in ascending row order
                int r[EMA_ROWS]; bool v[EMA_ROWS]; float t[EMA_ROWS];
#pragma unroll
                for (int q = 0; q < EMA_ROWS; ++q) {
                    v[q] = mask != 0;
                    r[q] = v[q] ? __builtin_ctzll(mask) : 0;
                    mask &= mask - 1;
                }
#pragma unroll
                for (int q = 0; q < EMA_ROWS; ++q) t[q] = v[q] ? rows[(size_t)r[q] * 64] : 0.f;
#pragma unroll
                for (int q = 0; q < EMA_ROWS; ++q) if (v[q]) acc = acc + t[q];
            }
            bool placed = false;                                     // push chunk c: carry while bit l of c is set
#pragma unroll
            for (int l = 0; l < EMA_LEVELS; ++l) {
                if (!placed) {
                    if ((c >> l) & 1) acc = st[l] + acc;
                    else { st[l] = acc; placed = true; }
                }
            }
        }
    }
    float sum = 0.f;                                                 // what is left: lowest level first, each older block on the left
    bool have = false;
#pragma unroll
    for (int l = 0; l < EMA_LEVELS; ++l) {
        if (mine > 0 && ((mine >> l) & 1)) { sum = have ? st[l] + sum : st[l]; have = true; }
    }
    part8[w][lane] = sum;
    __syncthreads();
    if (w != 0) return;

    const float lo = (part8[0][lane] + part8[1][lane]) + (part8[2][lane] + part8[3][lane]);
    const float hi = (part8[4][lane] + part8[5][lane]) + (part8[6][lane] + part8[7][lane]);
    const float dw = lo + hi;
    const float n = total;
    const float count = (p.cnt[m] + p.eps) / (n + p.meps) * n;
    const size_t o = (size_t)m * 64 + lane;
    const float a = p.decay * p.ema_weight[o], b = p.omd * dw;
    const float wgt = a + b;
    const float e = wgt / count;
    p.ema_weight[o] = wgt;
    p.embedding[o] = e;
    p.codebook[o] = e;
    if (lane == 0) p.ema_count[m] = count;
}

void launch_ema_prep(const int64_t *idx, int n_rows, const unsigned *hist, const float *ema_count, int n_emb, float decay, float omd,
                     uint16_t *idx16, float *cnt, hipStream_t s) {
    const int n = n_rows > n_emb ? n_rows : n_emb;
    hipLaunchKernelGGL(ema_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, s, idx, n_rows, hist, ema_count, n_emb, decay, omd, idx16, cnt);
}
void launch_ema_update(const EmaP &p, hipStream_t s) {
    hipLaunchKernelGGL(ema_update_kernel, dim3(p.n_emb), dim3(64 * EMA_WAVES), 0, s, p);
}
