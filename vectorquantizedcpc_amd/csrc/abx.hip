// ABX scoring of encoded units (own protocol): stands in for the outside "ABX evaluation script" that the
// reference's README 4-B runs on the text files of encode.py:48-52.  One call = three launches, nothing synchronises.
//
// abx_normalise_kernel, one wave per frame: sum of squares in a fixed order (lane q takes the 16-byte pieces q and q + 64 as
//   one fma chain, then a 6-step xor butterfly), every component times 1 / sqrt(sum) into the work copy `fn`.  A zero frame
//   stays zero.
// abx_dtw_kernel, 256 threads: a workgroup owns ONE X token and ABX_AT = 4 consecutive A tokens of one block.
//   Frame distance d = 2 atan2(|u - v|, |u + v|) / pi on the normalised frames: no arccos of a dot product near 1, bit-equal
//   frames give exactly 0, a zero frame gives 0.5 against a non-zero one and 0 against a zero one.
//   1. pair after pair, all 256 threads fill the pair's Ta x Tb distance tile: the cells are dealt out as c = tid + 256 r
//      (r < 16), so short tokens fill the workgroup; every cell keeps its two sums |u - v|^2, |u + v|^2 in registers across
//      chunks of ABX_DC = 32 components.  The X token's chunk is staged in LDS (T_MAX x D never has to fit whole); the A rows
//      come from L1 / L2, where the Tb threads of one row read the same 16 bytes.  Within a chunk four chains per sum
//      (component mod 4), combined (s0 + s1) + (s2 + s3) and added to the cell's running sum: a fixed order, so equal inputs
//      give equal bits.
//   2. d goes to the pair's 64 x 64 LDS tile (row stride 64: a diagonal's reads fall on different banks).
//   3. one wave per pair: DTW by anti-diagonals, lane i = row i:  C[i][j] = d[i][j] + min(C[i-1][j-1], C[i-1][j], C[i][j-1]),
//      the predecessor the FIRST minimum in that order, L[i][j] = L[pred] + 1, L[0][0] = 1.  One shuffle of (C, L) per
//      diagonal; at most Ta + Tb - 1 <= 127 steps.  Lane Ta - 1 stores cost, path length and cost / length.
//   No atomics; no loop's trip count depends on anything but D, the block count and the (clamped) token lengths.
// abx_count_kernel, one thread per output (block, x, q):  twice_wins = sum over a in x's own phone segment (a's token != x's
//   token), b in segment q of 2 [D(a, x) < D(b, x)] + [D(a, x) == D(b, x)], 0 for q = x's own segment.  Integers, plain stores.
//
// The index form (frames given as codebook indices: every frame distance of a call is one of M x M values):
// abx_code_table_kernel, one thread per cell of the (M, M) table: the distance between codebook rows i and j, by the same
//   abx_chunk_sums / abx_angle the DTW kernel's fill runs, chunk after chunk of ABX_DC components: the same sums in the same
//   order, so table[i][j] has the bits the fill gives an A frame equal to row i and an X frame equal to row j.
// abx_index_dtw_kernel, the same workgroup <-> (block, x, A tile) mapping: wave w owns pair w from start to end, no LDS, no
//   barrier, no D loop.  Lane i = row i holds code_a[i] * M and code_x[i]; on diagonal k it takes code_x[k - i] by one shuffle
//   and gathers d[i][k - i] = table[code_a[i] * M + code_x[k - i]] straight into the DTW kernel's own step (abx_front_step),
//   ABX_G diagonals ahead of the step that uses it.  26 VGPRs and no LDS: 8 workgroups per CU hide the gathers' latency.
// abx_edit_kernel, same mapping, no table and no LDS: Levenshtein distance of the two index runs on the same anti-diagonal
//   wavefront in integers, E(i, 0) = i, E(0, j) = j; cost = E(Ta, Tb), path length = max(Ta, Tb).
//
// Every index that comes from the caller's device tables is clamped before it is used as an address and every store is
// guarded by the output's size: a bad table cannot read or write out of bounds (the Python wrapper rejects it first).  Codes
// are clamped into [0, M).
#include "common.h"

namespace {

constexpr int ABX_TMAX = 64;         // frames per token
constexpr int ABX_AT = 4;            // A tokens (= waves) per workgroup
constexpr int ABX_DC = 32;           // components per chunk
constexpr int ABX_XS = ABX_DC + 4;   // LDS row stride of the X chunk: 16-byte reads of neighbouring rows on different bank quads
constexpr int ABX_R = ABX_TMAX * ABX_TMAX / 256;   // cells per thread of a 64 x 64 pair
constexpr int ABX_BW = 12;           // ints per block-table row (vqcpc.h)
constexpr int ABX_G = 4;             // diagonals whose table gathers the index kernel keeps in flight

struct AbxArgs {
    const float *fn;                 // normalised frames (n_frames, D); the index form: NULL
    const float *table;              // the index form: (M, M) frame distances between codebook rows (NULL: edit metric)
    const int *codes;                // the index form: (n_frames) codebook indices
    const int *tokens, *lists, *segs, *blocks;
    float *cost, *dist;
    int *path_len, *twice_wins;
    int n_frames, D, M, n_tokens, n_lists, n_segs, n_blocks;
    long long n_dist, n_out;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void abx_normalise_kernel(const float *__restrict__ f, float *__restrict__ fn, int n_frames, int D) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_frames) return;
    const int nq = D >> 2;
    const float4 *p = (const float4 *)(f + (size_t)row * D);
    float4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
    if (lane < nq) v0 = p[lane];
    if (lane + 64 < nq) v1 = p[lane + 64];
    float s = v0.x * v0.x;
    s = fmaf(v0.y, v0.y, s); s = fmaf(v0.z, v0.z, s); s = fmaf(v0.w, v0.w, s);
    s = fmaf(v1.x, v1.x, s); s = fmaf(v1.y, v1.y, s); s = fmaf(v1.z, v1.z, s); s = fmaf(v1.w, v1.w, s);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    const float inv = s > 0.f ? 1.0f / sqrtf(s) : 0.f;
    float4 *o = (float4 *)(fn + (size_t)row * D);
    if (lane < nq) o[lane] = make_float4(v0.x * inv, v0.y * inv, v0.z * inv, v0.w * inv);
    if (lane + 64 < nq) o[lane + 64] = make_float4(v1.x * inv, v1.y * inv, v1.z * inv, v1.w * inv);
}

// largest b with blocks[b][col] <= id (the column ascends); 0 when there is none.  At most 32 steps whatever the table holds.
__device__ __forceinline__ int abx_find_block(const int *blocks, int n_blocks, int col, long long id) {
    int lo = 0, hi = n_blocks;
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = (lo + hi) >> 1;
        if ((long long)blocks[(size_t)mid * ABX_BW + col] <= id) lo = mid; else hi = mid;
    }
    return lo;
}

// (first row, frames) of entry `at` of the token-id lists, both clamped into the frame table
__device__ __forceinline__ void abx_token(const AbxArgs &a, int at, int &tok, int &row, int &len) {
    tok = clampi(a.lists[clampi(at, 0, a.n_lists - 1)], 0, a.n_tokens - 1);
    row = clampi(a.tokens[2 * tok], 0, a.n_frames - 1);
    len = clampi(a.tokens[2 * tok + 1], 1, min(ABX_TMAX, a.n_frames - row));
}

// the workgroup's block row, its X token `x` and first A token `a0`; false (for the whole workgroup) when it has no work
__device__ __forceinline__ bool abx_workgroup(const AbxArgs &a, const int *&blk, int &nA, int &nX, int &x, int &a0) {
    const int b = abx_find_block(a.blocks, a.n_blocks, 9, (long long)blockIdx.x);
    blk = a.blocks + (size_t)b * ABX_BW;
    nA = max(blk[1], 0); nX = max(blk[3], 0);
    const int tiles = (nA + ABX_AT - 1) / ABX_AT;
    const int local = (int)blockIdx.x - blk[9];
    if (tiles == 0 || local < 0 || local / tiles >= nX) return false;
    x = local / tiles; a0 = (local - x * tiles) * ABX_AT;
    return true;
}

// one chunk of `dq` 16-byte pieces of an A frame `ap` and an X frame `xp`: four chains per sum (component mod 4), combined
// (s0 + s1) + (s2 + s3) and added to the running |u - v|^2 and |u + v|^2.  The ONE statement of the order of these sums.
__device__ __forceinline__ void abx_chunk_sums(const float4 *ap, const float4 *xp, int dq, float &sd, float &ss) {
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 4
    for (int q = 0; q < dq; ++q) {
        const float4 u = ap[q], v = xp[q];
        const float mx = u.x - v.x, my = u.y - v.y, mz = u.z - v.z, mw = u.w - v.w;
        const float px = u.x + v.x, py = u.y + v.y, pz = u.z + v.z, pw = u.w + v.w;
        d0 = fmaf(mx, mx, d0); d1 = fmaf(my, my, d1); d2 = fmaf(mz, mz, d2); d3 = fmaf(mw, mw, d3);
        s0 = fmaf(px, px, s0); s1 = fmaf(py, py, s1); s2 = fmaf(pz, pz, s2); s3 = fmaf(pw, pw, s3);
    }
    sd += (d0 + d1) + (d2 + d3);
    ss += (s0 + s1) + (s2 + s3);
}

__device__ __forceinline__ float abx_angle(float sd, float ss) {
    return (2.0f * atan2f(sqrtf(sd), sqrtf(ss))) * 0.318309886183790672f;
}

// cell c of a Ta x Tb tile -> (i, j) = (c / Tb, c % Tb), inv_tb = 1 / Tb: the quotient is >= 0.5 / 64 from an integer
__device__ __forceinline__ void abx_cell(int c, int Tb, float inv_tb, int &i, int &j) {
    i = (int)(((float)c + 0.5f) * inv_tb);
    j = c - i * Tb;
}

// DTW of one pair by one wave, lane i = row i: anti-diagonal k holds the cells i + j = k; lane i keeps its own last value (the
// left neighbour C[i][j-1]) and receives lane i - 1's last value (C[i-1][j]); the diagonal neighbour C[i-1][j-1] is what it
// received one step earlier.  After the last diagonal lane Ta - 1 holds the pair's cost `c1` and path length `l1`.
struct AbxFront {
    float c1 = __builtin_inff(), up_prev = __builtin_inff();
    int l1 = 0, upl_prev = 0;
};

__device__ __forceinline__ bool abx_on_diagonal(int lane, int k, int Ta, int Tb) { return lane < Ta && k - lane >= 0 && k - lane < Tb; }

// diagonal k: `d(j)` gives this lane's frame distance d[lane][j], j = k - lane, and is asked only where the lane has a cell on
// the diagonal; every lane of the wave calls the step
template <class F>
__device__ __forceinline__ void abx_front_step(AbxFront &f, int lane, int k, int Ta, int Tb, F d) {
    const float INF = __builtin_inff();
    float up = __shfl_up(f.c1, 1);
    int upl = __shfl_up(f.l1, 1);
    if (lane == 0) { up = INF; upl = 0; }
    const int j = k - lane;
    float cn = INF;
    int ln = 0;
    if (lane < Ta && j >= 0 && j < Tb) {
        float best = f.up_prev;
        int bl = f.upl_prev;
        if (up < best) { best = up; bl = upl; }
        if (f.c1 < best) { best = f.c1; bl = f.l1; }
        if (k == 0) { best = 0.f; bl = 0; }
        cn = d(j) + best;
        ln = bl + 1;
    }
    f.up_prev = up; f.upl_prev = upl;
    f.c1 = cn; f.l1 = ln;
}

// pair (ai, x) of block `blk`: cost, path length and cost / length into the block's (nA, nX) tables
__device__ __forceinline__ void abx_store_pair(const AbxArgs &a, const int *blk, int ai, int nX, int x, float c, int l) {
    const long long o = (long long)blk[6] + (long long)ai * nX + x;
    if (blk[6] >= 0 && o < a.n_dist) {
        if (a.cost) a.cost[o] = c;
        if (a.path_len) a.path_len[o] = l;
        a.dist[o] = c / (float)l;
    }
}

__global__ __launch_bounds__(256) void abx_dtw_kernel(AbxArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[ABX_TMAX][ABX_XS];
    __shared__ float dt[ABX_AT][ABX_TMAX * ABX_TMAX];
    // 74 752 bytes: more than the 64 KB of earlier architectures, two workgroups in the 160 KB of a gfx950 CU (the entry point
    // refuses any other device)
    static_assert(sizeof(float) * (ABX_TMAX * ABX_XS + ABX_AT * ABX_TMAX * ABX_TMAX) <= 80 * 1024, "two workgroups per CU");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *blk;
    int nA, nX, x, a0;
    if (!abx_workgroup(a, blk, nA, nX, x, a0)) return;                   // the whole workgroup: before any barrier
    const int D = a.D;
    int tok, rowx, Tb;
    abx_token(a, blk[2] + x, tok, rowx, Tb);
    const float inv_tb = 1.0f / (float)Tb;

    // ---- 1, 2. the distance tiles of the workgroup's pairs, one after the other, all 256 threads on each
    for (int p = 0; p < ABX_AT && a0 + p < nA; ++p) {
        int rowa, Ta;
        abx_token(a, blk[0] + a0 + p, tok, rowa, Ta);
        const int ncell = Ta * Tb, nr = (ncell + 255) >> 8;
        float sd[ABX_R], ss[ABX_R];
#pragma unroll
        for (int r = 0; r < ABX_R; ++r) { sd[r] = 0.f; ss[r] = 0.f; }
        for (int c0 = 0; c0 < D; c0 += ABX_DC) {
            const int dq = min(ABX_DC, D - c0) >> 2;                     // 16-byte pieces of this chunk (D % 4 == 0)
            __syncthreads();
            for (int e = tid; e < Tb * (ABX_DC / 4); e += 256) {
                const int j = e >> 3, q = e & 7;
                if (q < dq) *(float4 *)&xs[j][4 * q] = *(const float4 *)(a.fn + (size_t)(rowx + j) * D + c0 + 4 * q);
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < ABX_R; ++r) {
                if (r < nr) {
                    int i, j;
                    abx_cell(min(tid + 256 * r, ncell - 1), Tb, inv_tb, i, j);      // a thread past the last cell repeats it and stores nothing
                    abx_chunk_sums((const float4 *)(a.fn + (size_t)(rowa + i) * D + c0), (const float4 *)&xs[j][0], dq, sd[r], ss[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < ABX_R; ++r) {
            const int c = tid + 256 * r;
            if (c < ncell) {
                int i, j;
                abx_cell(c, Tb, inv_tb, i, j);
                dt[p][i * ABX_TMAX + j] = abx_angle(sd[r], ss[r]);
            }
        }
    }
    __syncthreads();

    // ---- 3. one wave per pair
    const int ai = a0 + wave;
    if (ai >= nA) return;
    int rowa, Ta;
    abx_token(a, blk[0] + ai, tok, rowa, Ta);
    const float *dw = dt[wave];
    AbxFront f;
    for (int k = 0; k < Ta + Tb - 1; ++k) abx_front_step(f, lane, k, Ta, Tb, [&](int j) { return dw[lane * ABX_TMAX + j]; });
    if (lane == Ta - 1) abx_store_pair(a, blk, ai, nX, x, f.c1, f.l1);
}

// ---- the index form
__global__ __launch_bounds__(256) void abx_code_table_kernel(const float *__restrict__ bn, float *__restrict__ table, int M, int D) {
    const int c = blockIdx.x * 256 + threadIdx.x;                        // M <= 4096: M * M fits
    if (c >= M * M) return;
    const int i = c / M, j = c - i * M;
    float sd = 0.f, ss = 0.f;
    for (int c0 = 0; c0 < D; c0 += ABX_DC)
        abx_chunk_sums((const float4 *)(bn + (size_t)i * D + c0), (const float4 *)(bn + (size_t)j * D + c0), min(ABX_DC, D - c0) >> 2, sd, ss);
    table[c] = abx_angle(sd, ss);
}

// the codes of a token's frames, lane l the one of frame l (a lane past the token repeats a row of the table), clamped
__device__ __forceinline__ int abx_code(const AbxArgs &a, int row, int lane) {
    return clampi(a.codes[min(row + lane, a.n_frames - 1)], 0, a.M - 1);
}

__global__ __launch_bounds__(256) void abx_index_dtw_kernel(AbxArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int *blk;
    int nA, nX, x, a0;
    if (!abx_workgroup(a, blk, nA, nX, x, a0)) return;                   // the whole workgroup
    const int ai = a0 + wave;
    if (ai >= nA) return;                                                // the whole wave; the kernel has no barrier
    int tok, rowx, Tb, rowa, Ta;
    abx_token(a, blk[2] + x, tok, rowx, Tb);
    abx_token(a, blk[0] + ai, tok, rowa, Ta);
    const int cx = abx_code(a, rowx, lane), ca = abx_code(a, rowa, lane) * a.M;
    const int steps = Ta + Tb - 1;
    // this lane's cell of diagonal k: the X code comes from lane k - lane by a shuffle that every lane runs
    auto gather = [&](int k) -> float {
        const int xj = __shfl(cx, clampi(k - lane, 0, ABX_TMAX - 1));
        return abx_on_diagonal(lane, k, Ta, Tb) ? a.table[ca + xj] : 0.f;
    };
    float d[ABX_G];                                                      // the cells of the next ABX_G diagonals, in flight
#pragma unroll
    for (int g = 0; g < ABX_G; ++g) d[g] = gather(g);
    AbxFront f;
    for (int k0 = 0; k0 < steps; k0 += ABX_G) {
#pragma unroll
        for (int g = 0; g < ABX_G; ++g) {
            const int k = k0 + g;
            if (k < steps) {                                             // the same in every lane
                const float dk = d[g];
                d[g] = gather(k + ABX_G);                                // past the last diagonal no lane loads
                abx_front_step(f, lane, k, Ta, Tb, [&](int) { return dk; });
            }
        }
    }
    if (lane == Ta - 1) abx_store_pair(a, blk, ai, nX, x, f.c1, f.l1);
}

__global__ __launch_bounds__(256) void abx_edit_kernel(AbxArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int *blk;
    int nA, nX, x, a0;
    if (!abx_workgroup(a, blk, nA, nX, x, a0)) return;
    const int ai = a0 + wave;
    if (ai >= nA) return;
    int tok, rowx, Tb, rowa, Ta;
    abx_token(a, blk[2] + x, tok, rowx, Tb);
    abx_token(a, blk[0] + ai, tok, rowa, Ta);
    const int cx = abx_code(a, rowx, lane), ca = abx_code(a, rowa, lane);
    // lane i = row i + 1 of E; before its first cell a lane's own value is E(i + 1, 0) = i + 1, which is also what lane i + 1
    // receives as its first diagonal neighbour; lane 0 receives row 0: E(0, j + 1) = k + 1 from above, E(0, j) = k diagonally
    int e1 = lane + 1, up_prev = 0;
    for (int k = 0; k < Ta + Tb - 1; ++k) {
        int up = __shfl_up(e1, 1);
        if (lane == 0) up = k + 1;
        const int j = k - lane;
        const int xj = __shfl(cx, clampi(j, 0, ABX_TMAX - 1));
        if (lane < Ta && j >= 0 && j < Tb) e1 = min(up_prev + (ca != xj ? 1 : 0), min(up, e1) + 1);
        up_prev = up;
    }
    if (lane == Ta - 1) abx_store_pair(a, blk, ai, nX, x, (float)e1, max(Ta, Tb));
}

__global__ __launch_bounds__(64) void abx_count_kernel(AbxArgs a) {
    const long long id = (long long)blockIdx.x * 64 + threadIdx.x;
    if (id >= a.n_out) return;
    const int b = abx_find_block(a.blocks, a.n_blocks, 7, id);
    const int *blk = a.blocks + (size_t)b * ABX_BW;
    const int nA = max(blk[1], 0), nX = max(blk[3], 0), nS = max(blk[5], 0);
    const long long local = id - blk[7];
    if (nS == 0 || local < 0 || local >= (long long)nX * nS) return;
    const int x = (int)(local / nS), q = (int)(local - (long long)x * nS);
    const int p = clampi(a.lists[clampi(blk[8] + x, 0, a.n_lists - 1)], 0, nS - 1);
    int twice = 0;
    if (q != p && blk[6] >= 0 && nS + 1 <= a.n_segs) {
        const int *sg = a.segs + clampi(blk[4], 0, a.n_segs - nS - 1);
        const int pa = clampi(sg[p], 0, nA), pe = clampi(sg[p + 1], pa, nA);
        const int qa = clampi(sg[q], 0, nA), qe = clampi(sg[q + 1], qa, nA);
        const int tokx = a.lists[clampi(blk[2] + x, 0, a.n_lists - 1)];
        const long long base = (long long)blk[6] + x;
        if (base + (long long)(nA - 1) * nX < a.n_dist) {
            for (int ia = pa; ia < pe; ++ia) {
                if (a.lists[clampi(blk[0] + ia, 0, a.n_lists - 1)] == tokx) continue;       // a token is never its own A
                const float da = a.dist[base + (long long)ia * nX];
                for (int ib = qa; ib < qe; ++ib) {
                    const float db = a.dist[base + (long long)ib * nX];
                    twice += da < db ? 2 : (da == db ? 1 : 0);
                }
            }
        }
    }
    a.twice_wins[id] = twice;
}

}  // namespace

extern "C" int vqcpc_abx_workspace_bytes(int n_frames, int D, uint64_t *bytes) {
    VQ_REQUIRE(bytes, "vqcpc_abx_workspace_bytes: null argument");
    VQ_REQUIRE(n_frames >= 1, "vqcpc_abx_workspace_bytes: n_frames = %d, need at least 1", n_frames);
    VQ_REQUIRE(D >= 4 && D <= 512 && D % 4 == 0, "vqcpc_abx_workspace_bytes: D = %d, need a multiple of 4 in [4, 512]", D);
    *bytes = (uint64_t)n_frames * D * sizeof(float);
    return VQCPC_OK;
}

extern "C" int vqcpc_abx_score(const float *feats, int n_frames, int D, const int32_t *tokens, int n_tokens, const int32_t *lists,
                               int n_lists, const int32_t *segs, int n_segs, const int32_t *blocks, int n_blocks, int n_workgroups,
                               int64_t n_dist, int64_t n_out, void *work, float *cost, int32_t *path_len, float *dist,
                               int32_t *twice_wins, void *stream) {
    VQ_REQUIRE(feats && tokens && lists && segs && blocks && work && dist && twice_wins, "vqcpc_abx_score: null argument");
    VQ_REQUIRE(D >= 4 && D <= 512 && D % 4 == 0, "vqcpc_abx_score: D = %d, need a multiple of 4 in [4, 512]", D);
    VQ_REQUIRE(n_frames >= 1 && n_tokens >= 1 && n_lists >= 1 && n_segs >= 2 && n_blocks >= 1,
               "vqcpc_abx_score: n_frames, n_tokens, n_lists, n_blocks must be >= 1 and n_segs >= 2");
    VQ_REQUIRE(n_workgroups >= 1, "vqcpc_abx_score: n_workgroups = %d, need at least 1", n_workgroups);
    VQ_REQUIRE(n_dist >= 1 && n_dist < (1ll << 31) && n_out >= 1 && n_out < (1ll << 31),
               "vqcpc_abx_score: n_dist = %lld and n_out = %lld must be in [1, 2^31): cut the call into chunks of blocks",
               (long long)n_dist, (long long)n_out);
    VQ_REQUIRE(((uintptr_t)feats & 15) == 0 && ((uintptr_t)work & 15) == 0, "vqcpc_abx_score: feats and work must be 16-byte aligned");
    TRY(vq_require_gfx950());
    AbxArgs a;
    a.fn = (const float *)work; a.table = nullptr; a.codes = nullptr; a.M = 0;
    a.tokens = tokens; a.lists = lists; a.segs = segs; a.blocks = blocks;
    a.cost = cost; a.dist = dist; a.path_len = path_len; a.twice_wins = twice_wins;
    a.n_frames = n_frames; a.D = D; a.n_tokens = n_tokens; a.n_lists = n_lists; a.n_segs = n_segs; a.n_blocks = n_blocks;
    a.n_dist = n_dist; a.n_out = n_out;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(abx_normalise_kernel, dim3((n_frames + 3) / 4), dim3(256), 0, s, feats, (float *)work, n_frames, D);
    HIP_TRY(hipGetLastError());                      // a launch that failed is reported before the next one is enqueued
    hipLaunchKernelGGL(abx_dtw_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(abx_count_kernel, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_abx_index_workspace_bytes(int M, int D, uint64_t *bytes) {
    VQ_REQUIRE(bytes, "vqcpc_abx_index_workspace_bytes: null argument");
    VQ_REQUIRE(M >= 1 && M <= 4096, "vqcpc_abx_index_workspace_bytes: M = %d, need 1 .. 4096", M);
    VQ_REQUIRE(D >= 4 && D <= 512 && D % 4 == 0, "vqcpc_abx_index_workspace_bytes: D = %d, need a multiple of 4 in [4, 512]", D);
    *bytes = ((uint64_t)M * D + (uint64_t)M * M) * sizeof(float);
    return VQCPC_OK;
}

extern "C" int vqcpc_abx_code_table(const float *codebook, int M, int D, void *work, float *table, void *stream) {
    VQ_REQUIRE(codebook && work && table, "vqcpc_abx_code_table: null argument");
    VQ_REQUIRE(M >= 1 && M <= 4096, "vqcpc_abx_code_table: M = %d, need 1 .. 4096", M);
    VQ_REQUIRE(D >= 4 && D <= 512 && D % 4 == 0, "vqcpc_abx_code_table: D = %d, need a multiple of 4 in [4, 512]", D);
    VQ_REQUIRE(((uintptr_t)codebook & 15) == 0 && ((uintptr_t)work & 15) == 0 && ((uintptr_t)table & 15) == 0,
               "vqcpc_abx_code_table: codebook, work and table must be 16-byte aligned");
    TRY(vq_require_gfx950());
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(abx_normalise_kernel, dim3((M + 3) / 4), dim3(256), 0, s, codebook, (float *)work, M, D);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(abx_code_table_kernel, dim3((M * M + 255) / 256), dim3(256), 0, s, (const float *)work, table, M, D);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

extern "C" int vqcpc_abx_score_indices(const float *table, int M, const int32_t *codes, int n_frames, const int32_t *tokens,
                                       int n_tokens, const int32_t *lists, int n_lists, const int32_t *segs, int n_segs,
                                       const int32_t *blocks, int n_blocks, int n_workgroups, int64_t n_dist, int64_t n_out,
                                       float *cost, int32_t *path_len, float *dist, int32_t *twice_wins, void *stream, int metric) {
    VQ_REQUIRE(metric == VQCPC_ABX_ANGULAR || metric == VQCPC_ABX_EDIT, "vqcpc_abx_score_indices: metric = %d, need VQCPC_ABX_ANGULAR (0) or VQCPC_ABX_EDIT (1)", metric);
    VQ_REQUIRE(codes && tokens && lists && segs && blocks && dist && twice_wins, "vqcpc_abx_score_indices: null argument");
    VQ_REQUIRE(table || metric == VQCPC_ABX_EDIT, "vqcpc_abx_score_indices: null table (only the edit metric runs without one)");
    VQ_REQUIRE(M >= 1 && M <= 4096, "vqcpc_abx_score_indices: M = %d, need 1 .. 4096", M);
    VQ_REQUIRE(n_frames >= 1 && n_tokens >= 1 && n_lists >= 1 && n_segs >= 2 && n_blocks >= 1,
               "vqcpc_abx_score_indices: n_frames, n_tokens, n_lists, n_blocks must be >= 1 and n_segs >= 2");
    VQ_REQUIRE(n_workgroups >= 1, "vqcpc_abx_score_indices: n_workgroups = %d, need at least 1", n_workgroups);
    VQ_REQUIRE(n_dist >= 1 && n_dist < (1ll << 31) && n_out >= 1 && n_out < (1ll << 31),
               "vqcpc_abx_score_indices: n_dist = %lld and n_out = %lld must be in [1, 2^31): cut the call into chunks of blocks",
               (long long)n_dist, (long long)n_out);
    VQ_REQUIRE(((uintptr_t)table & 15) == 0, "vqcpc_abx_score_indices: table must be 16-byte aligned");
    TRY(vq_require_gfx950());
    AbxArgs a;
    a.fn = nullptr; a.table = table; a.codes = codes; a.M = M; a.D = 0;
    a.tokens = tokens; a.lists = lists; a.segs = segs; a.blocks = blocks;
    a.cost = cost; a.dist = dist; a.path_len = path_len; a.twice_wins = twice_wins;
    a.n_frames = n_frames; a.n_tokens = n_tokens; a.n_lists = n_lists; a.n_segs = n_segs; a.n_blocks = n_blocks;
    a.n_dist = n_dist; a.n_out = n_out;
    hipStream_t s = (hipStream_t)stream;
    if (metric == VQCPC_ABX_EDIT) hipLaunchKernelGGL(abx_edit_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(abx_index_dtw_kernel, dim3(n_workgroups), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(abx_count_kernel, dim3((unsigned)((n_out + 63) / 64)), dim3(64), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
