// scan.hip -- the recurrent scans over a sequence whose input projection is hoisted (one GEMM ahead of the scan): the
// vocoder prenet's bidirectional GRU layers (network_vocoder.py:41-78) and the encoder's context LSTM (model.py:57, :69).
// A step is W_hh h_{t-1} on v_mfma_f32_16x16x4_f32 in fragment-ordered weights (the launch-per-step form of vocoder.hip's
// sample loop, DESIGN.md "Decode loop") plus the cell update; the encoder's single-utterance LSTM scan runs as one
// resident kernel instead (lstm_persist_kernel).
#include "common.h"
#include "ar_shared.h"
#include "seq_step.h"
#include <math.h>

// ------------------------------------------------------------------------------------------
// Fragment-ordered weights.  For row group `rg` (16 rows, row_of(rg, i) or -1 = zero row),
// K split over `ksplit` waves, super-step S = 16 consecutive k:
//   Wf[((rg*ksplit + w)*SW + s)*64 + lane] (float4) = W[row_of(rg, lane&15)][16*S + 4*(lane>>4) + 0..3]
// with S = w*SW + s.  rowmode: 0 plain (row = 16 rg + i), 8 half groups (row = 8 rg + i, i < 8), 16 GRU gate tiles (rg = 3 blk + gate: that gate of units 16 blk + i), 3 GRU gates, 4 LSTM gates
// (row = gate*H + 4 rg + i%4, gate = i/4; rows >= G*4 are zero).
// ------------------------------------------------------------------------------------------
__global__ void build_wfrag_kernel(const float *__restrict__ W, int ldw, float *__restrict__ Wf, int n_rg,
                                   int K, int ksplit, int rowmode, int H) {
    const int SW = K / 16 / ksplit;
    const size_t total = (size_t)n_rg * ksplit * SW * 64;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int lane = (int)(id & 63);
    size_t r = id >> 6;
    const int s = (int)(r % SW); r /= SW;
    const int w = (int)(r % ksplit);
    const int rg = (int)(r / ksplit);
    const int i = lane & 15, kq = lane >> 4, S = w * SW + s;
    int row;
    if (rowmode == 0) row = 16 * rg + i;
    else if (rowmode == 8) row = i < 8 ? 8 * rg + i : -1;
    else if (rowmode == 16) row = (rg % 3) * H + 16 * (rg / 3) + i;
    else row = (i >> 2) < rowmode ? (i >> 2) * H + 4 * rg + (i & 3) : -1;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row >= 0) v = *(const float4 *)(W + (size_t)row * ldw + 16 * S + 4 * kq);
    ((float4 *)Wf)[id] = v;
}

int vq_build_wfrag(const float *W, int ldw, int n_rg, int K, int ksplit, int rowmode, int H, DevBuf &out, hipStream_t s) {
    VQ_REQUIRE(K % (16 * ksplit) == 0 && ldw % 4 == 0, "build_wfrag: K=%d not a multiple of %d", K, 16 * ksplit);
    const size_t n4 = (size_t)n_rg * (K / 16) * 64;
    TRY(out.reserve(n4 * sizeof(float4)));
    hipLaunchKernelGGL(build_wfrag_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, W, ldw, out.as<float>(), n_rg, K,
                       ksplit, rowmode, H);
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}

// ------------------------------------------------------------------------------------------
// Sequence recurrences with a hoisted input projection (prenet bi-GRU, encoder LSTM).
// ------------------------------------------------------------------------------------------
template <int G, int SW>   // G = 3 GRU, 4 LSTM; the step itself: seq_step.h
__global__ __launch_bounds__(256) void seq_step_kernel(SeqP p, int step) {
    seq_step_body<G, SW, false>(p, step, SeqSave{});
}

// The LSTM step that also stores what back-propagation through time reads again (context_grad.hip).
template <int SW>
__global__ __launch_bounds__(256) void seq_step_save_kernel(SeqP p, int step, SeqSave sv) {
    seq_step_body<4, SW, true>(p, step, sv);
}

template <int G, bool SAVE = false>
static int launch_seq(const SeqP &p, int step, hipStream_t s, const SeqSave &sv = SeqSave{}) {
    static_assert(!SAVE || G == 4, "only the LSTM step saves");
    dim3 grid(p.H / 4, p.ndir, p.nbt), blk(256);
    // hidden sizes 64, 128 (the reference's prenet), 256 (its context LSTM), 512
    const bool built = vq_with_sw(p.H / 64, [&](auto sw) {
        constexpr int SW = decltype(sw)::value;
        if constexpr (SAVE) hipLaunchKernelGGL((seq_step_save_kernel<SW>), grid, blk, 0, s, p, step, sv);
        else hipLaunchKernelGGL((seq_step_kernel<G, SW>), grid, blk, 0, s, p, step);
    });
    if (!built) { vq_set_error("recurrent step: hidden size %d unsupported (64, 128, 256 and 512 are built)", p.H); return VQCPC_ERR_INVALID; }
    return VQCPC_OK;
}

int vq_bigru_scan(const float *Wf, const float *b_hh, const float *Gi, float *hbuf, float *out, const int *len, const int *row0,
                  int H, int B, int T, hipStream_t s) {
    const int nbt = (B + 15) / 16;
    HIP_TRY(hipMemsetAsync(hbuf, 0, (size_t)2 * 2 * nbt * H * 16 * sizeof(float), s));
    SeqP q{};
    q.Wf = Wf; q.b_hh = b_hh; q.Gi = Gi; q.hbuf = hbuf;
    q.out = out; q.len = len; q.row0 = row0; q.H = H; q.nbt = nbt; q.B = B; q.T = T; q.ndir = 2;
    for (int t = 0; t < T; ++t) TRY(launch_seq<3>(q, t, s));
    return VQCPC_OK;
}

__global__ void add_vec_kernel(const float *a, const float *b, float *o, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) o[i] = a[i] + b[i];
}

// ---- encoder LSTM plan (model.py:57)
struct LstmPlan {
    int D, H;
    DevPtr<float> w_ih, bias, Wf;
    DevPtr<float> w_hh;                  // plain [4H][H] copy for the persistent single-utterance scan
    LstmScratch k;
    DevBuf px;
    PinnedWord abort;                    // a timed-out exchange of the persistent scan is reported by the next call
    int persistent = -1;                 // -1 auto (one utterance, H = 256), 0 off, 2 = auto with agent-scope stores forced (tests)
    bool pending = false;                // a persistent scan may have raised the flag
    int dbg_drop_step = -1;              // tests: worker 3 skips its publish at this step -> the others time out
    int timeout_ms = 1000;               // bound of the scan's in-kernel waits
};
static int lstm_persist_launch(LstmPlan *p, int T, float *out, hipStream_t s);
void vq_lstm_plan_destroy(LstmPlan *p) { delete p; }
void vq_add_vec(const float *a, const float *b, float *o, int n, hipStream_t s) {
    hipLaunchKernelGGL(add_vec_kernel, dim3((n + 255) / 256), dim3(256), 0, s, a, b, o, n);
}
LstmWeights vq_lstm_plan_weights(const LstmPlan *p) { return LstmWeights{p->w_ih, p->w_hh, p->bias, p->Wf, p->D, p->H}; }
int vq_lstm_plan_create(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int D, int H,
                        LstmPlan **out) {
    VQ_REQUIRE(D % 32 == 0 && (H == 64 || H == 128 || H == 256 || H == 512), "LSTM: need D %% 32 == 0 and a hidden size of 64, 128, 256 "
               "(model.py:57) or 512 (got %d, %d)", D, H);
    LstmPlan *p = new LstmPlan();
    p->D = D; p->H = H;
    *out = p;
    TRY(dev_copy(p->w_ih, w_ih, (size_t)4 * H * D * sizeof(float), hipMemcpyDeviceToDevice));
    TRY(p->bias.reserve((size_t)4 * H * sizeof(float)));
    vq_add_vec(b_ih, b_hh, p->bias.as<float>(), 4 * H, 0);
    HIP_TRY(hipGetLastError());
    TRY(vq_build_wfrag(w_hh, H, H / 4, H, 4, 4, H, p->Wf));
    TRY(dev_copy(p->w_hh, w_hh, (size_t)4 * H * H * sizeof(float), hipMemcpyDeviceToDevice));
    return p->abort.create();
}
int vq_lstm_set_persistent(LstmPlan *p, int value) { p->persistent = value; return VQCPC_OK; }
int vq_lstm_set_debug(LstmPlan *p, int drop_step, int timeout_ms) { p->dbg_drop_step = drop_step; p->timeout_ms = timeout_ms; return VQCPC_OK; }
// Valid once the stream that carried the scan has been synchronised (the next call on the handle checks as well: by then
// the flag of a still-running scan may not be set yet, which is why callers that fetch results check after their sync).
int vq_lstm_check(LstmPlan *p) {
    if (!p->pending) return VQCPC_OK;
    p->pending = false;
    if (*(volatile unsigned *)p->abort.host != 0u) {
        *p->abort.host = 0u;
        p->persistent = 0;
        vq_set_error("encoder LSTM: an in-kernel exchange of the resident scan timed out (the context of that call is incomplete); "
                     "this handle now uses one launch per time step -- call again");
        return VQCPC_ERR_HIP;
    }
    return VQCPC_OK;
}
static size_t lstm_tile_bytes(int B, int H) { return (size_t)((B + 15) / 16) * H * 16 * sizeof(float); }
int vq_lstm_project(LstmScratch &k, const LstmWeights &w, const float *x, int B, int T, hipStream_t s) {
    const int H = w.H;
    TRY(k.gi.reserve((size_t)B * T * 4 * H * sizeof(float)));
    TRY(k.hbuf.reserve(2 * lstm_tile_bytes(B, H)));
    TRY(k.cbuf.reserve(lstm_tile_bytes(B, H)));
    return vq_gemm_chain(x, w.D, w.w_ih, w.bias, k.gi.as<float>(), 4 * H, B * T, 4 * H, w.D, w.D, s);
}
int vq_lstm_steps(LstmScratch &k, const LstmWeights &w, int B, int T, float *out, const SeqSave *save, hipStream_t s) {
    const size_t hsz = lstm_tile_bytes(B, w.H);
    HIP_TRY(hipMemsetAsync(k.hbuf.p, 0, 2 * hsz, s));
    HIP_TRY(hipMemsetAsync(k.cbuf.p, 0, hsz, s));
    SeqP q{};
    q.Wf = w.Wf; q.Gi = k.gi.as<float>(); q.hbuf = k.hbuf.as<float>(); q.cbuf = k.cbuf.as<float>();
    q.out = out; q.len = nullptr; q.H = w.H; q.nbt = (B + 15) / 16; q.B = B; q.T = T; q.ndir = 1;
    for (int t = 0; t < T; ++t) TRY((save ? launch_seq<4, true>(q, t, s, *save) : launch_seq<4>(q, t, s)));
    HIP_TRY(hipGetLastError());
    return VQCPC_OK;
}
int vq_lstm_run(LstmPlan *p, const float *x, int B, int T, float *out, hipStream_t s) {
    const LstmWeights w = vq_lstm_plan_weights(p);
    TRY(vq_lstm_project(p->k, w, x, B, T, s));
    TRY(vq_lstm_check(p));               // did an earlier persistent scan report a timeout?  (no HIP call: host-mapped word)
    // encode.py:42-46 calls encode() on ONE utterance at a time: that scan is a chain of T dependent 256-value exchanges,
    // 3.6 us each as launches, < 1 us each inside one resident kernel
    if (p->persistent != 0 && B == 1 && p->H == 256 && T >= 1) return lstm_persist_launch(p, T, out, s);
    return vq_lstm_steps(p->k, w, B, T, out, nullptr, s);
}

// ------------------------------------------------------------------------------------------
// fp32 fma chains on the vector ALU, bit-identical to the v_mfma_f32_16x16x4_f32 schedule of the launch-per-step kernels
// (a chain is a sequence of fp32 fmas in a fixed k order: two accumulators per K quarter, the x/z and y/w components of
// the fragment; partial sums combined a0 + a1, then ((q0 + q1) + q2) + q3) -- used by the resident context scan below.
// (Round 2's 64-workgroup persistent single-utterance decoder, ar_persist_kernel, lived in vocoder.hip; the per-XCD decoders of
// ar_xcd.hip replaced it in round 3 -- 2.6 us per sample against 4.95 -- and it was removed in round 4.)
// ------------------------------------------------------------------------------------------
// index of h[k] in the LDS copy: inside each 16-block, [component k % 4][k / 4 % 4], so that a chain reads the four
// k of one MFMA as one 16-byte LDS word
__device__ __forceinline__ int ps_perm(int k) { return (k & ~15) | ((k & 3) << 2) | ((k >> 2) & 3); }

// one accumulator chain: NS super-steps of this K quarter, components c0 then c0 + 2 (the x/z or y/w MFMA operands)
// (hipcc keeps one or two operand reads in flight here -- read, wait, 4 fmas.  Forcing a deeper window, by a register
// window, by volatile reads or by sched_group_barrier, each made it spill 70-240 registers; measured alternatives dropped.)
template <int NS>
__device__ __forceinline__ float ps_chain(const float (&w)[8 * NS], const float4 *hb, int kw, int c0) {
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float4 h0 = hb[(kw * NS + s) * 4 + c0], h1 = hb[(kw * NS + s) * 4 + c0 + 2];
        acc = __builtin_fmaf(w[8 * s + 0], h0.x, acc); acc = __builtin_fmaf(w[8 * s + 1], h0.y, acc);
        acc = __builtin_fmaf(w[8 * s + 2], h0.z, acc); acc = __builtin_fmaf(w[8 * s + 3], h0.w, acc);
        acc = __builtin_fmaf(w[8 * s + 4], h1.x, acc); acc = __builtin_fmaf(w[8 * s + 5], h1.y, acc);
        acc = __builtin_fmaf(w[8 * s + 6], h1.z, acc); acc = __builtin_fmaf(w[8 * s + 7], h1.w, acc);
    }
    return acc;
}
// the 8 chains of a row sit in 8 consecutive lanes (index 2 kw + a): returns, in the row's first lane, the row sum in
// the order of the launch-per-step kernels
// (DPP moves inside the row of 16 lanes instead of ds_bpermute round trips; only the row's first lane is meaningful)
__device__ __forceinline__ float ps_combine(float acc, int lane) {
    (void)lane;
    const float other = PS_DPP(acc, 0xB1);             // quad_perm [1,0,3,2]: lane ^ 1
    const float q = acc + other;                       // a0 + a1 (both lanes hold it)
    const float q1 = PS_DPP(q, 0x4E);                  // quad_perm [2,3,0,1]: lane ^ 2 (= base + 2 in the first lane)
    const float q2 = PS_DPP(q, 0x104);                 // row_shl:4: lane + 4
    const float q3 = PS_DPP(q, 0x106);                 // row_shl:6: lane + 6
    return ((q + q1) + q2) + q3;
}

// Every workgroup's granules start on a 128-byte line of their own (16 granules): lines shared by writers on different
// CUs serialised the write-through stores -- the 64 one-granule candidate stores into 4 lines took 2.7 us to be seen.
#define PS_PAD 16
__device__ __forceinline__ int ps_slot(int idx, int per_blk) { return (idx / per_blk) * PS_PAD + idx % per_blk; }

// Sweep N granules per lane (stride 64) until every tag equals `tag`; bounded.  Returns false on timeout / abort.
template <int N>
__device__ __forceinline__ bool ps_sweep(const u64 *g, int lane, int per_blk, unsigned tag, unsigned (&val)[N], unsigned *abort_flag,
                                         u64 ticks = 100000000ull) {
    const u64 t0 = __builtin_amdgcn_s_memrealtime();
    int slot[N];
#pragma unroll
    for (int j = 0; j < N; ++j) slot[j] = ps_slot(lane + 64 * j, per_blk);
    for (unsigned spins = 0;; ++spins) {
        bool ok = true;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const u64 x = ps_load(g + slot[j]);
            val[j] = (unsigned)x;
            ok &= (unsigned)(x >> 32) == tag;
        }
        if (__all(ok)) return true;
        if ((spins & 63) == 63) {
            const bool late = __builtin_amdgcn_s_memrealtime() - t0 > ticks;                 // default 1 s at 100 MHz
            if (late || __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) {
                if (late && lane == 0) __hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                return false;
            }
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// ------------------------------------------------------------------------------------------
// Persistent scan of the encoder LSTM for ONE utterance (model.py:57 as encode.py:42-46 calls it: batch 1).
// The input projection is hoisted (Gi), so a time step is W_hh h_{t-1} (1024 x 256) + the cell update + an all-to-all of
// 256 values.  32 workgroups of 256 threads stay resident, each with 8 hidden units = 32 gate rows in registers (8 chain
// lanes per row, the chains and their combination exactly those of seq_step_kernel's MFMAs -> the same bits), and exchange
// h_t as {tag, value} granules, one 128-B line per workgroup.
// All 32 sit on ONE XCD: the grid is 8 x 32 and only every 8th workgroup works (workgroup id % 8 is the XCD:
// profiles/r02_xcd_exchange_microbench.csv).  Parties that share an L2 can publish with plain stores -- the write-through
// L1 leaves them in that L2, where sc1 loads find them: 0.41 us per exchange against 1.2 us through memory.  The placement
// is CHECKED, not assumed: the workers first exchange their XCC_ID with agent-scope stores, and fall back to those for the
// scan unless all ids agree.  Every wait is bounded; a timeout raises a host-mapped flag the next call reports.
// ------------------------------------------------------------------------------------------
#define LP_NW 32          // workers
#define LP_UPB 8          // hidden units per worker (H = 256)
struct LstmPersistP {
    const float *w_hh;    // [4H][H]
    const float *Gi;      // [T][4H]  W_ih x_t + b_ih + b_hh
    float *out;           // [T][H]
    u64 *g;               // [2][LP_NW][PS_PAD] granules: h_t goes to buffer t & 1 -- with ONE exchange per step a fast worker
                          // publishes h_t while a slow one still sweeps h_{t-1}; it cannot reach h_{t+1} before that sweep ended
    unsigned *abort_flag;
    int T;
    int force_agent;      // tests: publish with agent-scope stores even when all workers share an XCD (the fallback path)
    int dbg_drop_step;    // tests: worker 3 skips its publish at this step
    unsigned timeout_ticks;
};
template <bool LOCAL>
__device__ __forceinline__ void lp_store(u64 *p, u64 v) {
    if (LOCAL) asm volatile("global_store_dwordx2 %0, %1, off sc0" :: "v"(p), "v"(v) : "memory");    // workgroup scope: leaves the CU, stays in this XCD's L2
    else ps_store(p, v);
}
__global__ __launch_bounds__(256) void lstm_persist_kernel(LstmPersistP p) {
    constexpr int H = 256;
    if (blockIdx.x % 8 != 0) return;
    const int blk = blockIdx.x / 8, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ __attribute__((aligned(16))) float hbuf[H];             // h_{t-1}, ps_perm order
    __shared__ float gsum[4 * LP_UPB];                                  // W_hh h_{t-1} of the owned rows [gate][unit]
    // ---- resident weights: row r = gate * 8 + unit, 8 chain lanes per row (as ar_persist_kernel)
    const int row_local = tid >> 3, gate = row_local / LP_UPB, ul = row_local % LP_UPB;
    const int kw = (lane & 7) >> 1, c0 = lane & 1;
    float w[8 * 4];
    ps_load_weights<4>(p.w_hh + (size_t)(gate * H + LP_UPB * blk + ul) * H, kw, c0, w);
    const int unit = LP_UPB * blk + (tid < LP_UPB ? tid : 0);
    const u64 *gw = p.g + (size_t)(8 * wave) * PS_PAD;                  // this wave sweeps granules 64 wave .. 64 wave + 63
    // ---- are all workers on one XCD?  (ids exchanged through memory: agent-scope stores, slot 8 of every line)
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 0xfu;
    if (tid == 0) ps_store(p.g + (size_t)blk * PS_PAD + 8, ((u64)0xC0DEu << 32) | xcc);
    bool dead = false, local = true;
    {
        const u64 t0 = __builtin_amdgcn_s_memrealtime();
        for (unsigned spins = 0;; ++spins) {
            const u64 x = ps_load(p.g + (size_t)(lane & 31) * PS_PAD + 8);
            if (__all((unsigned)(x >> 32) == 0xC0DEu)) { local = __all((unsigned)x == xcc) && !p.force_agent; break; }
            if ((spins & 63) == 63 && (__builtin_amdgcn_s_memrealtime() - t0 > 100000000ull ||
                                       __hip_atomic_load(p.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u)) {
                if (lane == 0) __hip_atomic_store(p.abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                dead = true;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    float cst = 0.f;                                                    // cell state of unit `tid` (tid < 8)
    float gi0 = 0.f, gi1 = 0.f, gi2 = 0.f, gi3 = 0.f;
    if (tid < LP_UPB) { const float *gp = p.Gi + unit; gi0 = gp[0]; gi1 = gp[H]; gi2 = gp[2 * H]; gi3 = gp[3 * H]; }
    for (int t = 0; t < p.T; ++t) {
        // ---- h_{t-1} from everyone (zero at t = 0)
        float hv = 0.f;
        if (t > 0 && !dead) {
            unsigned v[1];
            if (ps_sweep<1>(gw + (size_t)((t - 1) & 1) * LP_NW * PS_PAD, lane, LP_UPB, (unsigned)t, v, p.abort_flag, (u64)p.timeout_ticks)) hv = __uint_as_float(v[0]);
            else dead = true;
        }
        hbuf[ps_perm(tid)] = hv;
        ps_barrier();
        const float acc = ps_chain<4>(w, (const float4 *)hbuf, kw, c0);
        const float v = ps_combine(acc, lane);
        if ((lane & 7) == 0) gsum[row_local] = v;
        ps_barrier();
        if (tid < LP_UPB) {
            const float ig = sigmoidf_(gi0 + gsum[tid]), fg = sigmoidf_(gi1 + gsum[LP_UPB + tid]);
            const float gg = tanhf(gi2 + gsum[2 * LP_UPB + tid]), og = sigmoidf_(gi3 + gsum[3 * LP_UPB + tid]);
            cst = fg * cst + ig * gg;
            const float hn = og * tanhf(cst);
            const u64 gr = ((u64)(unsigned)(t + 1) << 32) | __float_as_uint(hn);
            u64 *dst = p.g + ((size_t)(t & 1) * LP_NW + blk) * PS_PAD + tid;
            const bool drop = p.dbg_drop_step == t && blk == 3;          // tests: the other workers' sweeps of h_t time out
            if (drop) { }
            else if (local) lp_store<true>(dst, gr);
            else lp_store<false>(dst, gr);
            p.out[(size_t)t * H + unit] = hn;
            if (t + 1 < p.T) { const float *gp = p.Gi + (size_t)(t + 1) * 4 * H + unit; gi0 = gp[0]; gi1 = gp[H]; gi2 = gp[2 * H]; gi3 = gp[3 * H]; }
        }
    }
}
static int lstm_persist_launch(LstmPlan *p, int T, float *out, hipStream_t s) {
    const size_t bytes = (size_t)2 * LP_NW * PS_PAD * sizeof(u64);
    TRY(p->px.reserve(bytes));
    HIP_TRY(hipMemsetAsync(p->px.p, 0, bytes, s));
    LstmPersistP q{};
    q.w_hh = p->w_hh; q.Gi = p->k.gi.as<float>(); q.out = out; q.g = p->px.as<u64>(); q.T = T;
    q.force_agent = p->persistent == 2;
    q.dbg_drop_step = p->dbg_drop_step;
    q.timeout_ticks = (unsigned)p->timeout_ms * 100000u;
    q.abort_flag = p->abort.dev;
    hipLaunchKernelGGL(lstm_persist_kernel, dim3(8 * LP_NW), dim3(256), 0, s, q);
    HIP_TRY(hipGetLastError());
    p->pending = true;
    return VQCPC_OK;
}
