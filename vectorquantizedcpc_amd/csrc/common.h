// Internal helpers shared by the HIP translation units of libvqcpc_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <type_traits>
#include "../../include/vqcpc.h"

// runtime.hip: the per-thread error string behind vqcpc_last_error, and the check every create call starts with
void vq_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int vq_require_gfx950();             // VQCPC_OK, or VQCPC_ERR_NO_DEVICE with the error set: the current device is not a gfx950

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            vq_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                         __LINE__);                                                        \
            return VQCPC_ERR_HIP;                                                          \
        }                                                                                  \
    } while (0)

#define VQ_REQUIRE(cond, ...)                   \
    do {                                        \
        if (!(cond)) {                          \
            vq_set_error(__VA_ARGS__);          \
            return VQCPC_ERR_INVALID;           \
        }                                       \
    } while (0)

// propagate a VQCPC_* status
#define TRY(x) do { int rc_ = (x); if (rc_ != VQCPC_OK) return rc_; } while (0)

// A call on a handle (`what`: the entry's name) must run on the device the handle was created on.
inline int vq_require_device(int handle_device, const char *what) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    VQ_REQUIRE(dev == handle_device, "%s: handle belongs to device %d, current device is %d", what, handle_device, dev);
    return VQCPC_OK;
}
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
template <class... P> inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15) == 0; }    // all of them; null counts
// H / 64 in {1, 2, 4, 8} (hidden sizes 64, 128, 256, 512) as a compile-time constant: f(std::integral_constant<int, H / 64>());
// false, and f not called, for any other value.
template <class F> inline bool vq_with_sw(int sw, F &&f) {
    switch (sw) {
        case 1: f(std::integral_constant<int, 1>()); return true;
        case 2: f(std::integral_constant<int, 2>()); return true;
        case 4: f(std::integral_constant<int, 4>()); return true;
        case 8: f(std::integral_constant<int, 8>()); return true;
        default: return false;
    }
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// runtime.hip: bytes held by the live DevBufs / HostBufs of this process (vqcpc_debug_live_bytes)
void vq_count_bytes(bool pinned, long long delta);

// Grow-only memory that frees itself: device memory (DevBuf) or page-locked host memory (HostBuf; `host_flags` are
// hipHostMalloc's and mean nothing to a DevBuf).  All device and pinned memory of the library is one of the two, a member of
// a handle or a local: destroying a handle is `delete`.  Contents are not kept across a growth.
template <bool PINNED> struct OwnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    ~OwnedBuf() { release(); }
    int reserve(size_t bytes, unsigned host_flags = hipHostMallocDefault) {
        if (bytes <= cap) return VQCPC_OK;
        release();
        hipError_t e = PINNED ? hipHostMalloc(&p, bytes, host_flags) : hipMalloc(&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            vq_set_error("%s(%zu) failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", bytes, hipGetErrorString(e));
            return VQCPC_ERR_ALLOC;
        }
        cap = bytes;
        vq_count_bytes(PINNED, (long long)bytes);
        return VQCPC_OK;
    }
    void release() {
        if (!p) return;
        (void)(PINNED ? hipHostFree(p) : hipFree(p));
        vq_count_bytes(PINNED, -(long long)cap);
        p = nullptr; cap = 0;
    }
    template <class T> T *as() const { return (T *)p; }
};
using DevBuf = OwnedBuf<false>;
using HostBuf = OwnedBuf<true>;
// The typed view: a DevBuf that reads as a T *.
template <class T> struct DevPtr : DevBuf {
    operator T *() const { return (T *)p; }
};
// reserve, then copy `bytes` from src (host or device, by `kind`) with a blocking hipMemcpy
inline int dev_copy(DevBuf &dst, const void *src, size_t bytes, hipMemcpyKind kind) {
    TRY(dst.reserve(bytes));
    HIP_TRY(hipMemcpy(dst.p, src, bytes, kind));
    return VQCPC_OK;
}

// A host-mapped word (on a 64-byte line of its own) that kernels write through `dev` and the host reads through `host`
// without a HIP call: the status word of a vocoder, the abort flag of the resident context scan.
struct PinnedWord {
    HostBuf mem;
    unsigned *host = nullptr, *dev = nullptr;
    int create() {
        TRY(mem.reserve(64, hipHostMallocMapped));
        host = (unsigned *)mem.p;
        *host = 0u;
        HIP_TRY(hipHostGetDevicePointer((void **)&dev, host, 0));
        return VQCPC_OK;
    }
};

// ---- exact-chain GEMM (gemm_chain.hip), also used for the hoisted projections of the vocoder.
// Y[m, n] = fold over K blocks of KC of an fp32 fma chain (k ascending, from 0) of
// A[m, k] * W[n, k]; first block: (bias ? bias[n] + chain : chain), later: tot + chain.
// A dense row-major (lda) ; W (N, K) row-major ; N % 64 == 0 ; K % 32 == 0 ; KC % 32 == 0.
int vq_gemm_chain(const float *A, int lda, const float *W, const float *bias, float *Y, int ldy,
                  int M, int N, int K, int KC, hipStream_t s);

// The same with an epilogue: optional ReLU, and an optional output row map for chunked scans -- row m is stored at
// (m / ydiv) * ystride + yoff + m % ydiv, or not at all when yoff + m % ydiv >= ylim (ydiv == 0: plain row m).
int vq_gemm_chain_ex(const float *A, int lda, const float *W, const float *bias, float *Y, int ldy,
                     int M, int N, int K, int KC, int relu, int ydiv, int ystride, int yoff, int ylim, hipStream_t s);

// ---- recurrent scans (scan.hip): the encoder's context LSTM and the vocoder prenet's bidirectional GRU layers.
// W (n_rg row groups x K) in fragment order for the launch-per-step MFMA kernels; rowmode and layout: scan.hip.  `out` is reserved here.
int vq_build_wfrag(const float *W, int ldw, int n_rg, int K, int ksplit, int rowmode, int H, DevBuf &out, hipStream_t s = 0);
// One bidirectional GRU layer's T steps from zero state.  Gi: hoisted input projection [rows][2][3H] (+ b_ih); Wf: both directions'
// W_hh, each from vq_build_wfrag(rowmode 3); b_hh [2][3H]; hbuf: 4 * ceil(B / 16) * 16 * H floats of state; out [rows][2H].
// len / row0: valid steps and first row of every utterance (ragged rows), or null = T steps from row b * T.
int vq_bigru_scan(const float *Wf, const float *b_hh, const float *Gi, float *hbuf, float *out, const int *len, const int *row0,
                  int H, int B, int T, hipStream_t s);
// W_hh^T of a recurrent layer (K gate rows, H columns) in the fragment order of the backward scans' MFMA (context_grad.hip,
// build_wfrag_t_kernel): (H / 16) (K / 16) 64 float4 into WfT.  H % 16 == 0, K % 64 == 0.
void vq_build_wfrag_t(const float *w_hh, float *WfT, int H, int K, hipStream_t s);
struct LstmPlan;   // opaque, owns fragment-ordered weights
int vq_lstm_plan_create(const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                        int D, int H, LstmPlan **out);
void vq_lstm_plan_destroy(LstmPlan *p);
// x (B, T, D) device -> out (B, T, H) device, zero initial state.
int vq_lstm_run(LstmPlan *p, const float *x, int B, int T, float *out, hipStream_t s);
int vq_lstm_set_persistent(LstmPlan *p, int value);                  // -1 auto (one utterance: the resident scan), 0 one launch per time step
int vq_lstm_set_debug(LstmPlan *p, int drop_step, int timeout_ms);   // tests of the abort path
int vq_lstm_check(LstmPlan *p);            // after the caller's sync: did the resident scan of the last call time out?
void vq_add_vec(const float *a, const float *b, float *o, int n, hipStream_t s);      // o = a + b, n floats
// The weights an LSTM computes with: the plan's copies, or a caller's tensors with the sums and fragments built from them.
struct LstmWeights {
    const float *w_ih, *w_hh;      // (4H, D), (4H, H) row-major
    const float *bias;             // b_ih + b_hh (4H)
    const float *Wf;               // w_hh in fragment order: vq_build_wfrag(w_hh, H, H / 4, H, 4, 4, H)
    int D, H;
};
LstmWeights vq_lstm_plan_weights(const LstmPlan *p);
// The launch-per-step scan of that LSTM, x (B, T, D) -> out (B, T, H) from zero state, in two halves over a grow-only scratch that
// the caller owns: vq_lstm_project reserves the scratch and enqueues the hoisted projection gi = x W_ih^T + bias; vq_lstm_steps
// zeroes the h and cell tiles and enqueues the T step launches (seq_step.h), which also fill *save if it is given.
struct LstmScratch {
    DevBuf gi, hbuf, cbuf;         // hoisted projection (B T, 4H), two h tiles, one cell tile
    size_t bytes() const { return gi.cap + hbuf.cap + cbuf.cap; }
};
struct SeqSave;                    // seq_step.h
int vq_lstm_project(LstmScratch &k, const LstmWeights &w, const float *x, int B, int T, hipStream_t s);
int vq_lstm_steps(LstmScratch &k, const LstmWeights &w, int B, int T, float *out, const SeqSave *save, hipStream_t s);

// ---- fixed-order sums over rows (grad_rows.hip; the orders: grad_slab.h), enqueued on s.  R < 2^31 rows.
// out (Na, ldo)[:, :Nb] += A^T B for A (R, lda), B (R, ldb); Na % 64 == 0, Nb % 16 == 0.
void vq_grad_atb(const float *A, int lda, const float *Bm, int ldb, float *out, int ldo, int R, int Na, int Nb, hipStream_t s);
// out (Na) += column sums of A (R, lda); Na % 64 == 0.
void vq_grad_colsum(const float *A, int lda, float *out, int R, int Na, hipStream_t s);
// out (R, N) = A (R, K) W (K rows of ldw); K % 64 == 0, N % 16 == 0.
void vq_grad_rows_w(const float *A, const float *W, int ldw, float *out, int R, int K, int N, hipStream_t s);

// ---- gradients of the context LSTM (context_grad.hip): a forward that keeps state, and back-propagation through time.
// The work space of both, grow-only, a member of the encoder handle.
struct CtxGradWork {
    LstmScratch fwd;               // forward: its own scratch of the launch-per-step scan (vq_lstm_run has the plan's)
    DevBuf bias, Wf;               // forward, caller's weights: b_ih + b_hh and the W_hh fragments
    DevBuf WfT;                    // backward: W_hh^T fragments
    DevBuf dA, carry, part;        // backward: pre-activation gradients (B T, 4H), the cell carry (B, H), slab partials
    size_t bytes() const { return fwd.bytes() + bias.cap + Wf.cap + WfT.cap + dA.cap + carry.cap + part.cap; }
};
size_t vq_ctx_saved_bytes(int B, int T, int H);
// c (B, T, H) from vq_lstm_run's own launch-per-step scan (vq_lstm_project, vq_lstm_steps); `saved` receives what vq_ctx_bwd reads again.
// own_weights: w.bias and w.Wf are not given -- they are built from b_ih, b_hh, w.w_hh into the work space, in stream order.
int vq_ctx_fwd(CtxGradWork &k, LstmWeights w, bool own_weights, const float *b_ih, const float *b_hh, const float *z, int B, int T,
               float *c, float *saved, hipStream_t s);
// Each gradient may be null: grad_z (B T, D), grad_w_ih (4H, D), grad_w_hh (4H, H), grad_bias (4H).
int vq_ctx_bwd(CtxGradWork &k, LstmWeights w, const float *z, int B, int T, const float *c, const float *saved, const float *grad_c,
               float *grad_z, float *grad_w_ih, float *grad_w_hh, float *grad_bias, hipStream_t s);
