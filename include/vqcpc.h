/*
 * vqcpc.h -- C ABI of libvqcpc_hip.so: the MI355X (gfx950) implementation of the
 * VQ-CPC inference hot path.
 *
 * The reference (tarepan/VectorQuantizedCPC) has no FFI for this path; its seam is the
 * nn.Module method surface.  Each entry point below names the reference interface it
 * replaces (file:line in /root/reference).  The Python drop-in classes in
 * vectorquantizedcpc_amd/{model,network_vocoder}.py bind these with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *  - Every pointer marked DEVICE is fp32 / int64 memory on the current HIP device,
 *    contiguous, borrowed for the duration of the enqueued work.  HOST pointers are read
 *    before the call returns.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream).  No call synchronises the device except where stated: the *_create calls do
 *    (once); vqcpc_melfront_run and vqcpc_loudness_* synchronise `stream` once while they upload
 *    host-built length tables BEFORE enqueuing their kernels, and return with the work still in
 *    flight; vqcpc_vocoder_kernel_times is a measurement call and returns after its launches have
 *    finished.  vqcpc_vocoder_generate / _logits do NOT synchronise the stream: their host-built
 *    tables (lengths, decode-slot schedule, call records) go through a pinned staging arena owned by
 *    the handle, and a call waits only for the event behind the PREVIOUS call's uploads before it
 *    reuses that arena.  "Does not synchronise" speaks of the library: the HIP runtime holds a bounded number of commands per
 *    stream, and a call that enqueues thousands of launches (a use_graph = 0 decode: three per sample) behind work that has not
 *    started waits on the host for room, as any such sequence of launches does (MI355X: between 1 920 and 2 880 of them).
 *    Held on a caller's stream, entry by entry, by tests/test_gpu_stream_contract.py.
 *  - Return 0 on success, a negative vqcpc_status otherwise; never throws.
 *    vqcpc_last_error() returns a thread-local message for the last failure.
 *  - One handle per device; a handle is not thread-safe; distinct handles are independent.
 *  - No CPU fallback exists: without a gfx950 device every compute call fails.
 */
#ifndef VQCPC_H
#define VQCPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQCPC_ABI_VERSION 1

typedef enum {
    VQCPC_OK = 0,
    VQCPC_ERR_INVALID = -1,     /* bad argument / unsupported shape        */
    VQCPC_ERR_HIP = -2,         /* a HIP runtime call failed               */
    VQCPC_ERR_NO_DEVICE = -3,   /* no gfx950 device visible                */
    VQCPC_ERR_ALLOC = -4
} vqcpc_status;

int vqcpc_abi_version(void);
const char *vqcpc_last_error(void);

/* Number of visible HIP devices whose arch is gfx950 (0 = none; never faults). */
int vqcpc_device_count(void);

/* ------------------------------------------------------------------ Encoder ---------- */

/* Encoder.state_dict() (model.py:43-57).  DEVICE pointers, shapes as in the reference:
 * conv_weight (channels, in_channels, 4); ln_*[i] (channels) for encoder.{0,3,6,9,12};
 * fc_weight[i] (channels, channels) for encoder.{2,5,8,11}; out_weight (z_dim, channels),
 * out_bias (z_dim); codebook (n_embeddings, z_dim) = codebook.embedding;
 * rnn_* = nn.LSTM(z_dim, c_dim) parameters (4*c_dim rows, gate order i,f,g,o).
 * Supported: in_channels % 16 == 0 (<= 256), channels == 512, z_dim == 64,
 * n_embeddings % 64 == 0 (<= 4096), c_dim 64, 128, 256 (the reference's) or 512. */
typedef struct {
    const float *conv_weight;
    const float *ln_weight[5];
    const float *ln_bias[5];
    const float *fc_weight[4];
    const float *out_weight;
    const float *out_bias;
    const float *codebook;
    const float *rnn_w_ih, *rnn_w_hh, *rnn_b_ih, *rnn_b_hh;
    int in_channels, channels, n_embeddings, z_dim, c_dim;
} vqcpc_encoder_weights;

typedef struct vqcpc_encoder vqcpc_encoder;

/* Replaces Encoder.__init__ + load_state_dict (model.py:33-57; encode.py:24-30).
 * Copies and re-lays the weights on the current device (synchronises once). */
int vqcpc_encoder_create(const vqcpc_encoder_weights *w, vqcpc_encoder **out);
void vqcpc_encoder_destroy(vqcpc_encoder *enc);

/* conv_mode: which of the reference's two CPU conv back-ends to reproduce bit for bit
 * (ATen chooses by call shape; they sum in different orders):
 *   0 = as the reference would for this (B, T): 2 if B > 1 or B*in_channels*T > 20480 else 1
 *   1 = im2col + sgemm order (a single short utterance, encode.py:44-46's batch-1 call)
 *   2 = oneDNN direct-conv order (batched calls, e.g. vocoder.py:59) */
#define VQCPC_CONV_AUTO 0
#define VQCPC_CONV_IM2COL 1
#define VQCPC_CONV_DIRECT 2

/* Replaces Encoder.encode (model.py:59-70; callers encode.py:46, convert.py:76,
 * vocoder.py:59).  mel DEVICE (B, in_channels, T), T >= 2; To = (T - 2) / 2 + 1 output frames
 * (= T/2 for even T; an odd T keeps its last frame, as Conv1d(k=4, s=2, p=1) does).  Outputs
 * DEVICE: z_q (B, To, z_dim) quantised vectors; idx (B, To) int64 code indices;
 * c (B, To, c_dim) LSTM context or NULL to skip the LSTM (convert.py:76 discards it);
 * z_pre (B, To, z_dim) pre-VQ activations (the encode.py:34-40 hook) or NULL.
 * Code indices are bit-identical to the reference's PyTorch-CPU path for calls with
 * >= 16 output frames ("Bit-exactness contract"). */
int vqcpc_encoder_encode(vqcpc_encoder *enc, const float *mel, int B, int T, int conv_mode,
                         float *z_q, float *c, int64_t *idx, float *z_pre, void *stream);

/* Encoder options.  fused: which schedule of the front end runs (all produce the same bits): 1 = ONE launch, conv +
 * LayerNorms + FC stack + VQ search for 16 whole rows per workgroup with the activations resident in LDS; 2 = six
 * column-split launches (one per Linear, LayerNorm applied on load, VQ in the last) for calls too small to fill the chip
 * with whole-row workgroups; 0 = the layered kernels, one launch per module of model.py:43-55; -1 (default) = 2 for calls
 * of up to `split_max_tiles` (default 80) 16-row tiles, else 1; 0 when 4 * in_channels > 512.
 * persistent_context (default 1): the context LSTM (model.py:57) of a ONE-utterance call -- encode.py:42-46's batch 1 --
 * runs as one resident kernel with in-kernel exchanges of h_t instead of one launch per time step; 0 = always launches;
 * 2 = the resident kernel with agent-scope stores forced (its fallback when the workers do not share an XCD; for tests).
 * Same bits either way. */
int vqcpc_encoder_set_option(vqcpc_encoder *enc, const char *name, int value);

/* Which schedule the front end of the last vqcpc_encoder_encode / _stage call on this handle ran, numbered as the `fused`
 * option: 2 = six column-split launches, 1 = one fused launch, 0 = layered kernels; -1 before the first call.  A host
 * word: no HIP call.  For tests of the automatic choice (split_max_tiles). */
int vqcpc_encoder_last_schedule(vqcpc_encoder *enc);

/* Activations after one stage of the front end for the same inputs as encode() -- the analogue
 * of a forward hook on the reference's modules (encode.py:34-40 hooks encoder.encoder[-1]):
 * stage 0 = conv output transposed to rows (model.py:65-67), 1 = encoder.0+1 (LN, ReLU),
 * 2+2l = encoder.{2,5,8,11}[l] (Linear), 3+2l = the LN+ReLU after it, 10 = encoder.14 (z_pre).
 * out DEVICE (B*To, channels) fp32, or (B*To, z_dim) for stage 10. */
int vqcpc_encoder_stage(vqcpc_encoder *enc, const float *mel, int B, int T, int conv_mode,
                        int stage, float *out, void *stream);

/* Replaces VQEmbeddingEMA.encode called on its own (model.py:103-115): x DEVICE (n_rows, z_dim) fp32 rows,
 * 16-byte aligned -> z_q DEVICE (n_rows, z_dim) = codebook rows, idx DEVICE (n_rows) int64, first index wins
 * ties.  The same kernel vqcpc_encoder_encode runs after the front end. */
int vqcpc_encoder_vq_encode(vqcpc_encoder *enc, const float *x, int n_rows, float *z_q, int64_t *idx,
                            void *stream);

/* Replaces the eval branch of VQEmbeddingEMA.forward as used by Encoder.forward
 * (model.py:72-86, :117-155): from encode()'s z_pre / z_q / idx (n_rows = B*T/2) computes
 * z_st = x + (q - x) (DEVICE, n_rows*z_dim, or NULL), loss = 0.25*mse (DEVICE scalar) and
 * perplexity (DEVICE scalar).  The context for forward() is the LSTM over z_st:
 * vqcpc_encoder_context. */
int vqcpc_encoder_forward_stats(vqcpc_encoder *enc, const float *z_pre, const float *z_q,
                                const int64_t *idx, int n_rows, float *z_st, float *loss,
                                float *perplexity, void *stream);

/* Replaces the training branch of VQEmbeddingEMA.forward (model.py:117-155 with the EMA update of
 * model.py:136-145): no gradient, a forward pass plus the moving average over the three buffers.
 * x DEVICE (n_rows, z_dim) fp32 rows, 16-byte aligned.  idx (n_rows int64), z_st = x + (q - x) (both DEVICE, or NULL),
 * loss and perplexity (DEVICE scalars) come from the OLD codebook, exactly as vqcpc_encoder_vq_encode +
 * vqcpc_encoder_forward_stats give them.  Then, every step a separately rounded fp32 operation:
 *   count = (float)decay * ema_count + (float)(1.0 - decay) * hist;  n = sum(count);
 *   ema_count = (count + (float)epsilon) / (n + (float)(n_embeddings * epsilon)) * n;
 *   ema_weight = (float)decay * ema_weight + (float)(1.0 - decay) * dw,  dw[m] = sum of the rows x[r] with idx[r] == m
 *   (64-row chunks in ascending row order, chunk partials combined by the adjacent-pair tree);
 *   embedding = ema_weight / ema_count[:, None].
 * embedding (n_embeddings, z_dim), ema_count (n_embeddings), ema_weight (n_embeddings, z_dim): DEVICE fp32, updated in
 * place; embedding must hold, on entry, what the handle was created from.  On return (in stream order) embedding AND the
 * handle's own codebook copy, |e|^2 and search fragments hold the new values: the handle equals one created from the new
 * buffers.  No synchronisation.  VQCPC_ERR_INVALID before anything is enqueued for a NULL argument, n_rows outside
 * [1, 2^24] (the histogram must be exact in fp32), decay outside (0, 1) or epsilon <= 0.
 * The work space (quantised rows, indices, counts, histogram) belongs to the handle and is shared by its calls: like every
 * other entry of a handle, one handle serves ONE stream at a time -- two calls on different streams need an event between
 * them or a handle each. */
int vqcpc_encoder_vq_adapt(vqcpc_encoder *enc, const float *x, int n_rows, double decay, double epsilon,
                           float *embedding, float *ema_count, float *ema_weight,
                           float *z_st, int64_t *idx, float *loss, float *perplexity, void *stream);

/* Device memory the handle's grow-only work buffers hold at the moment (front-end activations, statistics, the work space
 * of vqcpc_encoder_vq_adapt, of vqcpc_encoder_context_fwd / _bwd and of the front-end gradients (vqcpc_encoder_front_fwd / _bwd):
 * the peak of the calls so far; the weights are not counted). */
int vqcpc_encoder_workspace_bytes(vqcpc_encoder *enc, uint64_t *bytes);

/* After the caller has synchronised the stream that carried vqcpc_encoder_encode / _context: did the resident context
 * scan of that call (persistent_context) give up on an in-kernel exchange?  VQCPC_OK, or VQCPC_ERR_HIP: the context `c`
 * of that call is incomplete, the handle now runs one launch per time step, and the call should be repeated.  Reads a
 * host-mapped word: no HIP call, no synchronisation.  The reference has no counterpart (its operators are synchronous,
 * encode.py:45-46): consumers that read results back -- driver.encode_utterances, cli.encode_dataset -- call it
 * before anything is written.  Options for tests of this path: context_debug_drop_step (one worker skips its publish at
 * that time step), context_timeout_ms. */
int vqcpc_encoder_check(vqcpc_encoder *enc);

/* nn.LSTM over z (B, Tz, z_dim) -> c (B, Tz, c_dim)  (model.py:69 / :85). */
int vqcpc_encoder_context(vqcpc_encoder *enc, const float *z, int B, int Tz, float *c,
                          void *stream);

/* Bytes of the `saved` buffer that vqcpc_encoder_context_fwd fills for B utterances of Tz steps (its layout is private). */
int vqcpc_encoder_context_saved_bytes(vqcpc_encoder *enc, int B, int Tz, uint64_t *bytes);

/* vqcpc_encoder_context (model.py:57, :69, :85) as the forward of a training step: c (B, Tz, c_dim) DEVICE, and into `saved` --
 * DEVICE, the caller's, vqcpc_encoder_context_saved_bytes bytes, 16-byte aligned -- what vqcpc_encoder_context_bwd reads again
 * (the activated gates, the cell state and its tanh of every row).  c has the BITS vqcpc_encoder_context gives for the same
 * weights at every B (always one launch per time step; the resident single-utterance scan is not used).
 * w_ih (4 c_dim, z_dim), w_hh (4 c_dim, c_dim), b_ih, b_hh (4 c_dim) DEVICE: the LSTM's weights this call uses -- the caller's,
 * so that an optimizer step costs no new handle; the call builds b_ih + b_hh and the W_hh fragments from them in stream order.
 * All four NULL = the handle's copies.  The handle gives sizes and work space only.  Two forwards may precede their two
 * backwards: everything a backward needs is in z, c, saved and the weights.
 * VQCPC_ERR_INVALID before anything is enqueued: a NULL z, c or saved, B < 1 or Tz < 1, only some of the four weight pointers
 * given, a pointer that is not 16-byte aligned, a handle of another device.  Enqueues on `stream`, does not synchronise; the work
 * space belongs to the handle (one stream at a time, as every other entry). */
int vqcpc_encoder_context_fwd(vqcpc_encoder *enc, const float *z, int B, int Tz, const float *w_ih, const float *w_hh,
                              const float *b_ih, const float *b_hh, float *c, void *saved, void *stream);

/* Back-propagation through time of the context LSTM: what loss.backward() leaves in encoder.rnn in train_cpc.py:116-124, given
 * grad_c (B, Tz, c_dim) DEVICE = the gradient of the loss with respect to c (vqcpc_cpc_grad's grad_c), csrc/context_grad.hip.
 * z, c, saved: the input, the output and the saved state of the vqcpc_encoder_context_fwd call; w_ih, w_hh: the weights of
 * that call (both NULL = the handle's copies).
 * Gradients DEVICE, each may be NULL = not wanted (its launches are skipped): grad_z (B, Tz, z_dim), grad_w_ih (4 c_dim, z_dim),
 * grad_w_hh (4 c_dim, c_dim), grad_bias (4 c_dim) -- b_ih and b_hh both receive grad_bias.  Every element of a requested gradient
 * is written (Tz = 1: grad_w_hh is all +0).  One launch per time step, then fixed-order split-K products; every sum runs in one
 * fixed order (no floating-point atomics; csrc/context_grad.hip lists the orders): equal inputs give equal bits, whatever an
 * earlier call left in the work space.  The work space lives on the handle, grows to the largest call and is counted by
 * vqcpc_encoder_workspace_bytes.
 * VQCPC_ERR_INVALID before anything is enqueued: a NULL z, c, saved or grad_c, B < 1 or Tz < 1, exactly one of w_ih / w_hh
 * NULL, a pointer that is not 16-byte aligned, a handle of another device. */
int vqcpc_encoder_context_bwd(vqcpc_encoder *enc, const float *z, int B, int Tz, const float *w_ih, const float *w_hh,
                              const float *c, const void *saved, const float *grad_c, float *grad_z, float *grad_w_ih,
                              float *grad_w_hh, float *grad_bias, void *stream);

/* ------------------------------------------------------------------ Encoder: front-end and VQ gradients ---- */

/* The gradients of the encoder's front end (Conv1d / LayerNorm / Linear, model.py:43-55, :65-67) and of the VQ step's
 * straight-through estimator (model.py:147-150).  Together with vqcpc_cpc_grad and vqcpc_encoder_context_bwd they are
 * loss.backward() of the reference's training step (train_cpc.py:116-124), from the loss down to conv.weight.
 *
 * Every sum of these entries runs in one fixed order (vectorquantizedcpc_amd/csrc/front_grad.hip states each), without
 * floating-point atomics: equal inputs give equal bits, whatever an earlier call left in the handle's work space.  That work
 * space is grow-only and counted by vqcpc_encoder_workspace_bytes. */

/* The front-end part of vqcpc_encoder_weights: DEVICE pointers to the caller's tensors in the reference's shapes, 16-byte
 * aligned.  conv_weight (channels, in_channels, 4); ln_weight[i], ln_bias[i] (channels) for encoder.{0,3,6,9,12}; fc_weight[i]
 * (channels, channels) for encoder.{2,5,8,11}; out_weight (z_dim, channels), out_bias (z_dim).  Every member is required.
 * Where an entry takes `const vqcpc_encoder_front_weights *w`, NULL means the handle's copies; with a struct the handle gives
 * sizes and work space only, and whatever re-layout a kernel needs (the conv weight's k order, transposes) is made per call,
 * in stream order -- an optimizer step costs no new handle. */
typedef struct {
    const float *conv_weight;
    const float *ln_weight[5];
    const float *ln_bias[5];
    const float *fc_weight[4];
    const float *out_weight;
    const float *out_bias;
} vqcpc_encoder_front_weights;

/* The gradients vqcpc_encoder_front_bwd writes: the members of the weights struct as DEVICE output pointers, same shapes,
 * 16-byte aligned.  A NULL member is not wanted: its launches are skipped, and the chain of input-gradient products runs only
 * as far down as the lowest wanted tensor.  Every element of a wanted tensor is written. */
typedef struct {
    float *conv_weight;
    float *ln_weight[5];
    float *ln_bias[5];
    float *fc_weight[4];
    float *out_weight;
    float *out_bias;
} vqcpc_encoder_front_grads;

/* Bytes of the `saved` buffer that vqcpc_encoder_front_fwd fills for B utterances of T mel frames (its layout is private).
 * VQCPC_ERR_INVALID for NULL, B < 1 or T < 2. */
int vqcpc_encoder_front_saved_bytes(vqcpc_encoder *enc, int B, int T, uint64_t *bytes);

/* The front end of a training step: mel (B, in_channels, T) DEVICE -> z_pre (B, T / 2, z_dim) DEVICE, the rows before the VQ
 * (model.py:65-67).  z_pre has the bits of vqcpc_encoder_stage(..., stage 10, ...) for the same weights, shape and conv_mode
 * (the layered schedule: exact-chain GEMMs and ATen's LayerNorm moments).  `saved` (DEVICE, 16-byte aligned,
 * vqcpc_encoder_front_saved_bytes) receives what the backward reads again: the rows entering each of the five LayerNorms, the
 * rows leaving each ReLU, and mean and rstd of every row of every LayerNorm exactly as this forward computed them.
 * w: the caller's weights, or NULL = the handle's copies.
 * VQCPC_ERR_INVALID before anything is enqueued: a NULL enc, mel, z_pre or saved, B < 1, T < 2, conv_mode outside 0 .. 2, a
 * NULL member of *w, a pointer that is not 16-byte aligned, more than 2^22 rows, a handle of another device. */
int vqcpc_encoder_front_fwd(vqcpc_encoder *enc, const float *mel, int B, int T, int conv_mode,
                            const vqcpc_encoder_front_weights *w, float *z_pre, void *saved, void *stream);

/* The backward of vqcpc_encoder_front_fwd: grad_z_pre (B, T / 2, z_dim) DEVICE = dLoss / dz_pre -> the wanted members of
 * *grads.  mel, B, T, conv_mode, w, saved: those of the forward call (w's tensors unchanged since).  The ReLU mask is "the
 * saved post-ReLU value > 0".  There is no gradient with respect to mel.
 * VQCPC_ERR_INVALID before anything is enqueued: as the forward, a NULL grad_z_pre or grads, or no wanted member. */
int vqcpc_encoder_front_bwd(vqcpc_encoder *enc, const float *mel, int B, int T, int conv_mode,
                            const vqcpc_encoder_front_weights *w, const void *saved, const float *grad_z_pre,
                            const vqcpc_encoder_front_grads *grads, void *stream);

/* The backward of model.py:147-150, loss = 0.25 * mse_loss(z_pre, z_q.detach()) and z_st = z_pre + (z_q - z_pre).detach():
 *   grad_z_pre = grad_z_st + grad_loss * (0.5 / (n_rows * z_dim)) * (z_pre - z_q)
 * as separately rounded fp32 operations in this order, per element:
 *   d = z_pre - z_q;   s = grad_loss * k, k = 0.5 / (n_rows * z_dim) formed in double and rounded to fp32 once;
 *   t = s * d;         grad_z_pre = grad_z_st + t.
 * z_pre, z_q, grad_z_st, grad_z_pre (n_rows, z_dim) DEVICE, 16-byte aligned; grad_loss a DEVICE scalar.  grad_loss NULL drops
 * the loss term: grad_z_pre has the bits of grad_z_st.  grad_z_st NULL drops the straight-through term: grad_z_pre = t.
 * VQCPC_ERR_INVALID before anything is enqueued: a NULL enc, z_pre, z_q or grad_z_pre, both gradients NULL, n_rows < 1, a
 * pointer that is not 16-byte aligned, a handle of another device. */
int vqcpc_encoder_vq_bwd(vqcpc_encoder *enc, const float *z_pre, const float *z_q, int n_rows, const float *grad_z_st,
                         const float *grad_loss, float *grad_z_pre, void *stream);

/* ------------------------------------------------------------------ CPC scoring ------ */

/* CPCLoss.state_dict() (model.py:187-189): predictors.{i}.weight (z_dim, c_dim), predictors.{i}.bias (z_dim), DEVICE.
 * Only the first n_steps = n_prediction_steps / 2 predictors are ever used (model.py:181, :216), so only those are read.
 * Supported: z_dim == 64; c_dim 64, 128, 256 or 512; 1 <= n_steps <= 16; 1 <= n_negatives <= 64; n_speakers,
 * n_utterances >= 1 (n_speakers * n_utterances <= 65535). */
typedef struct {
    const float *weight[16], *bias[16];
    int n_steps, n_speakers, n_utterances, n_negatives, z_dim, c_dim;
} vqcpc_cpc_weights;

typedef struct vqcpc_cpc vqcpc_cpc;

/* Replaces CPCLoss.__init__ + load_state_dict (model.py:168-189; train_cpc.py:23-29).  Copies the predictors to the current
 * device (synchronises once). */
int vqcpc_cpc_create(const vqcpc_cpc_weights *w, vqcpc_cpc **out);
void vqcpc_cpc_destroy(vqcpc_cpc *cpc);

/* Replaces CPCLoss.forward (model.py:191-316) under no_grad: the forward VALUE of the objective (loss and per-step prediction
 * accuracies, what train_cpc.py:128-131 logs) -- checkpoint scoring; the gradient is vqcpc_cpc_grad's.
 * z DEVICE (N, T, z_dim), c DEVICE (N, T, c_dim), N = n_speakers * n_utterances utterances speaker-major, T >= n_steps + 2;
 * L = T - n_steps anchors per utterance.
 * Negatives: utt_index DEVICE (n_steps, Utt, Neg) int64 in [0, Utt) and seq_index DEVICE (n_steps, Spk, Utt, Neg, L) int64 in
 * [0, L) = the two index arrays of model.py:282 for every step (seq_index AFTER the remainder of model.py:272); or both NULL =
 * drawn in the kernel from (seed, stream_id) by the project's protocol (csrc/cpc_protocol.h, synth.cpc_negatives): the
 * reference draws them from torch's global CPU generator, which no device kernel can share.  The arithmetic is the same
 * either way.  Caller indices are CLAMPED into range on the device, silently: an out-of-range value cannot read out of
 * bounds, and it is the caller that rejects it (the Python wrapper raises IndexError before the call).
 * Outputs DEVICE: loss (1) = mean of step_loss (model.py:315); step_loss (n_steps) (model.py:305); accuracy (n_steps)
 * (model.py:307-308; a negative that ties the positive leaves the position correct, as argmax's first maximum does);
 * correct (n_steps, N, L) uint8 or NULL; scores (n_steps, N, 1 + Neg, L) fp32 = f of model.py:291 or NULL.
 * Sums run in a fixed order (no atomics): equal inputs give equal bits.  Enqueues on `stream`, does not synchronise. */
int vqcpc_cpc_score(vqcpc_cpc *cpc, const float *z, const float *c, int T, const int64_t *utt_index,
                    const int64_t *seq_index, uint64_t seed, uint32_t stream_id, float *loss, float *step_loss,
                    float *accuracy, uint8_t *correct, float *scores, void *stream);

/* vqcpc_cpc_score followed by the gradients of `loss` (upstream gradient 1) with respect to z, c and the first n_steps
 * predictors: the backward of CPCLoss.forward (what loss.backward() leaves in train_cpc.py:116), csrc/cpc_grad.hip.
 * z, c, T, the negatives (given or drawn), clamping, seed and stream_id, stream semantics and the device check are those of
 * vqcpc_cpc_score; loss, step_loss and accuracy have the BITS vqcpc_cpc_score gives for the same predictors.
 * W DEVICE (n_steps, 64, c_dim) and bias DEVICE (n_steps, 64): the predictors this call uses, stacked -- the caller's, so that an
 * optimizer step costs no new handle; both NULL = the handle's copies.  The handle gives sizes and work space only.
 * Gradients DEVICE, each may be NULL = not wanted (its launches are skipped): grad_z (N, T, 64), grad_c (N, T, c_dim), grad_W
 * (n_steps, 64, c_dim), grad_bias (n_steps, 64).  Every element is written, the zeros too (grad_z[:, 0], grad_c[:, L:]).
 * Every sum runs in one fixed order (no floating-point atomics; csrc/cpc_grad.hip lists the orders): equal inputs give equal
 * bits.  The work space lives on the handle and grows to the largest call.
 * VQCPC_ERR_INVALID before anything is enqueued: T < n_steps + 2, exactly one of W / bias NULL, exactly one index array NULL, a
 * handle of another device. */
int vqcpc_cpc_grad(vqcpc_cpc *cpc, const float *z, const float *c, int T, const float *W, const float *bias,
                   const int64_t *utt_index, const int64_t *seq_index, uint64_t seed, uint32_t stream_id, float *loss,
                   float *step_loss, float *accuracy, float *grad_z, float *grad_c, float *grad_W, float *grad_bias,
                   void *stream);

/* ------------------------------------------------------------------ ABX scoring ------ */

/* Own protocol (parity unpinned).  Stands in for the step the reference leaves to an outside package: README
 * 4-B "Run ABX evaluation script" on the per-frame text files that encode.py:48-52 writes.  The reference holds no ABX code and
 * no equality with any outside tool is claimed.
 *
 * Bytes of the `work` buffer of vqcpc_abx_score for n_frames frames of D components (the normalised copy of the frames). */
int vqcpc_abx_workspace_bytes(int n_frames, int D, uint64_t *bytes);

/* Own protocol; stands in for README 4-B's outside ABX script over the frames of encode.py:48-52.  Batched DTW distances between
 * tokens (runs of frames) and the integer ABX counts, for any number of blocks: one normalisation launch, one DTW launch, one
 * count launch on `stream`, no synchronisation, no atomics (equal inputs give equal bits).
 *
 * feats DEVICE (n_frames, D) fp32, 16-byte aligned.  Supported: D % 4 == 0, 4 <= D <= 512.  Each frame is normalised once (a
 * zero-norm frame stays zero); frame distance = 2 atan2(|u - v|, |u + v|) / pi in [0, 1], the angular distance arccos(cos) / pi
 * in a form that is exact 0 for bit-equal frames.  A zero frame is at 0.5 from every non-zero frame and at 0 from a zero frame.
 * Components are assumed to stay inside sqrt of the fp32 range (no rescaling before the squares).
 * tokens DEVICE (n_tokens, 2) int32 (first_row, n_frames), 1 <= n_frames <= 64 (T_MAX).
 * DTW: C[i][j] = d[i][j] + min(C[i-1][j-1], C[i-1][j], C[i][j-1]), predecessor = the first minimum in that order,
 * L[i][j] = L[pred] + 1, L[0][0] = 1; a pair's distance is C[Ta-1][Tb-1] / L[Ta-1][Tb-1].
 *
 * The block table: blocks DEVICE (n_blocks, 12) int32, one row per dense block
 *   [0] a_off   first entry in `lists` of the block's nA A/B token ids, sorted by phone
 *   [1] nA      [2] x_off  first entry in `lists` of its nX X token ids     [3] nX
 *   [4] seg_off first entry in `segs` of its n_seg + 1 ascending segment offsets into the A/B list (0 ... nA), one per phone
 *   [5] n_seg   [6] dist_base  first element of the block's (nA, nX) row-major tables in cost / path_len / dist
 *   [7] out_base  first element of its (nX, n_seg) table in twice_wins
 *   [8] xseg_off  first entry in `lists` of, per X token, the segment of its own phone
 *   [9] wg_base   sum over the earlier blocks of nX * ceil(nA / 4): the block's first workgroup of the DTW launch
 *   [10], [11]  0
 * out_base and wg_base ascend.  lists DEVICE (n_lists) int32, segs DEVICE (n_segs) int32.  HOST scalars: n_workgroups = the sum
 * that wg_base runs over, n_dist = sum nA * nX, n_out = sum nX * n_seg; each below 2^31 (cut larger work into several calls).
 * work DEVICE, vqcpc_abx_workspace_bytes(n_frames, D) bytes, 16-byte aligned.
 * Outputs DEVICE: cost (n_dist) fp32 or NULL, path_len (n_dist) int32 or NULL, dist (n_dist) fp32 = cost / path_len;
 * twice_wins (n_out) int32: for X token x of phone segment p and segment q != p,
 *   sum over a in segment p whose token id differs from x's, b in segment q of 2 [dist(a, x) < dist(b, x)] + [... == ...],
 * and 0 for q == p.
 * VQCPC_ERR_INVALID before anything is enqueued for whatever the host can see: D, the counts, NULL, alignment.  What lives in
 * DEVICE tables (token rows and lengths, list entries, offsets) is CLAMPED into range on the device, silently, and every store
 * is guarded by n_dist / n_out: a bad value cannot read or write out of bounds, and it is the caller that rejects it (the
 * Python wrapper raises before the call) -- the rule of vqcpc_cpc_score. */
int vqcpc_abx_score(const float *feats, int n_frames, int D, const int32_t *tokens, int n_tokens, const int32_t *lists,
                    int n_lists, const int32_t *segs, int n_segs, const int32_t *blocks, int n_blocks, int n_workgroups,
                    int64_t n_dist, int64_t n_out, void *work, float *cost, int32_t *path_len, float *dist,
                    int32_t *twice_wins, void *stream);

/* The index form of ABX scoring: the frames of quantised units are rows of a codebook, so a call's frame distances are M x M
 * values.  vqcpc_abx_code_table makes them once, vqcpc_abx_score_indices scores runs of indices with them (or, under the edit
 * metric, without them).
 *
 * Bytes of `work` (M * D * 4, the normalised codebook) plus `table` (M * M * 4) of vqcpc_abx_code_table. */
int vqcpc_abx_index_workspace_bytes(int M, int D, uint64_t *bytes);

/* codebook DEVICE (M, D) fp32, 1 <= M <= 4096, D % 4 == 0, 4 <= D <= 512 -> table DEVICE (M, M) fp32: table[i][j] = the frame
 * distance of vqcpc_abx_score between an A frame equal to row i and an X frame equal to row j, BIT FOR BIT (the same sums in the
 * same order, by the same device code), so index runs score exactly as their frames would.  Symmetric, 0 on the diagonal.
 * work DEVICE, M * D * 4 bytes.  codebook, work and table 16-byte aligned.  One normalisation launch and one table launch on
 * `stream`, no synchronisation.  VQCPC_ERR_INVALID before anything is enqueued for NULL, M, D and alignment. */
int vqcpc_abx_code_table(const float *codebook, int M, int D, void *work, float *table, void *stream);

/* metric of vqcpc_abx_score_indices */
#define VQCPC_ABX_ANGULAR 0 /* DTW over table[code_a][code_x]: cost, path_len, dist and twice_wins of vqcpc_abx_score on the frames */
#define VQCPC_ABX_EDIT 1    /* Levenshtein distance between the raw index runs (repeats are not collapsed) */

/* vqcpc_abx_score on runs of codebook indices: codes DEVICE (n_frames) int32 in [0, M), tokens (first_row, n_frames) as rows of
 * `codes`; lists, segs, blocks, the HOST scalars, the outputs and their layout are those of vqcpc_abx_score (same block table,
 * same workgroup numbering, a block lands where it lands there).  One DTW launch and the count launch of vqcpc_abx_score on
 * `stream`, no synchronisation, no atomics.
 * VQCPC_ABX_ANGULAR: table DEVICE (M, M) from vqcpc_abx_code_table, 16-byte aligned; a pair's tile is
 *   d[i][j] = table[code_a[i] * M + code_x[j]], then the DTW of vqcpc_abx_score: every output has the bits vqcpc_abx_score gives
 *   on feats[f] = codebook[codes[f]].
 * VQCPC_ABX_EDIT: table may be NULL, M only bounds the codes.  E(0, 0) = 0, E(i, 0) = i, E(0, j) = j,
 *   E(i, j) = min(E(i-1, j-1) + [a_i != x_j], E(i-1, j) + 1, E(i, j-1) + 1) on the INDICES (two equal codebook rows with
 *   different indices differ).  cost = E(Ta, Tb) (exact in fp32), path_len = max(Ta, Tb), dist = cost / path_len in [0, 1];
 *   fp32 division is correctly rounded, so equal ratios have equal bits and the counts' tie term is exact.
 * VQCPC_ERR_INVALID before anything is enqueued for NULL (table only under VQCPC_ABX_ANGULAR), M outside [1, 4096], the
 * counts, an unknown metric, a misaligned table.  What lives in DEVICE tables is clamped as in vqcpc_abx_score, codes into
 * [0, M): the caller rejects bad values (the Python wrapper raises IndexError before the call). */
int vqcpc_abx_score_indices(const float *table, int M, const int32_t *codes, int n_frames, const int32_t *tokens, int n_tokens,
                            const int32_t *lists, int n_lists, const int32_t *segs, int n_segs, const int32_t *blocks,
                            int n_blocks, int n_workgroups, int64_t n_dist, int64_t n_out, float *cost, int32_t *path_len,
                            float *dist, int32_t *twice_wins, void *stream, int metric);

/* ------------------------------------------------------------------ Vocoder ---------- */

/* Vocoder.state_dict(): own tables (network_vocoder.py:37-38) plus the RNN_MS core the
 * reference imports from the third-party `rnnms` package (network_vocoder.py:8, :39;
 * shapes from config.py:58-77, :198-199).  DEVICE pointers.
 * prenet: 2-layer bidirectional nn.GRU(dz+ds -> Hp), index [layer][direction];
 * ar: embedding (n_cls, de); nn.GRU(de + 2*Hp -> Hr) single layer, gate order r,z,n;
 * fc1 (Hf, Hr) + ReLU; fc2 (n_cls, Hf).
 * Supported: (dz + ds) % 32 == 0; Hp 64, 128 (the reference's), 256 or 512; Hr 512, 896 (the reference's) or 1024;
 * de % 32 == 0; Hf 256 (the reference's), 512, 768 or 1024; bits_mu_law 8 (the reference's), 9 or 10 with n_cls = 2^bits.
 * The resident decoders (`xcd`, `xcm`) exist for the reference's sizes (size_h_rnn 896 / size_h_fc 256 / 8-bit mu-law,
 * config.py:69,76-77); other sizes run on the launch-per-step kernels at about half the speed -- vqcpc_vocoder_last_path says which
 * loop a call ran. */
typedef struct {
    const float *code_embedding;      /* (n_codes, dz)           */
    const float *speaker_embedding;   /* (n_speakers, ds)        */
    const float *prenet_w_ih[2][2], *prenet_w_hh[2][2], *prenet_b_ih[2][2], *prenet_b_hh[2][2];
    const float *ar_embedding;        /* (n_cls, de)             */
    const float *ar_w_ih, *ar_w_hh, *ar_b_ih, *ar_b_hh;   /* (3Hr, de+2Hp), (3Hr, Hr), (3Hr) x2 */
    const float *fc1_weight, *fc1_bias, *fc2_weight, *fc2_bias;
    int n_codes, dz, n_speakers, ds, Hp, de, Hr, Hf, n_cls;
    int upsample_t;                   /* samples per conditioning frame (config.py:70 = hop 160) */
    int bits_mu_law;                  /* config.py:69 */
} vqcpc_vocoder_weights;

typedef struct vqcpc_vocoder vqcpc_vocoder;

/* Replaces Vocoder.__init__ + load_state_dict (network_vocoder.py:31-39; convert.py:33,45).
 * Accepted sizes (anything else: VQCPC_ERR_INVALID with a message that names the field):
 *   bits_mu_law            8 (config.py:69), 9, 10, with n_cls = 2^bits_mu_law
 *   Hf  = size_h_fc        256 (config.py:77), 512, 768, 1024
 *   Hr  = size_h_rnn       512, 896 (config.py:76), 1024
 *   Hp  = dim_voc_latent/2 64, 128 (config.py:68), 256, 512
 *   de  = size_i_embed_ar  any multiple of 32 (config.py:75: 256)
 *   dz + ds                any multiple of 32 (config.py:65-66: 64 + 64)
 *   upsample_t             any value > 0 (config.py:70: 160)
 *   n_codes, n_speakers    any value > 0
 * Every value of every list, and widths and hops from the smallest up, are checked against a float64 statement of the model
 * on every decode path they reach (tests/test_gpu_vocoder_sizes.py).  vqcpc_vocoder_nll additionally needs Hf 256 and 8 bits
 * (any listed Hr); the resident decoders need Hr 896, Hf 256 and 8 bits and take any de, Hp, dz + ds and upsample_t. */
int vqcpc_vocoder_create(const vqcpc_vocoder_weights *w, vqcpc_vocoder **out);
void vqcpc_vocoder_destroy(vqcpc_vocoder *voc);

/* Replaces Vocoder.generate (network_vocoder.py:69-78; callers convert.py:77,
 * vocoder.py:74-76).  idx DEVICE (B, Tc) int64 code indices; speaker DEVICE (B) int64;
 * n_codes HOST (B) per-utterance valid code counts, or NULL = all Tc (ragged batches:
 * utterance b produces 2*upsample_t*n_codes[b] samples, the rest of its row is zero).
 * Sampling protocol (project spec).  The reference draws x_t ~ Categorical(softmax(l_t)) from
 * torch's global CPU RNG, which ATen implements as an exponential race (argmax_k p_k / q_k,
 * q_k ~ Exp(1)); no device kernel can share that RNG stream, so the algorithm is kept and the
 * stream fixed: class k of sample t of utterance u (= utt_ids[b], HOST (B), or utt_base + b when
 * utt_ids is NULL -- an utterance's stream does not depend on how utterances are batched) uses
 * w = Philox4x32-10(counter = (t, u, k >> 2, 0), key = seed)[k & 3],
 * g_k = -log(-log(((w >> 9) + 0.5) * 2^-23)) (uniform exact in fp32, strictly inside (0, 1)), and x_t = first argmax_k (l_k + g_k).  Outputs DEVICE: wav (B, L) fp32 in [-1, 1] with
 * L = 2*upsample_t*Tc, mu-law decoded (preprocess.py:30-35); mulaw (B, L) int64 class
 * indices or NULL.  max_steps > 0 stops after that many samples (tests). */
int vqcpc_vocoder_generate(vqcpc_vocoder *voc, const int64_t *idx, const int64_t *speaker,
                           int B, int Tc, const int *n_codes, uint64_t seed, uint32_t utt_base,
                           const uint32_t *utt_ids, float *wav, int64_t *mulaw, int max_steps,
                           void *stream);

/* Streaming decode: the samples of vqcpc_vocoder_generate, chunk by chunk.  stream_open takes the arguments of generate (same
 * meaning; the utterance ids are fixed here) and runs the prenet over every utterance's full length (it is bidirectional, so all of
 * idx is needed up front); the stream keeps that conditioning and the decoder state itself, so generate() calls on the same handle
 * may run between chunks.  stream_next decodes samples [pos, pos + n_samples) of every utterance into DEVICE wav (B, n_samples)
 * fp32 and mulaw (B, n_samples) int64 or NULL (row stride n_samples; columns past an utterance's end are zero, as in generate) and
 * advances pos; n_samples > 0 and a multiple of upsample_t.  It sets vqcpc_vocoder_last_path / _last_slots / _last_timing like a
 * generate call, and returns VQCPC_ERR_INVALID once pos == total (2 * upsample_t * Tc).  The chunks concatenate to exactly the
 * samples of one generate call with the same seed and ids.  A chunk is checked like a call (vqcpc_vocoder_check after a sync);
 * stream_redo runs the last chunk again from the state it started from -- same samples -- e.g. after check reported that the
 * resident decoders' workgroups were not dealt 32 per XCD.  Chunks run on the per-XCD decoders (xcd) up to xcm_max utterances,
 * more than 32 back to back in their slots, never on the matrix-core form (xcm); otherwise, and for other dimensions, on the
 * launch-per-step kernels.  One chunk per stream in flight; close a stream before its vocoder is destroyed. */
typedef struct vqcpc_vocoder_stream vqcpc_vocoder_stream;
int vqcpc_vocoder_stream_open(vqcpc_vocoder *voc, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                              const int *n_codes, uint64_t seed, uint32_t utt_base, const uint32_t *utt_ids,
                              vqcpc_vocoder_stream **out, void *stream);
int vqcpc_vocoder_stream_next(vqcpc_vocoder_stream *st, int n_samples, float *wav, int64_t *mulaw, void *stream);
int vqcpc_vocoder_stream_redo(vqcpc_vocoder_stream *st, float *wav, int64_t *mulaw, void *stream);
int vqcpc_vocoder_stream_position(const vqcpc_vocoder_stream *st, int64_t *done, int64_t *total);
void vqcpc_vocoder_stream_close(vqcpc_vocoder_stream *st);

/* Replaces Vocoder.forward (network_vocoder.py:41-67; caller vocoder.py:62): teacher-forced
 * energies.  x DEVICE (B, Ts) int64 mu-law input samples, Ts <= 2*upsample_t*Tc;
 * logits DEVICE (B, Ts, n_cls) fp32.  Runs as a fused scan: with x given, only the GRU step is serial (one launch per
 * sample that also stores h_t); fc1 + ReLU and fc2 run as two batched GEMMs per chunk of steps. */
int vqcpc_vocoder_logits(vqcpc_vocoder *voc, const int64_t *x, const int64_t *idx,
                         const int64_t *speaker, int B, int Tc, int Ts, float *logits,
                         void *stream);

/* Teacher-forced scoring: the number the reference trains its vocoder on (vocoder.py:62-63: the energies of the inputs
 * audio[:, :-1] against the targets audio[:, 1:], cross-entropy), per utterance, for a padded batch of utterances of different
 * lengths.  audio DEVICE (B, L) int64 mu-law classes; n_audio HOST (B) valid samples per row or NULL = L; n_codes HOST (B) valid
 * codes per row or NULL = Tc.  Row b scores the positions t = 0 .. n_audio[b] - 2: input audio[b, t], target audio[b, t + 1]
 * (the shift is done inside); n_audio[b] - 1 <= 2 * upsample_t * n_codes[b], else VQCPC_ERR_INVALID; n_audio[b] < 2 scores
 * nothing (sum 0, count 0).  Nothing past n_audio[b] in a row is read.
 * Outputs DEVICE: nll_sum (B) fp64 = sum over the row's scored positions of lse(e_t) - e_t[target], in nats; n_scored (B) int64;
 * n_correct (B) int64 = positions whose target is the FIRST maximum of e_t (torch.argmax's rule); nll (B, L - 1) fp32 per
 * position, zero outside the scored ranges, or NULL.  sum(nll_sum) / sum(n_scored) over equal-length rows is the reference's
 * F.cross_entropy mean.
 * Runs the teacher-forced scan of vqcpc_vocoder_logits, but every chunk ends in ONE fused kernel (nll.hip: fc1 + ReLU, fc2,
 * log-sum-exp, gather, argmax) instead of two GEMMs: no (B, L, n_cls) energies exist anywhere, and no work buffer depends on L
 * (the scan's slot table is one row for the whole call).  The 256 terms of a log-sum-exp are added as a fixed tree and the per-utterance sums in step order, without atomics:
 * equal inputs give equal bits.  A class outside [0, n_cls) in a scored position is reported through the handle's status
 * word like a bad code index (vqcpc_vocoder_check).  Supported: size_h_fc 256 and 8-bit mu-law (the reference's).  Enqueues on
 * `stream`, does not synchronise. */
int vqcpc_vocoder_nll(vqcpc_vocoder *voc, const int64_t *audio, const int64_t *idx, const int64_t *speaker,
                      int B, int Tc, int L, const int *n_codes, const int *n_audio,
                      double *nll_sum, int64_t *n_scored, int64_t *n_correct, float *nll, void *stream);

/* ---- Vocoder gradients: the sample-rate network ---- */

/* The gradients of the vocoder objective (vocoder.py:62-63, F.cross_entropy of the teacher-forced energies of audio[:, :-1]
 * against audio[:, 1:]) through the sample-rate network rnnms.ar.* -- embedding, GRU, fc1, fc2 -- and with respect to the
 * conditioning series that feeds it.  The prenet and the two embedding tables in front of it are frozen here: grad_cond is where
 * their backward (vqcpc_vocoder_cond_bwd) starts.
 *
 * Every sum of these entries runs in one fixed order (vectorquantizedcpc_amd/csrc/vocoder_grad.hip states each), without
 * floating-point atomics: equal inputs give equal bits, whatever an earlier call left in the handle's work space.  That work
 * space is grow-only and counted by vqcpc_vocoder_workspace_bytes.
 *
 * Sizes: those vqcpc_vocoder_nll accepts -- size_h_fc 256, 256 classes, size_h_rnn 512, 896 or 1024, any size_i_embed_ar,
 * dim_voc_latent and upsampling_t vqcpc_vocoder_create accepts.  Below: n_cls = 256, Hf = 256, Hr = size_h_rnn,
 * de = size_i_embed_ar, C = dim_voc_latent. */

/* DEVICE pointers to the caller's nine tensors of rnnms.ar in the reference's shapes, fp32, 16-byte aligned: embedding (n_cls, de);
 * w_ih (3 Hr, de + C), w_hh (3 Hr, Hr), b_ih, b_hh (3 Hr), gate order r, z, n; fc1_weight (Hf, Hr), fc1_bias (Hf); fc2_weight
 * (n_cls, Hf), fc2_bias (n_cls).  Every member is required.  Where an entry takes `const vqcpc_vocoder_ar_weights *w`, NULL means
 * the handle's copies; with a struct the handle gives sizes, the frozen conditioning path (code and speaker embedding, prenet) and
 * work space only, and whatever re-layout the scan kernels need (the per-class and per-frame tables of the gates' input half, the
 * W_hh fragments) is made per call, in stream order, into work space the handle owns -- an optimizer step costs no new handle. */
typedef struct {
    const float *embedding;
    const float *w_ih;
    const float *w_hh;
    const float *b_ih;
    const float *b_hh;
    const float *fc1_weight;
    const float *fc1_bias;
    const float *fc2_weight;
    const float *fc2_bias;
} vqcpc_vocoder_ar_weights;

/* The gradients vqcpc_vocoder_ar_bwd writes: the members of the weights struct as DEVICE output pointers, same shapes, 16-byte
 * aligned.  A NULL member is not wanted and its launches are skipped.  Every element of a wanted tensor is written.  b_ih and b_hh
 * are both outputs: their gradients differ in the n third, where r multiplies the hidden half only. */
typedef struct {
    float *embedding;
    float *w_ih;
    float *w_hh;
    float *b_ih;
    float *b_hh;
    float *fc1_weight;
    float *fc1_bias;
    float *fc2_weight;
    float *fc2_bias;
} vqcpc_vocoder_ar_grads;

/* Bytes of the `saved` buffer that vqcpc_vocoder_ar_fwd fills for B utterances of L samples (its layout is private).
 * VQCPC_ERR_INVALID for NULL, B < 1 or L < 1, or a model the scoring head is not built for. */
int vqcpc_vocoder_ar_saved_bytes(vqcpc_vocoder *voc, int B, int L, uint64_t *bytes);

/* The forward of a training step.  audio, idx, speaker, B, Tc, L, n_codes, n_audio, nll_sum, n_scored, n_correct: those of
 * vqcpc_vocoder_nll, with its meaning and its conditions.  It is the same scan and the same head: with w == NULL the three
 * outputs have the bits of vqcpc_vocoder_nll for the same inputs, with a struct the bits of a handle created from those weights.
 * cond (B, 2 Tc, C) DEVICE fp32 or NULL: receives the conditioning rows the scan used (the prenet's output; rows past an
 * utterance's 2 n_codes[b] frames are +0).  saved (DEVICE, 16-byte aligned, vqcpc_vocoder_ar_saved_bytes) receives h_t of every
 * scored step.
 * Behind the valid data nothing is read, here and in the backward: of audio[b, :] the elements [0, n_audio[b]) where n_audio[b] >= 2
 * and none otherwise (step t < n_audio[b] - 1 is fed audio[b, t] and scored against audio[b, t + 1]), of idx[b, :] the elements
 * [0, n_codes[b]).  Whatever lies behind them -- a class or a code index outside its table included -- changes no bit of any output
 * and is not reported by vqcpc_vocoder_check.
 * VQCPC_ERR_INVALID before anything is enqueued: the NULL and range conditions of vqcpc_vocoder_nll, a NULL saved, a NULL member
 * of *w, a pointer that is not 16-byte aligned, a handle of another device. */
int vqcpc_vocoder_ar_fwd(vqcpc_vocoder *voc, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                         int L, const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, double *nll_sum,
                         int64_t *n_scored, int64_t *n_correct, float *cond, void *saved, void *stream);

/* The backward of vqcpc_vocoder_ar_fwd for the scalar loss = sum_b nll_sum[b] / N, N = sum_b max(n_audio[b] - 1, 0): the mean
 * over every scored sample of the batch (with equal lengths exactly F.cross_entropy's mean).  audio .. n_audio, w, saved: those
 * of the forward call (w's tensors unchanged since).  grad_loss: DEVICE fp32 scalar dL / dloss, NULL = 1.  1 / N is formed in
 * double on the host and rounded to fp32 once; the per-sample factor is s = grad_loss * (float)(1 / N).
 * grads: the wanted members receive dL / d(weight).  grad_cond (B, 2 Tc, C) DEVICE or NULL: dL / dcond; rows of frames that no
 * scored step of their utterance reads are +0.  Rows of grads->embedding for classes never fed are +0.
 * An utterance with n_audio[b] <= 1 contributes nothing.  The back-propagation through time of utterance b starts at its own last
 * scored step with dh = 0: a ragged batch equals its utterances run one at a time, in value.
 * VQCPC_ERR_INVALID before anything is enqueued: as the forward; N == 0; grads == NULL or without a wanted member while grad_cond
 * is NULL too. */
int vqcpc_vocoder_ar_bwd(vqcpc_vocoder *voc, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                         int L, const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w, const void *saved,
                         const float *grad_loss, const vqcpc_vocoder_ar_grads *grads, float *grad_cond, void *stream);

/* vqcpc_vocoder_ar_fwd and vqcpc_vocoder_ar_bwd with the conditioning series given: cond_in (B, T2, C) DEVICE, rows past an
 * utterance's frames not read.  The scan and the backward take their conditioning rows from it and do not run the prenet (idx and
 * speaker are not read); everything else is the statements of the two entries.  Given cond_in from
 * vqcpc_vocoder_cond_fwd with cw == NULL, every output -- the nine gradients and grad_cond among them -- has the bits of
 * vqcpc_vocoder_ar_fwd / _bwd.  VQCPC_ERR_INVALID: as those entries; a NULL or misaligned cond_in. */
int vqcpc_vocoder_ar_fwd_cond(vqcpc_vocoder *voc, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                              int L, const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w,
                              const float *cond_in, double *nll_sum, int64_t *n_scored, int64_t *n_correct, float *cond,
                              void *saved, void *stream);
int vqcpc_vocoder_ar_bwd_cond(vqcpc_vocoder *voc, const int64_t *audio, const int64_t *idx, const int64_t *speaker, int B, int Tc,
                              int L, const int *n_codes, const int *n_audio, const vqcpc_vocoder_ar_weights *w,
                              const float *cond_in, const void *saved, const float *grad_loss,
                              const vqcpc_vocoder_ar_grads *grads, float *grad_cond, void *stream);

/* ---- Vocoder gradients: the conditioning path ---- */

/* The gradients of the vocoder's conditioning path (network_vocoder.py:73-77 and rnnms.prenet: code_embedding,
 * speaker_embedding, the repeat of every code over two frames, the two bidirectional GRU layers) with respect to its eighteen
 * tensors, from any upstream gradient of the conditioning series -- vqcpc_vocoder_ar_bwd's grad_cond is one.  With the *_cond
 * forms of the scoring entries above, a step of the reference's vocoder trainer (vocoder.py:62-63) is vqcpc_vocoder_* calls from
 * the loss down to code_embedding.weight.
 *
 * Every DEVICE pointer of these entries is fp32 and 16-byte aligned, and VQCPC_ERR_INVALID is returned before anything is
 * enqueued.
 *
 * Every sum of these entries runs in one fixed order (vectorquantizedcpc_amd/csrc/prenet_grad.hip states each), without
 * floating-point atomics: equal inputs give equal bits, whatever an earlier call left in the handle's work space.  That work
 * space is grow-only and counted by vqcpc_vocoder_workspace_bytes.
 *
 * Below (and in the *_cond entries above): dz, ds = the two embedding widths, F = dz + ds, Hp = dim_voc_latent / 2, C = 2 Hp,
 * T2 = 2 Tc frames. */

/* DEVICE pointers to the caller's eighteen tensors of the conditioning path in the reference's shapes: code_embedding
 * (n_codes, dz), speaker_embedding (n_speakers, ds); of layer l and direction d (0 forward, 1 reverse) prenet_w_ih[l][d]
 * (3 Hp, F for l = 0, C for l = 1), prenet_w_hh[l][d] (3 Hp, Hp), prenet_b_ih[l][d], prenet_b_hh[l][d] (3 Hp), gate order
 * r, z, n.  Every member is required.  Where an entry takes `const vqcpc_vocoder_cond_weights *cw`, NULL means the handle's
 * copies; with a struct the handle gives sizes and work space only, and the stacked w_ih / b_ih / b_hh and the W_hh fragments
 * the scan reads are made per call, in stream order, into work space the handle owns -- an optimizer step costs no new handle. */
typedef struct {
    const float *code_embedding;
    const float *speaker_embedding;
    const float *prenet_w_ih[2][2];
    const float *prenet_w_hh[2][2];
    const float *prenet_b_ih[2][2];
    const float *prenet_b_hh[2][2];
} vqcpc_vocoder_cond_weights;

/* The gradients vqcpc_vocoder_cond_bwd writes: the same members as DEVICE output pointers, same shapes.  A NULL member is not
 * wanted and its launches are skipped.  Every element of a wanted tensor is written; rows of the two tables that the batch
 * never names are +0. */
typedef struct {
    float *code_embedding;
    float *speaker_embedding;
    float *prenet_w_ih[2][2];
    float *prenet_w_hh[2][2];
    float *prenet_b_ih[2][2];
    float *prenet_b_hh[2][2];
} vqcpc_vocoder_cond_grads;

/* Bytes of the `saved` buffer that vqcpc_vocoder_cond_fwd fills for B utterances of Tc codes (its layout is private).
 * VQCPC_ERR_INVALID for NULL, B < 1 or Tc < 1. */
int vqcpc_vocoder_cond_saved_bytes(vqcpc_vocoder *voc, int B, int Tc, uint64_t *bytes);

/* The conditioning series of a training step: glue, prenet layer 0, prenet layer 1 -- the statements of
 * vqcpc_vocoder_condition.  idx (B, Tc) and speaker (B) DEVICE int64; n_codes: HOST, valid codes per utterance in [0, Tc], NULL =
 * Tc.  cond (B, T2, C) DEVICE receives the series; rows past an utterance's 2 n_codes[b] frames are +0.  With cw == NULL its bits
 * equal vqcpc_vocoder_condition's (n_codes NULL) and the cond output of vqcpc_vocoder_ar_fwd; with a struct the bits of a handle
 * created from those tensors.  saved (DEVICE, 16-byte aligned, vqcpc_vocoder_cond_saved_bytes) receives what the backward reads
 * again: the glued series and both layers' outputs, over the utterances' own frames.  An index outside its table is clamped for
 * the read and reported by vqcpc_vocoder_check.  Of idx[b, :] the forward and the backward read the elements [0, n_codes[b]) and
 * nothing behind them: an index there, inside its table or not, changes no bit of any output and is not reported.
 * VQCPC_ERR_INVALID before anything is enqueued: a NULL argument (cw excepted), a NULL member of *cw, a pointer that is not
 * 16-byte aligned, B < 1 or Tc < 1, n_codes[b] outside [0, Tc], a handle of another device. */
int vqcpc_vocoder_cond_fwd(vqcpc_vocoder *voc, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes,
                           const vqcpc_vocoder_cond_weights *cw, float *cond, void *saved, void *stream);

/* The backward of vqcpc_vocoder_cond_fwd for L = sum(cond * grad_cond) over the utterances' own frames.  idx .. cw, saved: those
 * of the forward call (cw's tensors unchanged since).  grad_cond (B, T2, C) DEVICE: any upstream gradient; rows past an
 * utterance's frames are not read.  The wanted members of *grads receive dL / d(tensor).  The back-propagation through time of
 * utterance b runs over its own 2 n_codes[b] frames, each direction from its own last step with dh = 0: a ragged batch equals
 * its utterances run one at a time, in value.
 * VQCPC_ERR_INVALID before anything is enqueued: as the forward; grads NULL or without a wanted member. */
int vqcpc_vocoder_cond_bwd(vqcpc_vocoder *voc, const int64_t *idx, const int64_t *speaker, int B, int Tc, const int *n_codes,
                           const vqcpc_vocoder_cond_weights *cw, const void *saved, const float *grad_cond,
                           const vqcpc_vocoder_cond_grads *grads, void *stream);

/* ---- Vocoder: stage outputs, options, status ---- */

/* The wrapper's own glue alone (network_vocoder.py:73-77 / :56-66): series DEVICE (B, 2*Tc, dz + ds) = what the reference's
 * Vocoder.generate / Vocoder.forward hand to rnnms -- [:, :, :dz] the code embedding of code t/2, [:, :, dz:] the speaker
 * embedding.  The same kernel vqcpc_vocoder_generate / _logits / _condition run first; exposed so that it can be checked
 * against the fixture captured from the reference (tests/golden/vocoder_glue.npz). */
int vqcpc_vocoder_glue(vqcpc_vocoder *voc, const int64_t *idx, const int64_t *speaker, int B, int Tc, float *series,
                       void *stream);

/* Conditioning series after the prenet, (B, 2*Tc, 2*Hp) DEVICE -- stage-level tests. */
int vqcpc_vocoder_condition(vqcpc_vocoder *voc, const int64_t *idx, const int64_t *speaker,
                            int B, int Tc, float *cond, void *stream);

/* Decode-loop options.
 * fuse_fc2 (default 1): in calls of up to 4 utterance tiles (64 decode slots per tile group) the fc2 + draw of sample t-1
 * and the GRU step of sample t share ONE launch -- W_hh h does not depend on the drawn sample, so it runs while the fc2
 * workgroups of the same launch produce the candidates, which the GRU's gate waves then pick up through 8-byte granules.
 * Two launches per sample instead of three; same bits.  A wait that ever times out (0.25 s) sets the handle's status word
 * (vqcpc_vocoder_check).
 * xcd (default -1 = auto: up to xcm_min utterances in flight; 0 never, also turns xcm off; 1 whenever the dimensions are
 * the reference's): generate() runs as EIGHT resident,
 * weight-stationary decoders, one per XCD (ar_xcd.hip): decode slot s lives on XCD s % 8; each XCD keeps a full copy of the
 * recurrent weights on its 32 CUs (W_hh in VGPRs, fc1 / fc2 / the sample-embedding table in LDS) and exchanges h_t, a_t and
 * the draw candidates through its own L2; no launches per sample.  Same samples as every other path.  xcd_slots: decode
 * slots it may use (default and maximum 32); more utterances than slots run back to back in them (longest first).
 * xcm (default -1 = auto: more than xcm_min (68) and fewer than xcm_max (512) utterances in flight; 0 never; 1 whenever the
 * dimensions are the reference's): the same resident decoders with 16 decode slots per XCD on the matrix cores
 * (ar_xcm.hip): [W_hh; W_fc1] h_t as six v_mfma_f32_16x16x4_f32 tiles per workgroup, A fragments pinned in registers.
 * xcm_slots: decode slots it may use (default and maximum 128).  Same samples as every other path; shares xcd's timeout,
 * debug-drop and agent-store options and its status word.
 * The resident decoders (xcd, xcm) assume the GPU is theirs for the call: ONE launch of 256 workgroups (768 threads, ~150 KB of
 * LDS each: one per CU) that must all be resident, 32 on each XCD, within xcd_timeout_ms -- checked in-kernel, not assumed.
 * On a GPU shared with another process or stream the placement can miss: the launch then writes nothing and reports it
 * (vqcpc_vocoder_check: "not dealt 32"), the handle keeps its options and the caller repeats the call; only a second miss in a
 * row switches the resident decoders off for the handle.  A hand-off TIMEOUT inside a launch switches them off at once; the
 * handle re-arms itself after 16 clean calls, or when xcd / fuse_fc2 is set again.
 * xcd_agent_stores / xcd_timeout_ms / xcd_debug_drop_step, handoff_timeout_ms / handoff_debug_drop_step: A-B and tests
 * of the abort path (one worker skips a publish at that step; the waits give up after the timeout; vqcpc_vocoder_check).
 * xcd_debug_misplace (one shot): workgroup 0 of the next resident launch reports the XCD next to its own, so that the placement
 * check fails (tests of the "not dealt 32" path).
 * tf_chunk_replays: graph replays per chunk of the teacher-forced scan (vqcpc_vocoder_logits; default 4).
 * use_graph: replay the per-sample kernels from a captured hipGraph
 * (default 1) instead of launching them one by one.  steps_per_graph: samples per replay (even).
 * slots: continuous batching -- decode with this many slots, each running utterances back to back
 * (0 = one slot per utterance).  big_min_tiles: utterance tiles (of 16) from which the LDS-staged
 * large-batch GRU kernel is used (default 5, 0 = never).  two_groups: run calls of 3..big_min_tiles-1
 * tiles, or of >= 2*big_min_tiles tiles, as two independent tile groups on two streams (default 1). */
int vqcpc_vocoder_set_option(vqcpc_vocoder *voc, const char *name, int value);

/* After the caller has synchronised the stream that carried vqcpc_vocoder_generate: did an in-kernel hand-off of a call
 * since the last check (per-XCD decoders, fused fc2 || GRU launch) time out, or were the per-XCD decoders' workgroups not
 * dealt 32 to each XCD?  VQCPC_OK, or VQCPC_ERR_HIP: the waveform of that call is incomplete (or was not written at all) and
 * the call should be repeated -- the repeat gives the same samples the fast path would have (the sampling stream does not
 * depend on the path); the message names the call (the resident decoders tag the status word with the handle's call count)
 * and says whether the handle has switched its in-kernel hand-offs off (see the options).  Reads a host-mapped word: no HIP
 * call.  Without the synchronisation the word of a call still running reads zero: the next vqcpc_vocoder_generate on the
 * handle looks at it again (and reports what it finds) but clears nothing.  convert.py:75-83 writes the wav right after
 * generate(): the Python Vocoder.generate checks (and repeats once) by default; driver.convert_utterances, cli.convert and
 * shard.convert_sharded go through it before anything is written or gathered. */
int vqcpc_vocoder_check(vqcpc_vocoder *voc);

/* Which decode loop the last generate()/logits() call on the handle ran (measurement and tests; the samples do not depend
 * on it): 0 = launch-per-step kernels (more than 511 utterances in flight, dimensions other than the reference's 896 / 256 /
 * 8 bits, teacher-forced calls, the fallback), 2 = the per-XCD resident decoders, 3 = their matrix-core form (16 slots per XCD);
 * 1 = no decode loop has run yet; -1 = null handle. */
int vqcpc_vocoder_last_path(vqcpc_vocoder *voc);

/* Which decode loop a call of B utterances producing n_samples[b] samples each would take under these options (the arguments
 * mirror vqcpc_vocoder_set_option: xcd, xcm -1 / 0 / 1; xcm_min, xcm_max, xcd_slots, xcm_slots <= 0 = the defaults 68, 512, 32,
 * 128; slots 0 = one per utterance), for the reference's dimensions: *path as vqcpc_vocoder_last_path, *slots_used, and *longest =
 * the longest back-to-back schedule of a resident decode slot in samples.  Pure host arithmetic (no GPU): the rule
 * vqcpc_vocoder_generate applies.  A slot's schedule must stay below 2^24 - 1 samples for the resident decoders; in auto mode
 * such a call takes the launch path, with xcd / xcm = 1 it is VQCPC_ERR_INVALID. */
int vqcpc_vocoder_plan(int xcd, int xcm, int xcm_min, int xcm_max, int xcd_slots, int xcm_slots, int slots,
                       const int *n_samples, int B, int *path, int *slots_used, int64_t *longest);

/* Decode slots the last call's loop ran through (per-XCD decoders: at most 32; matrix-core form: at most 128; launch path:
 * the `slots` option or one per utterance); -1 = null handle. */
int vqcpc_vocoder_last_slots(vqcpc_vocoder *voc);

/* Device memory the handle's grow-only work buffers hold at the moment (conditioning rows, schedules, exchange areas, ...:
 * the peak of the calls so far; the weights are not counted). */
int vqcpc_vocoder_workspace_bytes(vqcpc_vocoder *voc, uint64_t *bytes);

/* Device time, in milliseconds, of the whole decode loop of the last generate()/logits() call
 * (HIP events on the launch stream) and the number of samples per utterance it covers.
 * Valid after the stream has been synchronised. */
int vqcpc_vocoder_last_timing(vqcpc_vocoder *voc, float *loop_ms, int *n_steps);

/* ------------------------------------------------------------------ Mel front-end ---- */

/* Replaces wave_to_mel (preprocess.py:53-75; convert.py:54-70 is the same sequence): peak-normalise
 * to 0.999, pre-emphasis (preprocess.py:16-17), centred STFT magnitude (periodic Hann `win`
 * zero-padded to n_fft, reflect padding: librosa ^0.8), Slaney mel filterbank from fmin to sr/2,
 * amplitude_to_db with top_db against the utterance maximum, / top_db + 1.  Defaults of the
 * reference: config.py:103-112 (16000, 2048, 80, 160, 400, 50, 0.97, 80). */
typedef struct vqcpc_melfront vqcpc_melfront;
int vqcpc_melfront_create(int sr, int n_fft, int n_mels, int hop, int win, float fmin, float preemph,
                          float top_db, vqcpc_melfront **out);
void vqcpc_melfront_destroy(vqcpc_melfront *f);
/* Frames of an n_samples utterance: 1 + n_samples / hop (centred STFT). */
int vqcpc_melfront_frames(const vqcpc_melfront *f, int n_samples);
/* wav DEVICE (B, Lmax) fp32, lens HOST (B) valid samples; mel DEVICE (B, n_mels, 1 + Lmax/hop) --
 * the encoder's input layout; frames past an utterance's own length are zero. */
int vqcpc_melfront_run(vqcpc_melfront *f, const float *wav, const int *lens, int B, int Lmax, float *mel,
                       void *stream);

/* ------------------------------------------------------------------ Resampling ---- */

/* Replaces the resampling inside librosa.load(path, sr=cfg.preprocessing.sr) (convert.py:54-56): librosa ^0.8's
 * res_type "kaiser_best" = resampy's band-limited sinc interpolation (64 zero crossings, 512 table entries per crossing,
 * Kaiser taper, linear interpolation between entries), fp64 arithmetic, fp32 result.  resampy is absent offline: parity
 * unpinned (oracle/resample_ref.py restates the algorithm and its published constants). */
typedef struct vqcpc_resampler vqcpc_resampler;
int vqcpc_resampler_create(int sr_in, int sr_out, vqcpc_resampler **out);
void vqcpc_resampler_destroy(vqcpc_resampler *r);
/* Output samples of an n_in-sample signal: ceil(n_in * sr_out / sr_in), as librosa.resample(fix=True). */
int vqcpc_resampler_out_len(const vqcpc_resampler *r, int n_in);
/* wav_in DEVICE (B, Lin_max) fp32, lens_in HOST (B) valid samples; wav_out DEVICE (B, Lout_max) fp32 with
 * Lout_max >= vqcpc_resampler_out_len(max lens_in): row b holds its utterance's resampled samples, zeros behind them.
 * Does not synchronise (the lengths travel as kernel arguments), except when a call needs a longer output-clock table than
 * any before it on this handle. */
int vqcpc_resampler_run(vqcpc_resampler *r, const float *wav_in, const int *lens_in, int B, int Lin_max,
                        float *wav_out, int Lout_max, void *stream);

/* ------------------------------------------------------------------ Loudness ---- */

/* Replaces pyloudnorm.Meter(sr) (convert.py:50) for mono audio: ITU-R BS.1770-4 gated integrated
 * loudness as pyloudnorm ^0.1.0 computes it (K-weighting biquads derived at `rate`, 400 ms blocks with
 * 75 % overlap, gates at -70 LUFS absolute and -10 LU relative).  fp64 on the device. */
typedef struct vqcpc_loudness vqcpc_loudness;
int vqcpc_loudness_create(int rate, vqcpc_loudness **out);
void vqcpc_loudness_destroy(vqcpc_loudness *m);
/* Gating blocks of an n_samples signal; 0 when it is shorter than one block (the meter refuses it). */
int vqcpc_loudness_blocks(const vqcpc_loudness *m, int n_samples);
/* meter.integrated_loudness (convert.py:57, :79) of B padded mono signals.  wav DEVICE (B, Lmax) fp32,
 * lens HOST (B); lufs DEVICE (B) fp64 (-inf when every block is gated out); block_energy DEVICE
 * (sum of vqcpc_loudness_blocks(lens[b])) fp64 or NULL.  VQCPC_ERR_INVALID when an utterance is shorter
 * than one block (pyloudnorm raises ValueError).  Synchronises `stream` once (host length tables). */
int vqcpc_loudness_integrated(vqcpc_loudness *m, const float *wav, const int *lens, int B, int Lmax, double *lufs,
                              double *block_energy, void *stream);
/* pyloudnorm.normalize.loudness (convert.py:80), in place: wav[b] *= 10^((target[b] - measured[b]) / 20),
 * product in fp64 rounded to fp32.  measured / target DEVICE (B) fp64. */
int vqcpc_loudness_normalize(vqcpc_loudness *m, float *wav, const int *lens, int B, int Lmax, const double *measured,
                             const double *target, void *stream);

/* Average wall time, in microseconds, of `reps` back-to-back launches of each per-sample kernel
 * of the decode loop on the state the last generate()/logits() call left (HIP events on
 * `stream`; synchronises it).  out_us[5] = {GRU step, fc1, fc2 + draw, decode slots one launch
 * covers (a call of 33..80 or >= 192 utterances runs as two independent tile groups), which GRU-step
 * kernel that is: 0 = one tile, 1 = two tiles per workgroup, 2 = LDS-staged large-batch kernel; 4 / 5 = the fused launch
 * (fc2 + draw of the previous sample in front of the GRU step) on the small / the large-batch kernel -- out_us[2] is then
 * fc2 as a launch of its own, for reference}.
 * Each time includes this chip's ~1.5 us dependent-launch boundary. */
int vqcpc_vocoder_kernel_times(vqcpc_vocoder *voc, int reps, float *out_us, void *stream);

/* ------------------------------------------------------------------ Optimizer step ---- */

/* The parameter update.  With the gradient entries above, a training step of either reference trainer (train_cpc.py:116-124,
 * vocoder.py:62-63) is vqcpc_* calls from the loss to the new parameters: the gradients come from the *_bwd / *_grad entries,
 * vqcpc_adam_step applies them.
 *
 * DEVICE pointers are fp32 and 16-byte aligned, and VQCPC_ERR_INVALID is returned before anything is enqueued.  There is no
 * handle: the entry allocates nothing, keeps nothing and copies nothing to the device -- the table of tensors travels in the
 * kernel arguments.
 *
 * The update is Adam as torch.optim.Adam runs it with its defaults (no weight decay, no amsgrad, no maximize), in ONE stated
 * order of fp32 operations.  Per element, with g the gradient, m = exp_avg, v = exp_avg_sq, p the parameter:
 *
 *     m' = m + (g - m) * w1
 *     v' = v * c2 + (g * g) * w2
 *     d  = sqrt(v') / rb + e
 *     p' = p - ss * (m' / d)
 *
 * Every operation is one IEEE fp32 operation rounded to nearest even, once; nothing is contracted into a fused multiply-add; the
 * square root and the two divisions are the correctly rounded ones.  The six scalars are formed in double on the host from the
 * hyper-parameters of update number t = step and rounded to fp32 once each:
 *
 *     w1 = 1 - beta1      c2 = beta2      w2 = 1 - beta2      rb = sqrt(1 - beta2^t)      e = eps      ss = lr / (1 - beta1^t)
 *
 * (beta^t is the C library's pow(beta, (double)t).)  Equal inputs give equal bits, whatever the list's split into launches.
 * Denormal g * g or v are outside the contract: keep |g| >= 1e-15 or exactly 0.
 * An element whose g * g overflows (|g| above about 1.8e19), or whose g is infinite or NaN, follows IEEE arithmetic in the stated
 * order: an overflow freezes that element's p -- v' = inf, so d = inf and m' / d = 0 -- for as long as its exp_avg_sq stays
 * infinite; an infinite or NaN g makes its p NaN.  No other element of the call is affected.  Nothing is detected or reported. */

/* One tensor of the update: four DEVICE buffers of numel fp32 elements each.  param, exp_avg and exp_avg_sq are read and
 * written, grad is read.  With numel == 0 the tensor is skipped and its pointers are not looked at.  The buffers of one call
 * must not overlap, neither within a tensor nor between tensors: every element is read and written by exactly one thread of one
 * launch, and nothing orders two tensors of a call. */
typedef struct { float *param; const float *grad; float *exp_avg; float *exp_avg_sq; uint64_t numel; } vqcpc_adam_tensor;

/* The hyper-parameters of one update.  step: the number of THIS update, >= 1 (the first update of a fresh state is 1). */
typedef struct { double lr, beta1, beta2, eps; int64_t step; } vqcpc_adam_hyper;

/* Tensors one launch covers (the four pointers, numel and a chunk prefix per tensor, by value, within the 4 KiB of kernel
 * arguments), and the elements one workgroup covers.  A list of n tensors takes ceil(n / VQCPC_ADAM_TABLE) launches, in list
 * order; a workgroup finds its tensor by searching the chunk prefix. */
#define VQCPC_ADAM_TABLE 72
#define VQCPC_ADAM_CHUNK 4096

/* One Adam update of n_tensors tensors with the hyper-parameters *h, as stated at the head of this section.  tensors and h are
 * HOST memory, read before the call returns.  Enqueues ceil(n_tensors / VQCPC_ADAM_TABLE) launches on `stream` and nothing else.
 * VQCPC_ERR_INVALID before anything is enqueued: tensors or h NULL; n_tensors < 1; a NULL or not 16-byte aligned member of a
 * tensor with numel > 0; step < 1; lr or eps not finite or negative; a beta outside [0, 1); memory of the first tensor with
 * numel > 0 that does not belong to the current device.  VQCPC_ERR_NO_DEVICE: the current device is not a gfx950. */
int vqcpc_adam_step(const vqcpc_adam_tensor *tensors, int n_tensors, const vqcpc_adam_hyper *h, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VQCPC_H */
