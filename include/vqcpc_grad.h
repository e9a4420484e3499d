/*
 * vqcpc_grad.h -- C ABI of libvqcpc_hip.so, second header: the gradients of the encoder's front end (Conv1d / LayerNorm /
 * Linear, model.py:43-55, :65-67) and of the VQ step's straight-through estimator (model.py:147-150).  Together with
 * vqcpc_cpc_grad and vqcpc_encoder_context_bwd of vqcpc.h they are loss.backward() of the reference's training step
 * (train_cpc.py:116-124), from the loss down to conv.weight.
 *
 * Why a header of its own: tests/test_gpu_stream_contract.py reads vqcpc.h and requires the set of its entries that take a
 * `stream` to equal its own table.  The entries below take a stream; they are held to the same contract, with the same
 * harness, by tests/test_gpu_front_grad_stream.py, which keeps the table of THIS header.  Merging the two tables -- and then the
 * two headers -- is left to a change that may edit that test.
 *
 * Conventions: those of vqcpc.h (DEVICE pointers are contiguous fp32 memory on the current HIP device, borrowed for the duration
 * of the enqueued work; all work is enqueued on `stream`, nothing synchronises; 0 on success, a negative vqcpc_status otherwise,
 * vqcpc_last_error() has the message; one stream at a time per handle).  The symbols are exported by the same library.
 *
 * Every sum of these entries runs in one fixed order (vectorquantizedcpc_amd/csrc/front_grad.hip states each), without
 * floating-point atomics: equal inputs give equal bits, whatever an earlier call left in the handle's work space.  That work
 * space is grow-only and counted by vqcpc_encoder_workspace_bytes.
 */
#ifndef VQCPC_GRAD_H
#define VQCPC_GRAD_H

#include "vqcpc.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* VQCPC_GRAD_H */
