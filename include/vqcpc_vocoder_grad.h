/*
 * vqcpc_vocoder_grad.h -- C ABI of libvqcpc_hip.so, third header: the gradients of the vocoder objective (vocoder.py:62-63,
 * F.cross_entropy of the teacher-forced energies of audio[:, :-1] against audio[:, 1:]) through the sample-rate network
 * rnnms.ar.* -- embedding, GRU, fc1, fc2 -- and with respect to the conditioning series that feeds it.  The prenet and the two
 * embedding tables in front of it are frozen here: grad_cond is where their backward (vqcpc_vocoder_cond_grad.h) starts.
 *
 * Why a header of its own: tests/test_gpu_stream_contract.py and tests/test_gpu_front_grad_stream.py each require the set of
 * stream-taking entries of ONE header (vqcpc.h, vqcpc_grad.h) to equal their own table.  The entries below take a stream; they
 * are held to the same contract, with the same harness, by tests/test_gpu_voc_grad_stream.py, which keeps the table of THIS
 * header.
 *
 * Conventions: those of vqcpc.h (DEVICE pointers are contiguous memory on the current HIP device, borrowed for the duration of the
 * enqueued work; all work is enqueued on `stream`, nothing synchronises; 0 on success, a negative vqcpc_status otherwise,
 * vqcpc_last_error() has the message; one stream at a time per handle).  The symbols are exported by the same library.
 *
 * Every sum of these entries runs in one fixed order (vectorquantizedcpc_amd/csrc/vocoder_grad.hip states each), without
 * floating-point atomics: equal inputs give equal bits, whatever an earlier call left in the handle's work space.  That work
 * space is grow-only and counted by vqcpc_vocoder_workspace_bytes.
 *
 * Sizes: those vqcpc_vocoder_nll accepts -- size_h_fc 256, 256 classes, size_h_rnn 512, 896 or 1024, any size_i_embed_ar,
 * dim_voc_latent and upsampling_t vqcpc_vocoder_create accepts.  Below: n_cls = 256, Hf = 256, Hr = size_h_rnn,
 * de = size_i_embed_ar, C = dim_voc_latent.
 */
#ifndef VQCPC_VOCODER_GRAD_H
#define VQCPC_VOCODER_GRAD_H

#include "vqcpc.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* VQCPC_VOCODER_GRAD_H */
