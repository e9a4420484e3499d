/*
 * vqcpc_vocoder_cond_grad.h -- C ABI of libvqcpc_hip.so, fourth header: the gradients of the vocoder's conditioning path
 * (network_vocoder.py:73-77 and rnnms.prenet: code_embedding, speaker_embedding, the repeat of every code over two frames, the
 * two bidirectional GRU layers) with respect to its eighteen tensors, from any upstream gradient of the conditioning series --
 * vqcpc_vocoder_ar_bwd's grad_cond is one.  With the *_cond forms of the scoring entries below, a step of the reference's vocoder
 * trainer (vocoder.py:62-63) is vqcpc_vocoder_* calls from the loss down to code_embedding.weight.
 *
 * Why a header of its own: each stream-contract test requires the set of stream-taking entries of ONE header to equal its own
 * table; tests/test_gpu_cond_grad_stream.py keeps the table of THIS header.
 *
 * Conventions: those of vqcpc.h (DEVICE pointers are contiguous memory on the current HIP device, fp32, 16-byte aligned, borrowed
 * for the duration of the enqueued work; all work is enqueued on `stream`, nothing synchronises; 0 on success, a negative
 * vqcpc_status otherwise, vqcpc_last_error() has the message; VQCPC_ERR_INVALID is returned before anything is enqueued; one stream
 * at a time per handle).  The symbols are exported by the same library.
 *
 * Every sum of these entries runs in one fixed order (vectorquantizedcpc_amd/csrc/prenet_grad.hip states each), without
 * floating-point atomics: equal inputs give equal bits, whatever an earlier call left in the handle's work space.  That work
 * space is grow-only and counted by vqcpc_vocoder_workspace_bytes.
 *
 * Below: dz, ds = the two embedding widths, F = dz + ds, Hp = dim_voc_latent / 2, C = 2 Hp, T2 = 2 Tc frames.
 */
#ifndef VQCPC_VOCODER_COND_GRAD_H
#define VQCPC_VOCODER_COND_GRAD_H

#include "vqcpc_vocoder_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

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

#ifdef __cplusplus
}
#endif
#endif /* VQCPC_VOCODER_COND_GRAD_H */
