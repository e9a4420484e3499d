/*
 * vqcpc_optim.h -- C ABI of libvqcpc_hip.so, fifth header: the parameter update.  With the gradient entries of vqcpc.h
 * (vqcpc_cpc_grad, vqcpc_encoder_context_bwd), vqcpc_grad.h, vqcpc_vocoder_grad.h and vqcpc_vocoder_cond_grad.h, a training step
 * of either reference trainer (train_cpc.py:116-124, vocoder.py:62-63) is vqcpc_* calls from the loss to the new parameters: the
 * gradients come from the *_bwd / *_grad entries, vqcpc_adam_step applies them.
 *
 * Why a header of its own: each stream-contract test requires the set of stream-taking entries of ONE header to equal its own
 * table; tests/test_gpu_adam_stream.py keeps the table of THIS header.
 *
 * Conventions: those of vqcpc.h (DEVICE pointers are contiguous memory on the current HIP device, fp32, 16-byte aligned, borrowed
 * for the duration of the enqueued work; all work is enqueued on `stream`, nothing synchronises; 0 on success, a negative
 * vqcpc_status otherwise, vqcpc_last_error() has the message; VQCPC_ERR_INVALID is returned before anything is enqueued).  The
 * symbols are exported by the same library.  There is no handle: the entry allocates nothing, keeps nothing and copies nothing
 * to the device -- the table of tensors travels in the kernel arguments.
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
 * infinite; an infinite or NaN g makes its p NaN.  No other element of the call is affected.  Nothing is detected or reported.
 */
#ifndef VQCPC_OPTIM_H
#define VQCPC_OPTIM_H

#include "vqcpc.h"

#ifdef __cplusplus
extern "C" {
#endif

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

/* One Adam update of n_tensors tensors with the hyper-parameters *h, as stated at the top of this file.  tensors and h are HOST
 * memory, read before the call returns.  Enqueues ceil(n_tensors / VQCPC_ADAM_TABLE) launches on `stream` and nothing else.
 * VQCPC_ERR_INVALID before anything is enqueued: tensors or h NULL; n_tensors < 1; a NULL or not 16-byte aligned member of a
 * tensor with numel > 0; step < 1; lr or eps not finite or negative; a beta outside [0, 1); memory of the first tensor with
 * numel > 0 that does not belong to the current device.  VQCPC_ERR_NO_DEVICE: the current device is not a gfx950. */
int vqcpc_adam_step(const vqcpc_adam_tensor *tensors, int n_tensors, const vqcpc_adam_hyper *h, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VQCPC_OPTIM_H */
