// optim.h -- what optim.hip (the kernel and the C entry) and optim_plan.hip (the host arithmetic of the entry) share.
#pragma once
#include "common.h"

// The six fp32 scalars of one update, formed in double and rounded once each (include/vqcpc.h states them).
struct AdamScalars { float w1, c2, w2, rb, e, ss; };

// One launch's table, passed BY VALUE as a kernel argument: per tensor the four pointers, numel and a chunk prefix.  Tensor i
// owns the workgroups [first[i], first[i + 1]); workgroup first[i] + c covers its elements [c CHUNK, min((c + 1) CHUNK, numel)).
struct AdamTable {
    float *p[VQCPC_ADAM_TABLE];
    const float *g[VQCPC_ADAM_TABLE];
    float *m[VQCPC_ADAM_TABLE];
    float *v[VQCPC_ADAM_TABLE];
    uint64_t numel[VQCPC_ADAM_TABLE];
    uint32_t first[VQCPC_ADAM_TABLE + 1];
    int n;
};
static_assert(sizeof(AdamTable) + sizeof(AdamScalars) <= 4096, "the table must fit the kernel-argument segment");

// A launch's grid stays below this many workgroups (the x dimension of a grid is 31 bits).
constexpr uint64_t ADAM_MAX_GROUPS = (1ull << 31) - 1;

// optim_plan.hip: pure host arithmetic (no HIP call), so that a stand-alone program can run it without a GPU.
// Every VQCPC_ERR_INVALID of vqcpc_adam_step that the host can see without the runtime.
int adam_validate(const vqcpc_adam_tensor *tensors, int n_tensors, const vqcpc_adam_hyper *h);
AdamScalars adam_scalars(const vqcpc_adam_hyper &h);
// Fill `tab` with the tensors of the list from *next on, in list order, skipping numel == 0, until the table is full, the list
// ends or the next tensor's workgroups would take the grid past ADAM_MAX_GROUPS; *next moves behind the last tensor looked at.
// -> the workgroups of the launch (0: nothing left to launch).
uint32_t adam_fill(const vqcpc_adam_tensor *tensors, int n_tensors, int *next, AdamTable &tab);
