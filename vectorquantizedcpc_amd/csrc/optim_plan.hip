// optim_plan.hip -- the host arithmetic of vqcpc_adam_step: argument validation, the six scalars and the split of a tensor list
// into per-launch tables.  Pure host code (no HIP call), so that it can be run without a GPU and under the host sanitizers
// (tests/host/adam_plan_main.hip).
#include "optim.h"
#include <math.h>

// ceil(numel / CHUNK) without the overflow of numel + CHUNK - 1
static uint64_t chunks_of(uint64_t numel) { return numel / VQCPC_ADAM_CHUNK + (numel % VQCPC_ADAM_CHUNK != 0); }

int adam_validate(const vqcpc_adam_tensor *tensors, int n_tensors, const vqcpc_adam_hyper *h) {
    VQ_REQUIRE(tensors && h, "vqcpc_adam_step: null argument");
    VQ_REQUIRE(n_tensors >= 1, "vqcpc_adam_step: n_tensors = %d, need at least 1", n_tensors);
    VQ_REQUIRE(h->step >= 1, "vqcpc_adam_step: step = %lld, need the number of this update, >= 1", (long long)h->step);
    VQ_REQUIRE(isfinite(h->lr) && h->lr >= 0.0, "vqcpc_adam_step: lr = %g, need a finite value >= 0", h->lr);
    VQ_REQUIRE(isfinite(h->eps) && h->eps >= 0.0, "vqcpc_adam_step: eps = %g, need a finite value >= 0", h->eps);
    VQ_REQUIRE(h->beta1 >= 0.0 && h->beta1 < 1.0, "vqcpc_adam_step: beta1 = %g outside [0, 1)", h->beta1);      // a NaN fails both
    VQ_REQUIRE(h->beta2 >= 0.0 && h->beta2 < 1.0, "vqcpc_adam_step: beta2 = %g outside [0, 1)", h->beta2);
    for (int i = 0; i < n_tensors; ++i) {
        const vqcpc_adam_tensor &t = tensors[i];
        if (t.numel == 0) continue;
        VQ_REQUIRE(t.param && t.grad && t.exp_avg && t.exp_avg_sq, "vqcpc_adam_step: tensor %d has a null member", i);
        VQ_REQUIRE(aligned16(t.param, t.grad, t.exp_avg, t.exp_avg_sq), "vqcpc_adam_step: tensor %d has a member that is not 16-byte aligned", i);
        VQ_REQUIRE(chunks_of(t.numel) <= ADAM_MAX_GROUPS,
                   "vqcpc_adam_step: tensor %d has %llu elements, more than one launch covers", i, (unsigned long long)t.numel);
    }
    return VQCPC_OK;
}

AdamScalars adam_scalars(const vqcpc_adam_hyper &h) {
    const double t = (double)h.step;
    AdamScalars k;
    k.w1 = (float)(1.0 - h.beta1);
    k.c2 = (float)h.beta2;
    k.w2 = (float)(1.0 - h.beta2);
    k.rb = (float)sqrt(1.0 - pow(h.beta2, t));
    k.e = (float)h.eps;
    k.ss = (float)(h.lr / (1.0 - pow(h.beta1, t)));
    return k;
}

uint32_t adam_fill(const vqcpc_adam_tensor *tensors, int n_tensors, int *next, AdamTable &tab) {
    uint64_t groups = 0;
    tab.n = 0;
    tab.first[0] = 0;
    int i = *next;
    for (; i < n_tensors && tab.n < VQCPC_ADAM_TABLE; ++i) {
        const vqcpc_adam_tensor &t = tensors[i];
        if (t.numel == 0) continue;
        const uint64_t mine = chunks_of(t.numel);
        if (groups + mine > ADAM_MAX_GROUPS) break;              // tab.n > 0 here: adam_validate holds one tensor below the limit
        const int k = tab.n++;
        tab.p[k] = t.param; tab.g[k] = t.grad; tab.m[k] = t.exp_avg; tab.v[k] = t.exp_avg_sq;
        tab.numel[k] = t.numel;
        groups += mine;
        tab.first[k + 1] = (uint32_t)groups;
    }
    *next = i;
    return (uint32_t)groups;
}
