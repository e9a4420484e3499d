// adam_plan_main.hip -- a stand-alone program over the host arithmetic of vqcpc_adam_step (csrc/optim_plan.hip): argument
// validation, the six scalars and the split of a tensor list into per-launch tables.  It makes no HIP call and needs no GPU; it
// is meant to be built with the host sanitizers and run as it is:
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -o adam_plan_main tests/host/adam_plan_main.hip vectorquantizedcpc_amd/csrc/optim_plan.hip && ./adam_plan_main
//
// Exit status 0 and "adam_plan_main: ... OK" when every check holds.
#include "../../vectorquantizedcpc_amd/csrc/optim.h"
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <vector>

static char g_err[512];
void vq_set_error(const char *fmt, ...) {                 // runtime.hip's, without the library
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

static int g_checks = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        ++g_checks;                                                                     \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s FAILED (last error: %s)\n", __FILE__, __LINE__, #cond, g_err); return 1; } \
    } while (0)

static float *fake(uintptr_t a) { return (float *)a; }    // an address that is only compared and stored, never read through

static vqcpc_adam_tensor tensor(uint64_t numel, uintptr_t base) {
    return vqcpc_adam_tensor{fake(base), fake(base + 0x1000000), fake(base + 0x2000000), fake(base + 0x3000000), numel};
}

// The whole list through adam_fill: every tensor with elements appears once, in order, with its own pointers; the prefix counts
// ceil(numel / CHUNK) workgroups each; no launch goes past the table or the grid limit.  -> launches, or -1.
static int walk(const std::vector<vqcpc_adam_tensor> &list) {
    int next = 0, launches = 0;
    size_t seen = 0;                                       // index into the list of the next tensor expected
    while (next < (int)list.size()) {
        AdamTable tab{};
        const int before = next;
        const uint32_t groups = adam_fill(list.data(), (int)list.size(), &next, tab);
        if (next <= before && groups == 0) return -1;
        if (groups == 0) break;
        ++launches;
        if (tab.n < 1 || tab.n > VQCPC_ADAM_TABLE || tab.first[0] != 0 || tab.first[tab.n] != groups) return -1;
        if ((uint64_t)groups > ADAM_MAX_GROUPS) return -1;
        for (int k = 0; k < tab.n; ++k) {
            while (seen < list.size() && list[seen].numel == 0) ++seen;
            if (seen >= list.size()) return -1;
            const vqcpc_adam_tensor &t = list[seen++];
            if (tab.p[k] != t.param || tab.g[k] != t.grad || tab.m[k] != t.exp_avg || tab.v[k] != t.exp_avg_sq || tab.numel[k] != t.numel) return -1;
            const uint64_t mine = t.numel / VQCPC_ADAM_CHUNK + (t.numel % VQCPC_ADAM_CHUNK != 0);
            if ((uint64_t)tab.first[k + 1] - tab.first[k] != mine) return -1;
            // the last workgroup of the tensor starts inside it: the kernel's `left` is >= 1
            if ((mine - 1) * VQCPC_ADAM_CHUNK >= t.numel) return -1;
        }
    }
    while (seen < list.size() && list[seen].numel == 0) ++seen;
    return seen == list.size() ? launches : -1;
}

int main() {
    const vqcpc_adam_hyper good{4e-4, 0.9, 0.999, 1e-8, 1};
    std::vector<vqcpc_adam_tensor> one{tensor(5, 0x10000)};

    // ---- validation: every VQCPC_ERR_INVALID the host can see
    CHECK(adam_validate(one.data(), 1, &good) == VQCPC_OK);
    CHECK(adam_validate(nullptr, 1, &good) == VQCPC_ERR_INVALID);
    CHECK(adam_validate(one.data(), 1, nullptr) == VQCPC_ERR_INVALID);
    CHECK(adam_validate(one.data(), 0, &good) == VQCPC_ERR_INVALID);
    CHECK(adam_validate(one.data(), -3, &good) == VQCPC_ERR_INVALID);
    for (int member = 0; member < 4; ++member)
        for (int how = 0; how < 2; ++how) {                // 0: NULL, 1: misaligned by 4 bytes
            vqcpc_adam_tensor t = tensor(5, 0x10000);
            float **slot[4] = {&t.param, (float **)&t.grad, &t.exp_avg, &t.exp_avg_sq};
            *slot[member] = how ? fake((uintptr_t)*slot[member] + 4) : nullptr;
            CHECK(adam_validate(&t, 1, &good) == VQCPC_ERR_INVALID);
            CHECK(strstr(g_err, how ? "aligned" : "null") != nullptr);
            t.numel = 0;                                   // an empty tensor's pointers are not looked at
            CHECK(adam_validate(&t, 1, &good) == VQCPC_OK);
        }
    {
        vqcpc_adam_hyper h = good;
        h.step = 0; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.step = -1; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h = good; h.lr = -1e-3; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.lr = NAN; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.lr = INFINITY; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.lr = 0.0; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_OK);
        h = good; h.eps = -1e-8; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.eps = NAN; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.eps = INFINITY; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        h.eps = 0.0; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_OK);
        const double bad_beta[] = {-0.1, 1.0, 1.5, NAN, INFINITY};
        for (double b : bad_beta) {
            h = good; h.beta1 = b; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
            h = good; h.beta2 = b; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_ERR_INVALID);
        }
        h = good; h.beta1 = 0.0; h.beta2 = 0.0; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_OK);
        h = good; h.step = INT64_MAX; CHECK(adam_validate(one.data(), 1, &h) == VQCPC_OK);
    }
    {   // one tensor that no launch covers
        vqcpc_adam_tensor t = tensor((ADAM_MAX_GROUPS + 1) * VQCPC_ADAM_CHUNK, 0x10000);
        CHECK(adam_validate(&t, 1, &good) == VQCPC_ERR_INVALID);
        t.numel = ADAM_MAX_GROUPS * VQCPC_ADAM_CHUNK;
        CHECK(adam_validate(&t, 1, &good) == VQCPC_OK);
        t.numel = UINT64_MAX;
        CHECK(adam_validate(&t, 1, &good) == VQCPC_ERR_INVALID);
    }

    // ---- the scalars: formed in double, rounded once
    {
        const vqcpc_adam_hyper h{4e-4, 0.9, 0.999, 1e-8, 20};
        const AdamScalars k = adam_scalars(h);
        CHECK(k.w1 == (float)(1.0 - 0.9) && k.c2 == (float)0.999 && k.w2 == (float)(1.0 - 0.999) && k.e == (float)1e-8);
        CHECK(k.rb == (float)sqrt(1.0 - pow(0.999, 20.0)) && k.ss == (float)(4e-4 / (1.0 - pow(0.9, 20.0))));
        const AdamScalars z = adam_scalars(vqcpc_adam_hyper{0.0, 0.0, 0.5, 0.0, 10000});
        CHECK(z.w1 == 1.0f && z.c2 == 0.5f && z.w2 == 0.5f && z.rb == 1.0f && z.e == 0.0f && z.ss == 0.0f);
        const AdamScalars far = adam_scalars(vqcpc_adam_hyper{1.0, 0.9, 0.999, 1e-8, INT64_MAX});
        CHECK(far.rb == 1.0f && far.ss == 1.0f);
    }

    // ---- the split into launches
    const int T = VQCPC_ADAM_TABLE, C = VQCPC_ADAM_CHUNK;
    CHECK(walk(one) == 1);
    {
        std::vector<vqcpc_adam_tensor> l;
        const uint64_t sizes[] = {1, 3, 4, 5, (uint64_t)C - 1, (uint64_t)C, (uint64_t)C + 1, 2ull * C + 3};
        for (size_t i = 0; i < sizeof sizes / sizeof *sizes; ++i) l.push_back(tensor(sizes[i], 0x10000 + 0x40 * i));
        CHECK(walk(l) == 1);
        int next = 0;
        AdamTable tab{};
        CHECK(adam_fill(l.data(), (int)l.size(), &next, tab) == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3 && next == (int)l.size() && tab.n == 8);
    }
    {   // empty tensors: between two others, first, last, all of them
        std::vector<vqcpc_adam_tensor> l{tensor(5, 0x10000), tensor(0, 0), tensor(7, 0x20000)};
        CHECK(walk(l) == 1);
        l.insert(l.begin(), tensor(0, 0));
        l.push_back(tensor(0, 0));
        CHECK(walk(l) == 1);
        std::vector<vqcpc_adam_tensor> none(5, tensor(0, 0));
        CHECK(walk(none) == 0);
        int next = 0;
        AdamTable tab{};
        CHECK(adam_fill(none.data(), 5, &next, tab) == 0 && next == 5 && tab.n == 0);
    }
    for (int n : {T - 1, T, T + 1, 2 * T, 2 * T + 5}) {    // the table fills: ceil(n / T) launches
        std::vector<vqcpc_adam_tensor> l;
        for (int i = 0; i < n; ++i) l.push_back(tensor(2 + i % 5, 0x10000 + 0x40 * (uintptr_t)i));
        CHECK(walk(l) == (n + T - 1) / T);
        for (int i = n; i > 0; i -= 7) l.insert(l.begin() + i, tensor(0, 0));     // empty ones take no slot
        CHECK(walk(l) == (n + T - 1) / T);
    }
    {   // the grid limit closes a launch before the table is full
        const uint64_t big = (ADAM_MAX_GROUPS / 2 + 1) * C;
        std::vector<vqcpc_adam_tensor> l{tensor(big, 0x10000), tensor(big, 0x20000), tensor(9, 0x30000)};
        CHECK(adam_validate(l.data(), 3, &good) == VQCPC_OK);
        CHECK(walk(l) == 2);
        std::vector<vqcpc_adam_tensor> edge{tensor(ADAM_MAX_GROUPS * C, 0x10000), tensor(1, 0x20000)};
        CHECK(walk(edge) == 2);
        std::vector<vqcpc_adam_tensor> fits{tensor((ADAM_MAX_GROUPS - 1) * C, 0x10000), tensor(C, 0x20000)};
        CHECK(walk(fits) == 1);
    }
    printf("adam_plan_main: %d checks OK\n", g_checks);
    return 0;
}
