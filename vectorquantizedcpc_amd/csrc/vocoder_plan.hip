// vocoder_plan.hip -- the decode planner of the vocoder handle: pure host arithmetic (no HIP call), so that it can be tested
// without a GPU (vqcpc_vocoder_plan, tests/test_plan_cpu.py).  It reads the handle's options as a PlanOpts.
#include "vocoder_internal.h"
#include <algorithm>

// Which decode loop takes a call, and the resident decoders' slot schedule: pure host arithmetic (no HIP call), so that it can be
// tested without a GPU (vqcpc_vocoder_plan).  samples[b] = samples utterance b produces; `order` = utterances longest first.
// Paths: DecodePlan.  A slot's schedule must stay below 2^24 - 1 steps (the candidate tag of step t is
// (t + 1) << 8 in 32 bits): a call `auto` would have put on the resident decoders then takes the launch path; asked for by name
// (xcd / xcm = 1) it is an error (returns false).
std::vector<int> longest_first(const int *samples, int B) {
    std::vector<int> order(B);
    for (int b = 0; b < B; ++b) order[b] = b;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return samples[a] > samples[b]; });
    return order;
}

// Longest-first assignment (LPT) of the utterances of `order` over xs slots: each onto the slot that frees up first (the lowest
// on a tie), where it starts; a slot frees up at the first multiple of `gran` steps from the end of its last utterance
// (steps_per_graph on the launch path, whose utterances start at replay boundaries; 1 on the resident decoders).
static void lpt(const std::vector<int> &order, const int *samples, const unsigned *utt, int xs, int gran, DecodePlan &pl) {
    pl.xend.assign(xs, 0);
    pl.lists.assign(xs, {});
    for (int row : order) {
        const int len = samples[row];
        if (len <= 0) continue;
        int best = 0;
        for (int q = 1; q < xs; ++q) if (pl.xend[q] < pl.xend[best]) best = q;
        pl.lists[best].push_back(XdSeg{row, (int)pl.xend[best], len, utt ? utt[row] : (unsigned)row});
        pl.xend[best] = (pl.xend[best] + len + gran - 1) / gran * gran;
    }
    pl.longest = 0;
    for (long e : pl.xend) pl.longest = e > pl.longest ? e : pl.longest;
}

bool plan_decode(const PlanOpts &o, const int *samples, const unsigned *utt, const std::vector<int> &order, DecodePlan &pl) {
    int nz = 0;
    long max_len = 0;
    for (int row : order) { nz += samples[row] > 0; max_len = samples[row] > max_len ? samples[row] : max_len; }
    pl = DecodePlan{};
    // auto: up to xcm_min (68) utterances in flight ar_xcd.hip (8.5 M samples/s through its 32 slots at 32 and 64 utterances
    // against 3.4 / 4.7 M on the launch path), from there to xcm_max the 16-slot matrix-core form through its 128 slots (9.3 M at 96,
    // 12.4 M from 128), above that the launch-per-step kernels; `xcd` = 0 turns both off, = 1 asks for ar_xcd.hip whatever the count
    const int in_flight = o.n_slots > 0 && o.n_slots < nz ? o.n_slots : nz;
    const bool xcm_wanted = o.xcd != 0 && (o.xcm == 1 || (o.xcm == -1 && o.xcd == -1 && in_flight > o.xcm_min && in_flight < o.xcm_max));
    const bool xcd_wanted = xcm_wanted || o.xcd == 1 || (o.xcd == -1 && in_flight <= o.xcm_min);
    if (!xcd_wanted || !o.supported || max_len <= 0 || nz <= 0) return true;
    int xs = xcm_wanted ? o.xcm_slots : (o.xcd_slots < 1 ? 1 : o.xcd_slots);
    if (o.n_slots > 0 && o.n_slots < xs) xs = o.n_slots;
    if (nz < xs) xs = nz;
    const int bxt = xcm_wanted ? XM_BX : xd_pick_bxt((xs + 7) / 8);
    lpt(order, samples, utt, xs, 1, pl);
    const bool fits = bxt > 0 && pl.longest + 1 < (1L << 24);
    if (!fits) {
        pl.lists.clear(); pl.xend.clear();
        return !(o.xcd == 1 || o.xcm == 1);
    }
    pl.path = xcm_wanted ? 3 : 2; pl.xs = xs; pl.bxt = bxt;
    return true;
}

extern "C" int vqcpc_vocoder_plan(int xcd, int xcm, int xcm_min, int xcm_max, int xcd_slots, int xcm_slots, int slots,
                                  const int *n_samples, int B, int *path, int *slots_used, int64_t *longest) {
    VQ_REQUIRE(n_samples && B > 0 && path && slots_used && longest, "vqcpc_vocoder_plan: bad argument");
    DecodePlan pl;
    const PlanOpts o{xcd, xcm, xcm_min < 0 ? XCM_MIN_DEFAULT : xcm_min, xcm_max < 0 ? XCM_MAX_DEFAULT : xcm_max,
                     xcd_slots <= 0 ? XCD_SLOTS_DEFAULT : xcd_slots, xcm_slots <= 0 ? XCM_SLOTS_DEFAULT : xcm_slots, slots, true};
    VQ_REQUIRE(plan_decode(o, n_samples, nullptr, longest_first(n_samples, B), pl), "vocoder: a decode slot's schedule does not fit "
               "the resident decoders (< 2^24 - 1 samples); use more slots or xcd = -1");
    *path = pl.path; *slots_used = pl.path ? pl.xs : (slots > 0 && slots < B ? slots : B); *longest = pl.longest;
    return VQCPC_OK;
}

// The per-utterance layout of a call: frames for the prenet (ragged conditioning rows), samples for the AR loop.
int utt_layout(int B, int Tc, const int *n_codes_host, int upsample_t, unsigned utt_base, const uint32_t *utt_ids_host, UttLayout &u) {
    const int Bp = (B + 15) / 16 * 16;
    u.lens.assign(2 * Bp, 0);
    u.utt.resize(B);
    u.gbase.assign(Bp, 0);
    u.grows = 0;
    for (int b = 0; b < B; ++b) {
        const int nc = n_codes_host ? n_codes_host[b] : Tc;
        VQ_REQUIRE(nc >= 0 && nc <= Tc, "vocoder: n_codes[%d] = %d outside [0, %d]", b, nc, Tc);
        u.lens[b] = 2 * nc;
        u.lens[Bp + b] = upsample_t * 2 * nc;
        u.utt[b] = utt_ids_host ? utt_ids_host[b] : utt_base + (unsigned)b;
        u.gbase[b] = (int)u.grows;
        u.grows += 2 * nc;
    }
    VQ_REQUIRE(u.grows < (1L << 31), "vocoder: %ld conditioning frames in one call", u.grows);
    return VQCPC_OK;
}

int plan_call(const PlanOpts &o, int B, int Tc, const int *n_codes_host, bool tf, int Ts, int max_steps, unsigned utt_base,
              const uint32_t *utt_ids_host, CallPlan &cp, const int *tf_len) {
    TRY(utt_layout(B, Tc, n_codes_host, o.upsample_t, utt_base, utt_ids_host, cp));
    int *samples = cp.lens.data() + (B + 15) / 16 * 16;
    for (int b = 0; b < B; ++b) {
        int ns = samples[b];
        if (tf) ns = ns < Ts ? ns : Ts;
        if (tf && tf_len) ns = ns < tf_len[b] ? ns : tf_len[b];      // a scoring call: the utterance's own scored length
        if (max_steps > 0 && ns > max_steps) ns = max_steps;
        samples[b] = ns;
    }
    const std::vector<int> order = longest_first(samples, B);
    PlanOpts po = o;                      // a teacher-forced scan takes the launch path, one slot per utterance
    if (tf) { po.n_slots = 0; po.supported = false; }
    VQ_REQUIRE(plan_decode(po, samples, cp.utt.data(), order, cp.dp), "vocoder: a decode slot's schedule does not fit the resident "
               "decoders (< 2^24 - 1 samples); use more slots or xcd = -1");
    if (cp.dp.path != 0) return VQCPC_OK;
    return plan_launch_tables(po, samples, order, tf, B, 0, cp);
}

// The launch path's schedule: slots, tile groups and per-replay slot tables.  s0 > 0 (a stream chunk): every utterance resumes at
// absolute sample s0, and its slot rows say t0 - s0 and s0 + len (ArCall::s0).
int plan_launch_tables(const PlanOpts &o, const int *samples, const std::vector<int> &order, bool tf, int B, int s0, CallPlan &cp) {
    const int S = o.steps_per_graph;
    // Launch path (continuous batching): n_slots >= B: everything starts at 0.
    DecodePlan &dp = cp.dp;
    dp.xs = !tf && o.n_slots > 0 && o.n_slots < B ? o.n_slots : B;
    lpt(order, samples, cp.utt.data(), dp.xs, S, dp);
    VQ_REQUIRE(dp.longest < (1L << 30), "vocoder: schedule too long");
    const int nbt = (dp.xs + 15) / 16;
    // Tile groups: 3..big_min_tiles-1 tiles, or >= 2*big_min_tiles (both halves on the large-batch kernel), split in two.  (Measured: 2 x 16 utterances is slower than one
    // group of 32 -- the chip retires only ~0.43 dependent launches per us across queues -- while
    // 2 x 32 runs at 14.5 us per sample against 17.3 us for one group of 64.)  A teacher-forced scan runs as one group.
    // With the fused fc2 || GRU launch the overlap two groups were for happens inside one launch, and two fused launches in
    // flight only compete (64 utterances: 17.4 us per step on two groups, 13.4 on one: profiles/r02_gru_variants.csv): the
    // small kernel runs as ONE group; only large-batch calls of >= 2 * big_min_tiles tiles are still split.
    const bool small_fused = o.fuse_fc2 && !(o.big_min_tiles > 0 && nbt >= o.big_min_tiles);
    const bool split = !tf && o.two_groups && o.use_graph && nbt >= 3 && !small_fused &&
                       !(o.big_min_tiles > 0 && nbt >= o.big_min_tiles && nbt < 2 * o.big_min_tiles);
    cp.n_grp = split ? 2 : 1;
    cp.tiles[0] = split ? (nbt + 1) / 2 : nbt;
    cp.tiles[1] = split ? nbt / 2 : 0;
    for (int g = 0; g < cp.n_grp; ++g) {
        const int slot0 = g * cp.tiles[0] * 16, Spg = cp.tiles[g] * 16;
        const int q_end = slot0 + Spg < dp.xs ? slot0 + Spg : dp.xs;
        long end = 0;
        for (int q = slot0; q < q_end; ++q) end = dp.xend[q] > end ? dp.xend[q] : end;
        cp.gmax[g] = (int)end; cp.rep[g] = cp.gmax[g] / S;
        cp.table[g].assign((size_t)(cp.rep[g] > 0 ? cp.rep[g] : 1) * Spg, XdSeg{-1, 0, 0, 0u});
        for (int q = slot0; q < q_end; ++q)
            for (XdSeg sg : dp.lists[q]) {
                const int r0 = sg.t0 / S, r1 = (sg.t0 + sg.len + S - 1) / S;
                sg.t0 -= s0; sg.len += s0;
                for (int r = r0; r < r1; ++r) cp.table[g][(size_t)r * Spg + (q - slot0)] = sg;
            }
    }
    return VQCPC_OK;
}
