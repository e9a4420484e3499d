"""-m gpu: every entry point of ``include/vqcpc.h`` that takes a ``stream``, held to the header's first convention on a CALLER's
stream: *all work is enqueued on `stream`; no call synchronises except where stated*.

Procedure: tests/stream_harness.py (its docstring says what each step catches).  In short: the call runs once on the default
stream for its reference bits; then, on a fresh stream ``s``, behind a delay of matmuls, the true inputs are written into buffers that
hold a DECOY until then (valid inputs of another seed: finite, in range), the call is made, ``busy`` is taken (the stream not idle
AND an event recorded behind the delay not yet reached), the outputs are cloned on ``s`` and the inputs overwritten with the decoy
again -- all without a host synchronisation, and all of it twice, on two fresh streams in a row.  The clones must have the
reference's bits, and ``busy`` must be true for every entry the header does not list as synchronising.  Nothing numeric
is judged here: the other GPU files judge the default-stream results against float64, and the header promises equal bits for equal
inputs.  One library call is in flight at a time; two streams are used only one after the other, with ``wait_stream`` between
them (the header's "an event between" rule).

Entries against the header.  N = held to "does not synchronise" (``busy`` asserted) and to ordering; O = ordering only (the header
says the entry synchronises ``stream``); the tests that hold it, in this file unless the row names another (the gradient and
optimizer entries are held, with the same harness, next to the cases they are run on):

  ==================================  ===  ====================================================================================
  vqcpc_encoder_encode                N    test_encoder_encode (fused 0, 1, 2)
  vqcpc_encoder_stage                 N    test_encoder_stage
  vqcpc_encoder_vq_encode             N    test_vq_encode_and_forward_stats
  vqcpc_encoder_forward_stats         N    test_vq_encode_and_forward_stats, test_vq_adapt
  vqcpc_encoder_vq_adapt              N    test_vq_adapt (embedding, ema_count, ema_weight are in-out)
  vqcpc_encoder_context               N    test_encoder_context (1 x 300 resident scan, 17 x 33 one launch per step)
  vqcpc_encoder_context_fwd           N    test_context_fwd_bwd_weights_in_stream_order
  vqcpc_encoder_context_bwd           N    test_context_fwd_bwd_weights_in_stream_order
  vqcpc_encoder_front_fwd             N    test_gpu_front_grad_stream.py::test_front_fwd_bwd_weights_in_stream_order
  vqcpc_encoder_front_bwd             N    test_gpu_front_grad_stream.py::test_front_fwd_bwd_weights_in_stream_order
  vqcpc_encoder_vq_bwd                N    test_gpu_front_grad_stream.py::test_vq_bwd
  vqcpc_cpc_score                     N    test_cpc_score (given and seeded negatives)
  vqcpc_cpc_grad                      N    test_cpc_grad (given / seeded negatives; W and bias written on s)
  vqcpc_abx_score                     N    test_abx_pair_distances
  vqcpc_abx_code_table                N    test_abx_code_table
  vqcpc_abx_score_indices             N    test_abx_pair_distances_indices (angular, edit)
  vqcpc_vocoder_generate              N    test_generate_resident (paths 2, 3), test_generate_launch_path (fused, two tile groups,
                                           large batch, no graph), test_generate_second_group_outlasts_the_first,
                                           test_staging_arena_back_to_back
  vqcpc_vocoder_stream_open           N    test_streaming (busy after open: the chunks behind it may wait for the staging arena)
  vqcpc_vocoder_stream_next           O*   test_streaming (one stream; two streams alternating; a generate between two chunks)
  vqcpc_vocoder_stream_redo           O*   test_streaming
  vqcpc_vocoder_logits                N    test_logits
  vqcpc_vocoder_nll                   N    test_nll
  vqcpc_vocoder_ar_fwd                N    test_gpu_voc_grad_stream.py::test_ar_fwd_then_bwd_weights_in_stream_order
  vqcpc_vocoder_ar_bwd                N    test_gpu_voc_grad_stream.py::test_ar_bwd_alone
  vqcpc_vocoder_ar_fwd_cond           N    test_gpu_cond_grad_stream.py::test_ar_fwd_cond_then_bwd_cond
  vqcpc_vocoder_ar_bwd_cond           N    test_gpu_cond_grad_stream.py::test_ar_bwd_cond_alone
  vqcpc_vocoder_cond_fwd              N    test_gpu_cond_grad_stream.py::test_cond_fwd_then_bwd_weights_in_stream_order
  vqcpc_vocoder_cond_bwd              N    test_gpu_cond_grad_stream.py::test_cond_bwd_alone
  vqcpc_vocoder_glue                  N    test_glue_and_condition
  vqcpc_vocoder_condition             N    test_glue_and_condition
  vqcpc_vocoder_kernel_times          O    test_kernel_times_between_two_calls (must return with the stream idle)
  vqcpc_melfront_run                  O    test_melfront
  vqcpc_resampler_run                 N    test_resampler (on a handle whose clock table is long enough, the header's condition)
  vqcpc_loudness_integrated           O    test_loudness
  vqcpc_loudness_normalize            O    test_loudness
  vqcpc_adam_step                     N    test_gpu_adam_stream.py::test_adam_step_on_a_callers_stream
  ==================================  ===  ====================================================================================

  O*: a call on a vocoder handle waits on the host for the event behind the PREVIOUS call's uploads (the header says so), and
  in these tests the previous call sits behind the delay; so ``busy`` is taken after the first call of such a sequence only.

``test_every_stream_entry_is_listed`` reads the header and fails when an entry with a ``stream`` argument is missing above.
``test_harness_rejects_faulty_entries`` shows on every run that a pass is not vacuous: four pure-torch entries that break the
contract (work on another stream, and on the default stream; a fork that is never joined; a stream synchronisation) are
rejected, a correct one passes.

Found with this file, on an MI355X:

* ``abx.pair_distances`` / ``pair_distances_indices`` say "does not synchronise", but their table upload was
  ``torch.from_numpy(...).to(device)`` from pageable memory, which torch ends with a stream synchronisation: with that line put
  back, ``test_abx_pair_distances`` and both cases of ``test_abx_pair_distances_indices`` fail on ``busy``.  The upload now goes
  through pinned memory with ``non_blocking=True``.  The C entries were not at fault, and no other entry failed.
* The resident decoders place as well from a caller's stream as from the default one: paths 2 and 3 never reported a miss
  (``check()`` after every case).
* ``use_graph`` = 0 at B = 40, Tc = 4 returns with the delay gone, and not because the library synchronises: the HIP runtime makes
  the host wait once enough commands sit behind work that has not started (``test_generate_launch_path`` has the figures).  That
  case is held to ordering, the same call at Tc = 1 to "does not synchronise", and the header's conventions say so now.
* Two properties of the procedure itself, both in the harness now: ``not s.query()`` alone passes an entry that synchronises first
  and enqueues afterwards (the self-test's synchronising entry did), and work that falls onto the default stream is in order, by accident,
  with every fourth fresh stream (the runtime's hardware queues), hence the event behind the delay and the two streams in a row.

Measured on an MI355X (the whole file: 43 tests in 11 - 12 s, three runs).  One 2048 x 2048 fp32 ``torch.mm`` takes 119.6 us; the
delay is 169 of them (20.2 ms) while the largest ``t_host`` seen is below 2 ms, 45 ms for the no-graph call at Tc = 1 and 157 - 202
ms from the no-graph call at Tc = 4 on.  ``t_host`` of the call on an idle default stream, in ms: encode 0.15 - 0.20, stage 0.03, vq_encode 0.04,
forward_stats 0.06, vq_adapt 0.13 (fresh handle), context 0.04 (1 x 300, resident) / 0.17 (17 x 33), context_fwd + bwd 0.11,
cpc_score 0.04 - 0.05, cpc_grad 0.06 - 0.15, abx 0.03 - 0.24, generate 0.25 - 0.42 on the resident decoders, 1.2 - 2.1 through captured
graphs, 4.5 / 15.7 - 20.2 without a graph at Tc = 1 / 4, stream open + 3 chunks + redo 2.0 (14.6 at B = 40 on the launch path), logits 0.38,
glue 0.01, condition 0.07, nll 1.2, resampler 0.04; the synchronising entries 0.05 - 0.10 (they then wait out the delay: 132 -
171 ms on the host).  Every ``busy`` precondition was met; the second call of a back-to-back pair does wait for the first one's
uploads (133 - 170 ms on the host, the delay), as documented.

Would the file notice?  Five host-side faults (wrong values at worst, never an address), each built as a library of its own with
``tools/build_variant.sh NAME "" UNIT changed-copy.hip`` (none committed) and run once in place of the real one, on this file:

  1. ``launch_enc_fused`` given stream 0 in ``encoder_fused``: 2 failed -- ``test_encoder_encode[1]`` and ``test_encoder_stage``
     (values; the two callers of that launch).
  2. the ``hipMemsetAsync`` of ``wav`` in ``run_ar`` given stream 0: 12 failed -- every case of ``test_generate_resident`` and
     ``test_generate_launch_path``, ``test_generate_second_group_outlasts_the_first``, both cases of
     ``test_staging_arena_back_to_back`` and ``test_kernel_times_between_two_calls`` (values, ``wav`` only: the columns behind a
     short utterance keep the dirt of the harness's step (b')).
  3. ``hipStreamWaitEvent(s, ev_join)`` of the two-group path removed: ``test_generate_second_group_outlasts_the_first`` failed
     (values, ``wav`` and ``mulaw``); the B = 40 case of the issue passed, as group 1 holds the shortest utterances there and is done
     first -- the reason that test exists.  Run on the ``test_generate*`` tests only: between two calls the missing join would
     let one chunk's call record change under the other's kernels.
  4. ``hipStreamSynchronize(stream)`` added at the top of ``vqcpc_cpc_score``: both cases of ``test_cpc_score`` failed (``busy``).
  5. ``begin_call`` no longer waiting for the pending upload event (``HostStage::begin``): both cases of
     ``test_staging_arena_back_to_back`` failed (values: the first call ran on the second call's tables).  Run on that test only,
     whose two calls have tables of equal shape; elsewhere the fault mixes tables of different layouts.

  On the first harness (one stream per case) fault 1 got past ``test_encoder_encode[1]`` and fault 2 past the B = 5 case: the
  hardware-queue accident above.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abx_index_ref
import cpc_grad_ref
import ctx_grad_ref
import ema_ref
import nll_ref
import stream_harness as H
import vectorquantizedcpc_amd as V
from test_gpu_abx import blocks_of, geometry_case
from vectorquantizedcpc_amd import _lib, abx, loudness, preprocess, synth

pytestmark = pytest.mark.gpu

# every entry of include/vqcpc.h with a `stream` argument -> how it is held (the table of the docstring)
ENTRIES = {
    "vqcpc_encoder_encode": "N", "vqcpc_encoder_stage": "N", "vqcpc_encoder_vq_encode": "N", "vqcpc_encoder_forward_stats": "N",
    "vqcpc_encoder_vq_adapt": "N", "vqcpc_encoder_context": "N", "vqcpc_encoder_context_fwd": "N", "vqcpc_encoder_context_bwd": "N",
    "vqcpc_cpc_score": "N", "vqcpc_cpc_grad": "N", "vqcpc_abx_score": "N", "vqcpc_abx_code_table": "N", "vqcpc_abx_score_indices": "N",
    "vqcpc_vocoder_generate": "N", "vqcpc_vocoder_stream_open": "N", "vqcpc_vocoder_stream_next": "O", "vqcpc_vocoder_stream_redo": "O",
    "vqcpc_vocoder_logits": "N", "vqcpc_vocoder_nll": "N", "vqcpc_vocoder_glue": "N", "vqcpc_vocoder_condition": "N",
    "vqcpc_vocoder_kernel_times": "O", "vqcpc_melfront_run": "O", "vqcpc_resampler_run": "N", "vqcpc_loudness_integrated": "O",
    "vqcpc_loudness_normalize": "O",
    "vqcpc_encoder_front_fwd": "N", "vqcpc_encoder_front_bwd": "N", "vqcpc_encoder_vq_bwd": "N",
    "vqcpc_vocoder_ar_fwd": "N", "vqcpc_vocoder_ar_bwd": "N", "vqcpc_vocoder_ar_fwd_cond": "N", "vqcpc_vocoder_ar_bwd_cond": "N",
    "vqcpc_vocoder_cond_fwd": "N", "vqcpc_vocoder_cond_bwd": "N", "vqcpc_adam_step": "N",
}


def cur():
    return _lib.current_stream()


def ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------------- the harness itself
def test_every_stream_entry_is_listed():
    assert len(H.check_entries_listed(ENTRIES, __doc__)) >= 36


def test_harness_rejects_faulty_entries():
    x = synth._uniform("sc/self/x", (1 << 20,), 1.0, synth.SEED).cuda()
    decoy = synth._uniform("sc/self/decoy", (1 << 20,), 1.0, synth.SEED).cuda()
    other = torch.cuda.Stream()

    def correct(t):
        return t * 2.0 + 1.0

    def on_another_stream(t):                              # (i) not ordered behind the caller's stream
        with torch.cuda.stream(other):
            return t * 2.0 + 1.0

    def on_the_default_stream(t):                          # (i') the same on the stream a dropped `s` falls onto
        with torch.cuda.stream(torch.cuda.default_stream()):
            return t * 2.0 + 1.0

    def fork_without_join(t):                              # (ii) ordered behind it, but never joined back
        out = torch.zeros_like(t)                          # cleared on the caller's stream, as the library clears its outputs
        other.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            y = t * 2.0 + 1.0
            for _ in range(300):                           # ~1 ms of dependent kernels before the result lands
                y = y * 1.0
            out.copy_(y)
        return out

    def synchronises(t):                                   # (iii)
        torch.cuda.current_stream().synchronize()
        return t * 2.0 + 1.0

    H.hold(correct, [x], [decoy], label="self-test: correct entry")
    for entry, kind in ((on_another_stream, "values"), (on_the_default_stream, "values"), (fork_without_join, "values"),
                        (synchronises, "sync")):
        with pytest.raises(H.ContractBreach) as e:
            H.hold(entry, [x], [decoy], label="self-test: " + entry.__name__)
        assert e.value.kind == kind, (entry.__name__, str(e.value))
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- encoder
@functools.lru_cache(maxsize=None)
def encoder():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict(ln_affine="random", codebook="data"))
    return enc.cuda().eval()


@pytest.mark.parametrize("fused", [0, 1, 2])
def test_encoder_encode(fused):
    enc = encoder()
    enc.set_option("fused", fused)
    try:
        mel, decoy = synth.mel("sc/enc", 3, 70).cuda(), synth.mel("sc/enc/decoy", 3, 70).cuda()
        H.hold(lambda m: enc.encode(m), [mel], [decoy], label=f"encode (3, 70) fused={fused}")
        assert enc.last_schedule() == fused
    finally:
        enc.set_option("fused", -1)


def test_encoder_stage():
    enc = encoder()
    mel, decoy = synth.mel("sc/stage", 2, 64).cuda(), synth.mel("sc/stage/decoy", 2, 64).cuda()
    H.hold(lambda m: enc.stage(m, 10), [mel], [decoy], label="stage 10 (2, 64)")


def test_vq_encode_and_forward_stats():
    enc = encoder()
    x = synth._uniform("sc/vq/x", (1, 65, 64), 1.5, synth.SEED).cuda()
    decoy = synth._uniform("sc/vq/decoy", (1, 65, 64), 1.5, synth.SEED).cuda()
    H.hold(lambda t: enc.codebook.encode(t), [x], [decoy], label="vq_encode 65 rows")
    H.hold(lambda t: enc.codebook(t), [x], [decoy], label="vq_encode + forward_stats 65 rows")


def test_vq_adapt():
    """n = 129 rows, 64 codes.  The call moves the handle's own codebook, so every run starts from a handle rebuilt from the
    module's (untouched) buffers; the caller's three buffers are live in-out tensors, written on ``s`` behind the delay."""
    case = ema_ref.make_case("sc_adapt", 64, 129, "skewed", "warm")
    other = ema_ref.make_case("sc_adapt_decoy", 64, 129, "uniform", "warm")
    enc = V.Encoder(V.ConfEncoder(80, 512, 64, 64, 256))
    sd = dict(synth.encoder_state_dict(n_embeddings=64))
    sd.update({"codebook." + k: torch.from_numpy(case[k]) for k in ("embedding", "ema_count", "ema_weight")})
    enc.load_state_dict(sd)
    enc = enc.cuda().eval()
    lib = _lib.load()

    def reset():
        enc.refresh()
        enc._native()

    def entry(x, emb, cnt, w):
        z_st, idx = torch.empty_like(x), torch.empty(x.size(0), dtype=torch.int64, device="cuda")
        stats = torch.empty(2, device="cuda")
        _lib.check(lib.vqcpc_encoder_vq_adapt(enc._native(), ptr(x), x.size(0), 0.999, 1e-5, ptr(emb), ptr(cnt), ptr(w), ptr(z_st),
                                              ptr(idx), ptr(stats[0:]), ptr(stats[1:]), cur()))
        q, idx2 = enc.codebook.encode(x[None])                  # the handle's own copy followed, in stream order
        return z_st, idx, stats, emb, cnt, w, q, idx2

    keys = ("x", "embedding", "ema_count", "ema_weight")
    res = H.hold(entry, [torch.from_numpy(case[k]).cuda() for k in keys], [torch.from_numpy(other[k]).cuda() for k in keys],
                 reset=reset, label="vq_adapt n=129 M=64")
    assert not torch.equal(res["3"], torch.from_numpy(case["embedding"]).cuda())        # the update did move the codebook


@pytest.mark.parametrize("B,T", [(1, 300), (17, 33)])
def test_encoder_context(B, T):
    enc = encoder()
    z = synth._uniform(f"sc/ctx/z{B}", (B, T, 64), 1.5, synth.SEED).cuda()
    decoy = synth._uniform(f"sc/ctx/decoy{B}", (B, T, 64), 1.5, synth.SEED).cuda()
    H.hold(lambda t: enc.context(t), [z], [decoy], label=f"context ({B}, {T})")
    enc.check()                                                      # the resident scan of (1, 300) gave up on no exchange


def test_context_fwd_bwd_weights_in_stream_order():
    """fwd then bwd back to back on ``s``; z, the four LSTM tensors and the upstream gradient are all written on ``s`` behind the
    delay: ``b_ih + b_hh`` and the W_hh fragments must be built from what the stream holds when the call's turn comes."""
    g = ctx_grad_ref.load("partial_tile")
    enc = encoder()
    keys = ("z", "w_ih", "w_hh", "b_ih", "b_hh", "G")
    true = [g[k].cuda() for k in keys]
    w2 = ctx_grad_ref.lstm_weights("sc_decoy", 64, 256)
    decoy = [ctx_grad_ref._u("sc_decoy/z", tuple(g["z"].shape), 1.0).cuda()] + [w2[k].cuda() for k in keys[1:5]] + \
            [ctx_grad_ref._u("sc_decoy/G", tuple(g["G"].shape), 1.0).cuda()]

    def entry(z, w_ih, w_hh, b_ih, b_hh, G):
        ws = [w_ih, w_hh, b_ih, b_hh]
        c, saved = enc._context_fwd(z, ws)
        return [c, saved] + enc._context_bwd(z, c, saved, G, ws[:2])

    H.hold(entry, true, decoy, label="context_fwd + context_bwd partial_tile")


# ---------------------------------------------------------------------------------------------------- CPC
@functools.lru_cache(maxsize=None)
def cpc_case():
    g = cpc_grad_ref.load("small_odd")
    cpc = V.CPCLoss(V.ConfCPC(g["n_pred"], g["Spk"], g["Utt"], g["Neg"], 64, g["c_dim"]))
    cpc.load_state_dict(g["sd"])
    cpc = cpc.cuda().eval()
    zd, cd = synth.cpc_inputs("sc_decoy", g["N"], g["T"], c_dim=g["c_dim"])
    ud, sd = synth.cpc_negatives(99, 7, g["K"], g["Spk"], g["Utt"], g["Neg"], g["L"])
    Wd = synth._uniform("sc/cpc/W", tuple(g["W"].shape), g["c_dim"] ** -0.5, synth.SEED)
    bd = synth._uniform("sc/cpc/b", tuple(g["b"].shape), g["c_dim"] ** -0.5, synth.SEED)
    true = {k: g[k].cuda().contiguous() for k in ("z", "c", "W", "b", "utt", "seq")}
    decoy = {k: v.cuda().contiguous() for k, v in dict(z=zd, c=cd, W=Wd, b=bd, utt=ud, seq=sd).items()}
    return g, cpc, true, decoy


@pytest.mark.parametrize("negatives", ["given", "seeded"])
def test_cpc_score(negatives):
    g, cpc, true, decoy = cpc_case()
    K, N, L, J = g["K"], g["N"], g["L"], g["J"]
    lib, h = _lib.load(), cpc._native()
    if negatives == "seeded":                               # the public class: nothing in it reads a value back
        entry = lambda z, c: cpc.forward_detailed(z, c, seed=(7 << 32) | 5, stream_id=3, want_correct=True, want_scores=True)
        keys = ("z", "c")
    else:                                                   # the class checks the index range on the host: the ABI directly

        def entry(z, c, utt, seq):
            out = torch.empty(1 + 2 * K, device="cuda")
            correct = torch.empty(K, N, L, dtype=torch.uint8, device="cuda")
            scores = torch.empty(K, N, J, L, device="cuda")
            _lib.check(lib.vqcpc_cpc_score(h, ptr(z), ptr(c), g["T"], ptr(utt), ptr(seq), 0, 0, ptr(out[0:]), ptr(out[1:]),
                                           ptr(out[1 + K:]), ptr(correct), ptr(scores), cur()))
            return out, correct, scores
        keys = ("z", "c", "utt", "seq")
    H.hold(entry, [true[k] for k in keys], [decoy[k] for k in keys], label=f"cpc_score small_odd, {negatives} negatives")


@pytest.mark.parametrize("negatives", ["given", "seeded", "seeded, public class"])
def test_cpc_grad(negatives):
    g, cpc, true, decoy = cpc_case()
    if negatives == "seeded, public class":                 # CPCLoss.gradients: W and bias are stacked from the module on the stream
        entry = lambda z, c: cpc.gradients(z, c, seed=(7 << 32) | 5, stream_id=3)
        keys = ("z", "c")
    elif negatives == "seeded":
        entry = lambda z, c, W, b: cpc._grad_call(z, c, W, b, None, None, (7 << 32) | 5, 3, (True,) * 4)
        keys = ("z", "c", "W", "b")
    else:
        entry = lambda z, c, W, b, utt, seq: cpc._grad_call(z, c, W, b, utt, seq, 13, 0, (True,) * 4)
        keys = ("z", "c", "W", "b", "utt", "seq")
    H.hold(entry, [true[k] for k in keys], [decoy[k] for k in keys], label=f"cpc_grad small_odd, {negatives} negatives")


# ---------------------------------------------------------------------------------------------------- ABX
def test_abx_pair_distances():
    frames, tokens, pairs = geometry_case()
    blocks = blocks_of(pairs[:4])
    feats = torch.from_numpy(frames).cuda()
    decoy = synth._normalish("sc/abx/decoy", tuple(feats.shape), synth.SEED).cuda()
    H.hold(lambda f: tuple(abx.pair_distances(f, tokens, blocks)[:4]), [feats], [decoy], label="abx pair_distances, 4 blocks")


def test_abx_code_table():
    book = synth._normalish("sc/abx/book", (24, 20), synth.SEED).cuda()
    decoy = synth._normalish("sc/abx/book/decoy", (24, 20), synth.SEED).cuda()
    H.hold(lambda b: abx.code_table(b), [book], [decoy], label="abx code_table (24, 20)")


@pytest.mark.parametrize("metric", ["angular", "edit"])
def test_abx_pair_distances_indices(metric):
    book, codes, tokens, pairs = abx_index_ref.geometry_case()
    blocks = blocks_of(pairs[:4])
    M = book.shape[0]
    codes = torch.from_numpy(codes).cuda()
    codes_decoy = synth.randint("sc/abx/codes/decoy", tuple(codes.shape), M).cuda()
    if metric == "angular":
        table = abx.code_table(torch.from_numpy(book).cuda()).clone()
        table_decoy = abx.code_table(synth._normalish("sc/abx/book/decoy2", tuple(book.shape), synth.SEED).cuda()).clone()
        torch.cuda.synchronize()
        H.hold(lambda c, t: tuple(abx.pair_distances_indices(c, tokens, blocks, table=t)[:4]), [codes, table], [codes_decoy, table_decoy],
               label="abx pair_distances_indices, angular")
    else:
        H.hold(lambda c: tuple(abx.pair_distances_indices(c, tokens, blocks, n_codes=M, metric="edit")[:4]), [codes], [codes_decoy],
               label="abx pair_distances_indices, edit")


# ---------------------------------------------------------------------------------------------------- vocoder
@functools.lru_cache(maxsize=None)
def vocoder(kind):
    """"resident": the default options (paths 2 and 3); "launch": ``xcd`` = 0, the tests set the other options they need."""
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    voc = voc.cuda().eval()
    if kind == "launch":
        voc.set_option("xcd", 0)
    return voc


def launch_vocoder(fuse_fc2=1, use_graph=1, slots=0):
    voc = vocoder("launch")
    for name, value in (("fuse_fc2", fuse_fc2), ("use_graph", use_graph), ("slots", slots)):
        voc.set_option(name, value)
    return voc


def codes(tag, B, Tc):
    """-> (true [z, speaker], decoy [z, speaker], ragged n_codes) on the device."""
    make = lambda t: [synth.randint(f"sc/{t}/z{B}", (B, Tc), 512).cuda(), synth.randint(f"sc/{t}/s{B}", (B,), 102).cuda()]
    n_codes = [max(1, Tc - (b % Tc)) for b in range(B)] if B > 1 else None
    return make(tag), make(tag + "/decoy"), n_codes


def generate_entry(voc, n_codes, seed=17, utt_base=5):
    return lambda z, spk: voc.generate(z, spk, n_codes=n_codes, seed=seed, utt_base=utt_base, return_mulaw=True, async_=True)


def hold_generate(voc, B, Tc, path, label, n_codes="ragged", expect_busy=True):
    true, decoy, ragged = codes("gen", B, Tc)
    res = H.run(generate_entry(voc, ragged if n_codes == "ragged" else n_codes), true, decoy, label=label, expect_busy=expect_busy)
    assert voc.last_path() == path
    voc.check()                                             # after the final synchronise: no hand-off gave up, no placement miss
    res.verify()
    assert int((res["1"] != 0).sum()) > 0
    return res


@pytest.mark.parametrize("B,Tc,path", [(5, 4, 2), (20, 4, 2), (69, 2, 3)])
def test_generate_resident(B, Tc, path):
    hold_generate(vocoder("resident"), B, Tc, path, f"generate B={B} Tc={Tc} path {path}")


@pytest.mark.parametrize("B,Tc,fuse_fc2,use_graph,slots_per_launch,kind,expect_busy", [
    (3, 4, 1, 1, 16, 4.0, True),   # one tile, the fused fc2 || GRU launch
    (40, 4, 0, 1, 32, 1.0, True),  # three tiles as two tile groups (2 + 1): group 1 on side_stream, joined by ev_join
    (80, 4, 1, 1, 80, 5.0, True),  # five tiles: the large-batch kernel
    (40, 1, 0, 0, 48, 1.0, True),  # no graph, one launch after the other, one group: 960 launches
    (40, 4, 0, 0, 48, 1.0, False), # the same at Tc = 4: 3 840 launches, more than the runtime queues behind pending work
])
def test_generate_launch_path(B, Tc, fuse_fc2, use_graph, slots_per_launch, kind, expect_busy):
    """``use_graph`` = 0 at Tc = 4 is held to ordering only.  Its 3 840 launches do not fit behind work that has not started: the
    HIP runtime holds a bounded number of commands per stream and makes the host wait for room (measured on an MI355X behind a
    120 ms delay: 960 / 1 920 launches of this call at Tc = 1 / 2 return in 2.7 / 5.4 ms with the delay still ahead, 2 880 at
    Tc = 3 in 104 ms with it gone; plain ``x.add_(1)`` launches of torch do the same between 6 000 and 8 000).  The library does not
    synchronise there -- the same call at Tc = 1, well inside the bound, is held to that -- and the header's conventions now say
    so."""
    voc = launch_vocoder(fuse_fc2, use_graph)
    hold_generate(voc, B, Tc, 0, f"generate xcd=0 B={B} Tc={Tc} fuse_fc2={fuse_fc2} use_graph={use_graph}", expect_busy=expect_busy)
    times = voc.kernel_times(2)
    assert times[3] == slots_per_launch and times[4] == kind, times


def test_generate_second_group_outlasts_the_first():
    """48 utterances through 40 slots, xcd = 0, three-launch steps: the 32 long ones fill group 0 (1280 steps), the 16 short ones
    run two after the other in the 8 slots of group 1 (1920 steps), so ``side_stream`` is still decoding when the caller's stream
    has nothing left but the join.  (With one utterance per slot, group 1 holds the shortest and finishes first: a missing join
    would go unseen.)"""
    voc = launch_vocoder(0, 1, slots=40)
    try:
        res = hold_generate(voc, 48, 4, 0, "generate xcd=0 B=48 slots=40, group 1 longer", n_codes=[4] * 32 + [3] * 16)
        assert voc.last_slots() == 40 and voc.kernel_times(2)[3] == 32
        assert int((res["1"][32:, :960] != 0).sum()) > 0.9 * 16 * 960
    finally:
        voc.set_option("slots", 0)


@pytest.mark.parametrize("kind", ["resident", "launch"])
def test_staging_arena_back_to_back(kind):
    """Two generate calls on ``s`` behind one delay, no host synchronisation between them: the second call's tables must not
    reach the pinned arena before the first call's have been uploaded.  Both calls have the same shapes and the same set of
    lengths in another order (and other seeds and ids), so the tables differ in every word but not in size.  The second call may
    wait on the host for the first one's upload event (documented): ``busy`` is taken after the first."""
    voc = vocoder("resident") if kind == "resident" else launch_vocoder(1, 1)
    B, Tc = 5, 4
    t1, d1, n1 = codes("arena1", B, Tc)
    t2, d2, _ = codes("arena2", B, Tc)
    n2 = n1[::-1]

    def entry(z1, s1, z2, s2):
        a = voc.generate(z1, s1, n_codes=n1, seed=17, utt_base=5, return_mulaw=True, async_=True)
        busy = H.probe()
        b = voc.generate(z2, s2, n_codes=n2, seed=23, utt_base=50, return_mulaw=True, async_=True)
        return H.Early([a, b], busy)

    res = H.run(entry, t1 + t2, d1 + d2, label=f"two generate calls back to back ({kind})")
    voc.check()
    res.verify()
    assert not torch.equal(res["0.1"], res["1.1"])


def stream_entry(voc, B, n_codes, keep, alternate=False, between=None):
    """open, three chunks of 320 samples, the third once more (redo); every stream that was opened is left in ``keep``
    (closing one frees device memory, which synchronises: the test does it at the end)."""
    lib = _lib.load()

    def chunk(st, redo=False):
        w = torch.empty(B, 320, device="cuda")
        m = torch.empty(B, 320, dtype=torch.int64, device="cuda")
        if redo:
            _lib.check(lib.vqcpc_vocoder_stream_redo(st._st, ptr(w), ptr(m), cur()))
        else:
            _lib.check(lib.vqcpc_vocoder_stream_next(st._st, 320, ptr(w), ptr(m), cur()))
        return [w, m]

    def entry(z, spk):
        main = torch.cuda.current_stream()
        st = voc.generate_stream(z, spk, chunk_samples=320, n_codes=n_codes, seed=17, utt_base=5, return_mulaw=True)
        busy = H.probe()
        keep.append(st)
        side = torch.cuda.Stream() if alternate else None
        outs = []
        for i in range(3):
            if alternate and i == 1:                        # a -> b -> a, an event between
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    outs += chunk(st)
                main.wait_stream(side)
            else:
                outs += chunk(st)
            if between is not None and i == 0:              # the header allows generate() on the handle between chunks
                outs += list(voc.generate(*between, seed=5, utt_base=100, return_mulaw=True, async_=True))
        return H.Early(outs + chunk(st, redo=True), busy)
    return entry


@pytest.mark.parametrize("kind,B,mode", [("resident", 5, "one stream"), ("resident", 5, "two streams"), ("launch", 40, "two streams"),
                                         ("resident", 5, "generate between")])
def test_streaming(kind, B, mode):
    voc = vocoder("resident") if kind == "resident" else launch_vocoder(0, 1)
    true, decoy, n_codes = codes("stream", B, 4)
    want_w, want_m = voc.generate(*true, n_codes=n_codes, seed=17, utt_base=5, return_mulaw=True)
    between = None
    if mode == "generate between":
        between = codes("between", 3, 2)[0]
    keep = []
    try:
        res = H.run(stream_entry(voc, B, n_codes, keep, alternate=mode == "two streams", between=between), true, decoy,
                    label=f"stream_open + 3 x stream_next + stream_redo, {kind} B={B}, {mode}")
        assert voc.last_path() == (2 if kind == "resident" else 0)
        voc.check()
        res.verify()
    finally:
        torch.cuda.synchronize()
        for st in keep:
            st.close()
    want_b = voc.generate(*between, seed=5, utt_base=100, return_mulaw=True) if between is not None else None
    for got in map(list, res.got):
        if between is not None:
            assert torch.equal(got[2], want_b[0]) and torch.equal(got[3], want_b[1])
            del got[2:4]
        assert torch.equal(torch.cat(got[0:6:2], 1), want_w[:, :960]) and torch.equal(torch.cat(got[1:6:2], 1), want_m[:, :960])
        assert torch.equal(got[6], got[4]) and torch.equal(got[7], got[5])           # the redo repeats the third chunk


def test_logits():
    voc = vocoder("resident")
    lib, h = _lib.load(), voc._native()
    B, Tc = 2, 3
    Ts = 2 * 160 + 1
    (z, spk), (zd, sd), _ = codes("logits", B, Tc)
    x, xd = synth.randint("sc/logits/x", (B, Ts), 256).cuda(), synth.randint("sc/logits/x/decoy", (B, Ts), 256).cuda()

    def entry(x, z, spk):
        out = torch.empty(B, Ts, 256, device="cuda")
        _lib.check(lib.vqcpc_vocoder_logits(h, ptr(x), ptr(z), ptr(spk), B, Tc, Ts, ptr(out), cur()))
        return out

    H.hold(entry, [x, z, spk], [xd, zd, sd], label="logits B=2 Tc=3 Ts=321")
    voc.check()


def test_glue_and_condition():
    voc = vocoder("resident")
    lib, h = _lib.load(), voc._native()

    def glue(z, spk):
        out = torch.empty(z.size(0), 2 * z.size(1), 128, device="cuda")
        _lib.check(lib.vqcpc_vocoder_glue(h, ptr(z), ptr(spk), z.size(0), z.size(1), ptr(out), cur()))
        return out

    def condition(z, spk):
        out = torch.empty(z.size(0), 2 * z.size(1), 256, device="cuda")
        _lib.check(lib.vqcpc_vocoder_condition(h, ptr(z), ptr(spk), z.size(0), z.size(1), ptr(out), cur()))
        return out

    true, decoy, _ = codes("glue", 2, 3)
    H.hold(glue, true, decoy, label="glue B=2 Tc=3")
    true, decoy, _ = codes("cond", 17, 3)
    H.hold(condition, true, decoy, label="condition B=17 Tc=3")
    voc.check()


def test_nll():
    voc = vocoder("resident")
    lib, h = _lib.load(), voc._native()
    c = nll_ref.case_ragged()
    B, L = c["audio"].shape
    Tc = c["z"].shape[1]
    nc, na = _lib.int_array(c["n_codes"], B, "n_codes"), _lib.int_array(c["lengths"], B, "lengths")
    true = [c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda()]
    decoy = [synth.randint("sc/nll/a", (B, L), 256).cuda(), synth.randint("sc/nll/z", (B, Tc), 512).cuda(),
             synth.randint("sc/nll/s", (B,), 102).cuda()]

    def entry(audio, z, spk):
        nll_sum = torch.empty(B, dtype=torch.float64, device="cuda")
        n_scored, n_correct = torch.empty(B, dtype=torch.int64, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
        nll = torch.empty(B, L - 1, device="cuda")
        _lib.check(lib.vqcpc_vocoder_nll(h, ptr(audio), ptr(z), ptr(spk), B, Tc, L, nc, na, ptr(nll_sum), ptr(n_scored), ptr(n_correct),
                                         ptr(nll), cur()))
        return nll_sum, n_scored, n_correct, nll

    res = H.hold(entry, true, decoy, label="nll, ragged case of nll_ref")
    voc.check()
    assert res["1"].tolist() == [max(0, n - 1) for n in c["lengths"]]


def test_kernel_times_between_two_calls():
    """The measurement entry synchronises ``stream`` and returns after its launches: ordering only, and the stream must be idle
    when it returns.  It runs on the state the call before it left and the call after it must not see what it did."""
    voc = launch_vocoder(1, 1)
    lib, h = _lib.load(), voc._native()
    true, decoy, n_codes = codes("ktimes", 3, 2)
    seen = []

    def entry(z, spk):
        a = voc.generate(z, spk, n_codes=n_codes, seed=17, utt_base=5, return_mulaw=True, async_=True)
        out = (C.c_float * 5)()
        _lib.check(lib.vqcpc_vocoder_kernel_times(h, 3, out, cur()))
        seen.append((torch.cuda.current_stream().query(), out[0] > 0 and out[1] > 0 and out[2] > 0, out[3], out[4]))
        b = voc.generate(z, spk, n_codes=n_codes, seed=23, utt_base=9, return_mulaw=True, async_=True)
        return [a, b]

    H.hold(entry, true, decoy, expect_busy=False, label="generate, kernel_times, generate")
    voc.check()
    assert seen == [(True, True, 16.0, 4.0)] * (2 + H.N_STREAMS), seen


# ---------------------------------------------------------------------------------------------------- front ends
def waves(tag, lens, scale=0.3):
    w = torch.zeros(len(lens), max(lens))
    for b, n in enumerate(lens):
        w[b, :n] = torch.from_numpy(((synth.uniform01(f"sc/{tag}/{b}", n) * 2.0 - 1.0) * scale).astype(np.float32))
    return w.cuda()


def test_melfront():
    lens = [1600, 1377]
    H.hold(lambda w: preprocess.wave_to_mel(w, lengths=lens), [waves("mel", lens)], [waves("mel/decoy", lens, 0.1)], expect_busy=False,
           label="melfront_run B=2")


def test_resampler():
    """After the handle's first call of this length the header's one condition for a synchronisation (a longer clock table) is
    gone: held to "does not synchronise"."""
    lens = [2205, 1898]
    H.hold(lambda w: preprocess.resample(w, 22050, 16000, lengths=lens), [waves("rs", lens)], [waves("rs/decoy", lens, 0.1)],
           label="resampler_run 22050 -> 16000 B=2")


def test_loudness():
    lens = [8000, 7000]
    w, wd = waves("loud", lens), waves("loud/decoy", lens, 0.05)
    meter = loudness.Meter(16000)

    def integrated(t):
        lufs, blocks = meter.integrated_loudness(t, lengths=lens, return_blocks=True)
        return [lufs] + blocks

    res = H.hold(integrated, [w], [wd], expect_busy=False, label="loudness_integrated B=2")
    assert torch.isfinite(res["0"]).all()
    meas, target = res["0"].clone(), torch.tensor([-23.0, -20.0], dtype=torch.float64, device="cuda")
    meas_d, target_d = meas + 3.0, target - 2.0
    H.hold(lambda t, m, g: loudness.loudness(t, m, g, lengths=lens), [w, meas, target], [wd, meas_d, target_d], expect_busy=False,
           label="loudness_normalize B=2")


def test_report():
    """Prints what the session measured (the figures of the docstring)."""
    print("\nstream harness: delay %.1f ms at the end of the session, one torch.mm %.1f us" % (H.delay().target_ms(), H.delay().ms_per_mm * 1e3))
    for label, t_host, t_stream, delay_ms, busy in H.REPORT:
        print("  %-78s t_host %8.3f ms (%8.3f behind the delay)  delay %7.1f ms  busy %s" % (label, t_host, t_stream, delay_ms, busy))
