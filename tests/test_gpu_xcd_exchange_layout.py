"""-m gpu: the exchange regions of the per-XCD resident decoders (csrc/ar_chain.h: h_t [rank][slot][32], a_t [slot][rank][8]) and the
16-byte sweep of a_t (two independent {tag, value} granules per load), where a permutation of a region or of the lanes that sweep it
can go wrong and the shapes of test_gpu_xcd.py may not show it.  Every case is 2 code frames cut at max_steps = 320 samples on the
resident decoders (``xcd`` 1, last_path() == 2) against the launch-per-step kernels (``xcd`` 0): waveforms and mu-law classes must be
EQUAL.  An utterance's length is a whole number of code frames (320 samples each) -- ``n_codes`` is the interface's only per-utterance
length -- so the ragged cases run their two frames out (max_steps 0): 320 next to 640 samples; a slot that is through keeps publishing
tagged zeros, and its neighbours in a 16-byte pair must go on without it.
"""
import pytest
import torch

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu
TC, STEPS, SEED, UTT_BASE = 2, 320, 29, 3
_cache = {}


def _vocoder(fresh=False):
    if fresh or "v" not in _cache:
        v = V.Vocoder(V.ConfVocoder())
        v.load_state_dict(synth.vocoder_state_dict())
        v = v.to("cuda").eval()
        if fresh:
            return v
        _cache["v"] = v
    return _cache["v"]


def _inputs(B, ragged):
    z = synth.randint(f"xl/z{B}", (B, TC), 512).cuda()
    spk = synth.randint(f"xl/s{B}", (B,), 102).cuda()
    # 1, 2, 2, 1, 2, 1, 1, 2, ...: both lengths in every XCD, in both granules of a pair and in neighbouring pairs
    n_codes = [1 + ((b * 5 + b // 8) % 3 != 0) for b in range(B)] if ragged else None
    return z, spk, n_codes


def _launch_path(B, ragged):
    """The launch-per-step kernels' bits for a case: computed once, shared by the tests that compare against them."""
    key = ("ref", B, ragged)
    if key not in _cache:
        voc = _vocoder()
        z, spk, n_codes = _inputs(B, ragged)
        voc.set_option("xcd", 0)
        try:
            wav, mu = voc.generate(z, spk, n_codes=n_codes, seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=0 if ragged else STEPS)
            voc.check()
            assert voc.last_path() != 2
        finally:
            voc.set_option("xcd", -1)
        _cache[key] = (wav.cpu(), mu.cpu())
    return _cache[key]


def _resident(voc, B, ragged, **opts):
    z, spk, n_codes = _inputs(B, ragged)
    voc.set_option("xcd", 1)
    for k, v in opts.items():
        voc.set_option(k, v)
    try:
        wav, mu = voc.generate(z, spk, n_codes=n_codes, seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=0 if ragged else STEPS,
                               async_=True)
        voc.check()                                        # no hand-off timed out
        assert voc.last_path() == 2
    finally:
        voc.set_option("xcd", -1)
    return wav.cpu(), mu.cpu(), n_codes


def _assert_equal(got, want, B, n_codes):
    assert torch.equal(got[1], want[1]) and torch.equal(got[0], want[0])
    assert int((got[1] != 0).sum()) > 0.9 * 320 * sum(n_codes or [1] * B)


@pytest.mark.parametrize("B", [17, 25, 31])
def test_partially_filled_four_slot_xcds(B):
    """ar_xcd_kernel<4> with XCDs that run two or three of their four slots: the other granules of a 16-byte load are zeros
    or stale and must be neither waited for nor used."""
    wav, mu, n_codes = _resident(_vocoder(), B, False)
    _assert_equal((wav, mu), _launch_path(B, False), B, n_codes)


def test_every_slot_and_both_granules_of_a_pair_ragged():
    """32 utterances of 320 and 640 samples: every slot of every XCD, neighbours of a pair ending at different steps; check()
    inside _resident says that no wait ran into its deadline."""
    wav, mu, n_codes = _resident(_vocoder(), 32, True)
    assert {1, 2} == set(n_codes[0::8]) and {1, 2} == set(n_codes[7::8])      # both lengths among the slots of XCD 0 and of XCD 7
    _assert_equal((wav, mu), _launch_path(32, True), 32, n_codes)
    for b, n in enumerate(n_codes):
        assert not mu[b, 320 * n:].any()


@pytest.mark.parametrize("B,ragged", [(16, True), (9, False), (8, True), (1, False)])
def test_two_slot_and_one_slot_forms(B, ragged):
    wav, mu, n_codes = _resident(_vocoder(), B, ragged)
    _assert_equal((wav, mu), _launch_path(B, ragged), B, n_codes)


def test_more_utterances_than_slots():
    """40 utterances of 320 and 640 samples through 32 slots: a slot's second utterance starts in the middle of the call -- the tags run on, the
    rows change."""
    voc = _vocoder()
    try:
        wav, mu, n_codes = _resident(voc, 40, True, xcd_slots=32)
    finally:
        voc.set_option("xcd_slots", 32)
    _assert_equal((wav, mu), _launch_path(40, True), 40, n_codes)


def test_stream_of_two_chunks_equals_one_shot():
    """The resume kernels share the sweeps: one code frame in two chunks of 160 samples equals the one-shot call."""
    voc = _vocoder()
    z, spk, _ = _inputs(32, False)
    z = z[:, :1].contiguous()
    voc.set_option("xcd", 0)
    want = [t.cpu() for t in voc.generate(z, spk, seed=SEED, utt_base=UTT_BASE, return_mulaw=True)]
    voc.set_option("xcd", 1)
    try:
        st = voc.generate_stream(z, spk, chunk_samples=160, seed=SEED, utt_base=UTT_BASE, return_mulaw=True)
        chunks = []
        for w, m in st:
            assert voc.last_path() == 2
            chunks.append((w.cpu(), m.cpu()))
        voc.check()
    finally:
        voc.set_option("xcd", -1)
    assert [c[0].shape[1] for c in chunks] == [160, 160]
    assert want[1].shape[1] == 320 and int((want[1] != 0).sum()) > 0.9 * 320 * 32
    assert torch.equal(torch.cat([c[1] for c in chunks], 1), want[1]) and torch.equal(torch.cat([c[0] for c in chunks], 1), want[0])


def test_agent_scope_stores_same_bits():
    """The publishers' stride changed with the layout: agent-scope stores give the bits of the default workgroup-scope ones."""
    voc = _vocoder()
    try:
        wav, mu, n_codes = _resident(voc, 32, False, xcd_agent_stores=1)
    finally:
        voc.set_option("xcd_agent_stores", 0)
    _assert_equal((wav, mu), _launch_path(32, False), 32, n_codes)


def test_a_handoff_that_never_comes_is_still_reported():
    """One worker skips one candidate publish (the library's bounded-wait test hook, once): the waits behind it give up after
    the shortened deadline -- a_t and h_t of the next step never come either, so every sweep's exit is taken -- check() reports the
    timeout for that call, and the repeated call, on the fallback, gives the launch path's bits."""
    voc = _vocoder(fresh=True)
    z, spk, _ = _inputs(32, False)
    voc.set_option("xcd", 1)
    voc.set_option("xcd_timeout_ms", 20)
    voc.set_option("xcd_debug_drop_step", 200)
    voc.generate(z, spk, seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=STEPS, async_=True)
    with pytest.raises(RuntimeError, match="timed out"):
        voc.check()
    voc.set_option("xcd_debug_drop_step", -1)
    wav, mu = voc.generate(z, spk, seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=STEPS)
    assert voc.last_path() == 0
    want = _launch_path(32, False)
    assert torch.equal(mu.cpu(), want[1]) and torch.equal(wav.cpu(), want[0])
