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

import decode_harness as H

pytestmark = pytest.mark.gpu
TC, STEPS, SEED, UTT_BASE = 2, 320, 29, 3
vocoder = H.Handles()
CASES = H.CutCases(vocoder, "xl/?{B}", TC, STEPS, SEED, UTT_BASE)


@pytest.mark.parametrize("B", [17, 25, 31])
def test_partially_filled_four_slot_xcds(B):
    """ar_xcd_kernel<4> with XCDs that run two or three of their four slots: the other granules of a 16-byte load are zeros
    or stale and must be neither waited for nor used."""
    CASES.assert_equal(CASES.resident(B, False), B, False)


def test_every_slot_and_both_granules_of_a_pair_ragged():
    """32 utterances of 320 and 640 samples: every slot of every XCD, neighbours of a pair ending at different steps; check()
    inside CASES.resident says that no wait ran into its deadline."""
    n_codes = H.ragged_pairs(32)
    assert {1, 2} == set(n_codes[0::8]) and {1, 2} == set(n_codes[7::8])      # both lengths among the slots of XCD 0 and of XCD 7
    CASES.assert_equal(CASES.resident(32, True), 32, True)


@pytest.mark.parametrize("B,ragged", [(16, True), (9, False), (8, True), (1, False)])
def test_two_slot_and_one_slot_forms(B, ragged):
    CASES.assert_equal(CASES.resident(B, ragged), B, ragged)


def test_more_utterances_than_slots():
    """40 utterances of 320 and 640 samples through 32 slots: a slot's second utterance starts in the middle of the call -- the tags run on, the
    rows change."""
    CASES.assert_equal(CASES.resident(40, True, xcd_slots=32), 40, True)


def test_stream_of_two_chunks_equals_one_shot():
    """The resume kernels share the sweeps: one code frame in two chunks of 160 samples equals the one-shot call."""
    CASES.assert_stream_equals_one_shot(32, chunk=160)


def test_agent_scope_stores_same_bits():
    """The publishers' stride changed with the layout: agent-scope stores give the bits of the default workgroup-scope ones."""
    CASES.assert_equal(CASES.resident(32, False, xcd_agent_stores=1), 32, False)


def test_a_handoff_that_never_comes_is_still_reported():
    """One worker skips one candidate publish (the library's bounded-wait test hook, once): the waits behind it give up after
    the shortened deadline -- a_t and h_t of the next step never come either, so every sweep's exit is taken -- check() reports the
    timeout for that call, and the repeated call, on the fallback, gives the launch path's bits."""
    voc, _ = vocoder(fresh=True)
    z, spk, _ = CASES.inputs(32, False)
    voc.set_option("xcd", 1)
    voc.set_option("xcd_timeout_ms", 20)
    voc.set_option("xcd_debug_drop_step", 200)
    voc.generate(z, spk, seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=STEPS, async_=True)
    with pytest.raises(RuntimeError, match="timed out"):
        voc.check()
    voc.set_option("xcd_debug_drop_step", -1)
    wav, mu = voc.generate(z, spk, seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=STEPS)
    assert voc.last_path() == 0
    want = CASES.launch_bits(32, False)
    assert torch.equal(mu.cpu(), want[1]) and torch.equal(wav.cpu(), want[0])
