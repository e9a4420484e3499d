"""-m gpu: the four-slot resident decoders (ar_xcd_kernel<4> / ar_xcd_resume_kernel<4>) with ONE operand read per group of 8 chain
terms: the two halves of a wave read different 16-byte words of h_t and the matrix instruction's B lane-group pattern picks the half
that holds the term (csrc/ar_chain.h, mfma_group8).  Every check is bit equality, mu-law classes and waveform, with a path that does
not run those chains: the launch-per-step kernels (`xcd` = 0), or the one-shot call for the streamed case.

The shapes are the smallest in which each thing that could go wrong does: a wrong half or a wrong term order inside a group changes
every W_hh and fc1 row from the first sample on; 17 utterances leave XCDs 1..7 with slot columns they do not run (XCD 0: 3 of 4, the
others 2 of 4) and 25 one; 3 code frames = 960 sample steps cross the chain waves' pause between two groups (XD_GSPLIT) 960 times per
wave; ragged lengths end slots while their neighbours run on; 40 utterances through 32 slots start a second utterance in a column
that was live; the streamed case runs the resume kernel's priming step at every chunk.
"""
import pytest
import torch

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu
FRAME = 320                     # samples per code frame
_cache = {}


def vocoder():
    if "v" not in _cache:
        v = V.Vocoder(V.ConfVocoder())
        v.load_state_dict(synth.vocoder_state_dict())
        _cache["v"] = v.to("cuda").eval()
    return _cache["v"]


def inputs(B, Tc, ragged):
    z = synth.randint(f"halves/z{B}", (B, Tc), 512).cuda()
    spk = synth.randint(f"halves/s{B}", (B,), 102).cuda()
    n_codes = [1 + (7 * b) % Tc for b in range(B)] if ragged else None
    return z, spk, n_codes


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [17, 25, 32, 40])
def test_same_bits_as_the_launch_path(B, ragged):
    voc = vocoder()
    Tc = 3
    z, spk, n_codes = inputs(B, Tc, ragged)
    out = {}
    try:
        voc.set_option("xcd_slots", 32)
        for mode in (1, 0):
            voc.set_option("xcd", mode)
            wav, mu = voc.generate(z, spk, n_codes=n_codes, return_mulaw=True, seed=13, utt_base=3)
            voc.check()
            assert voc.last_path() == (2 if mode else 0)
            if mode:
                assert voc.last_slots() == min(B, 32)          # 17..32 slots: four per XCD, ar_xcd_kernel<4>
            out[mode] = (wav.cpu(), mu.cpu())
    finally:
        voc.set_option("xcd_slots", 32)                  # the default (the option takes 1..32)
        voc.set_option("xcd", -1)
    assert torch.equal(out[1][1], out[0][1]) and torch.equal(out[1][0], out[0][0])
    assert int((out[1][1] != 0).sum()) > 0.9 * FRAME * sum(n_codes or [Tc] * B)


def test_streamed_in_chunks_of_one_frame_same_bits_as_one_call():
    voc = vocoder()
    B, Tc = 20, 4
    z, spk, _ = inputs(B, Tc, False)
    want_w, want_m = voc.generate(z, spk, return_mulaw=True, seed=17, utt_base=5)
    voc.check()
    assert voc.last_path() == 2
    ws, ms = [], []
    for w, m in voc.generate_stream(z, spk, chunk_samples=FRAME, return_mulaw=True, seed=17, utt_base=5):
        assert voc.last_path() == 2 and 17 <= voc.last_slots() <= 32      # ar_xcd_resume_kernel<4>
        ws.append(w)
        ms.append(m)
    assert len(ws) == Tc
    got_w, got_m = torch.cat(ws, 1), torch.cat(ms, 1)
    assert got_w.shape == want_w.shape
    assert torch.equal(got_m, want_m) and torch.equal(got_w, want_w)
    assert int((got_m != 0).sum()) > 0.9 * FRAME * Tc * B
