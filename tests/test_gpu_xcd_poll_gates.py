"""-m gpu: the resident decoders (ar_xcd_kernel<1|2|4>, ar_xcd_resume_kernel<...>) with exchange polls whose START is delayed to when
their data can exist.  What is in the tree: at four slots per XCD the chain waves nap before the first round of their h_t sweep
(csrc/ar_xcd.hip, XD_HNAP).  The same tests held the gates that were measured and dropped -- polls that wait for a word in LDS
("this workgroup has published", posted by the publishing wave at every step, live slots or not).
Either is a timing hint, every granule is still validated by its own tag, so every check is bit equality, mu-law classes and
waveform, with a path that has no such delay: the launch-per-step kernels (`xcd` = 0), or the one-shot call for the streamed case.

What could go wrong is a start that never comes (the call then times out and check() fails it) or one that comes early on something
left over from an earlier step or call (harmless to the bits, caught by the tags).  The shapes: 1, 9 and 16 utterances run one and
two slots per XCD, 17 and 25 four slots with idle slot columns, 32 all of them, 40 start a second utterance in a live column; ragged
lengths end slots while their neighbours run on; with one code frame on the even (odd) slot rows and three on the others, wave 0's
(wave 1's) slots are dead for two thirds of the call while the other wave's run on; the streamed case runs the resume kernels'
priming step at every chunk.  3 code frames = 960 sample steps per call.
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


def inputs(B, Tc):
    z = synth.randint(f"gates/z{B}", (B, Tc), 512).cuda()
    spk = synth.randint(f"gates/s{B}", (B,), 102).cuda()
    return z, spk


def both_paths(voc, z, spk, n_codes):
    B = z.shape[0]
    out = {}
    try:
        voc.set_option("xcd_slots", 32)
        for mode in (1, 0):
            voc.set_option("xcd", mode)
            wav, mu = voc.generate(z, spk, n_codes=n_codes, return_mulaw=True, seed=13, utt_base=3)
            voc.check()
            assert voc.last_path() == (2 if mode else 0)
            if mode:
                assert voc.last_slots() == min(B, 32)
            out[mode] = (wav.cpu(), mu.cpu())
    finally:
        voc.set_option("xcd_slots", 32)                  # the default (the option takes 1..32)
        voc.set_option("xcd", -1)
    return out


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [1, 9, 16, 17, 25, 32, 40])
def test_same_bits_as_the_launch_path(B, ragged):
    voc = vocoder()
    Tc = 3
    z, spk = inputs(B, Tc)
    n_codes = [1 + (7 * b) % Tc for b in range(B)] if ragged else None
    out = both_paths(voc, z, spk, n_codes)
    assert torch.equal(out[1][1], out[0][1]) and torch.equal(out[1][0], out[0][0])
    assert int((out[1][1] != 0).sum()) > 0.9 * FRAME * sum(n_codes or [Tc] * B)


@pytest.mark.parametrize("short", [0, 1])
def test_one_service_waves_slots_dead_for_two_thirds_of_the_call(short):
    # slot index b // 8: the even slots are wave 0's, the odd ones wave 1's
    voc = vocoder()
    B, Tc = 32, 3
    z, spk = inputs(B, Tc)
    n_codes = [1 if (b // 8) % 2 == short else 3 for b in range(B)]
    out = both_paths(voc, z, spk, n_codes)
    assert torch.equal(out[1][1], out[0][1]) and torch.equal(out[1][0], out[0][0])
    assert int((out[1][1] != 0).sum()) > 0.9 * FRAME * sum(n_codes)


def test_streamed_in_chunks_of_one_frame_same_bits_as_one_call():
    voc = vocoder()
    B, Tc = 20, 4
    z, spk = inputs(B, Tc)
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


@pytest.mark.parametrize("B", [1, 16, 32])
def test_two_calls_in_a_row_on_one_handle_give_equal_bits(B):
    # nothing a call leaves behind (LDS words, exchange area) may start the next call's polls on stale data
    voc = vocoder()
    z, spk = inputs(B, 3)
    got = []
    for _ in range(2):
        wav, mu = voc.generate(z, spk, return_mulaw=True, seed=21, utt_base=1)
        voc.check()
        assert voc.last_path() == 2
        got.append((wav.cpu(), mu.cpu()))
    assert torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][0], got[1][0])
    assert int((got[0][1] != 0).sum()) > 0.9 * FRAME * 3 * B
