"""-m gpu: the four-slot resident decoders (ar_xcd_kernel<4>, ar_xcd_resume_kernel<4>) exchange h_t as 4-byte words -- the value's
own bits with bit 30, which |h| < 2 leaves free, replaced by the step's parity (csrc/ar_shared.h: xd_word_h) -- swept by the chain
waves with one 16-byte load of four words per lane; a_t can be built the same way (xd_word_a, bit 31; -DXD_WORDS_A=4) and measured
slower, so it and the one- and two-slot kernels keep their 8-byte {tag, value} granules.  The format changes no arithmetic, so every
check is bit equality, mu-law classes and waveform, with a path that has no such format: the launch-per-step kernels (`xcd` = 0),
or the one-shot call for the streamed case.

What could go wrong: a word taken for this step's that is the last step's (one parity bit is all that tells them apart), a chunk
whose four words were not all validated, a chunk of an idle slot column waited for, a value put at the wrong place of the LDS copy,
or something a call leaves in the exchange area read by the next.  The shapes (those of test_gpu_xcd_poll_gates.py): 1, 9 and 16
utterances run one and two slots per XCD, 17 and 25 four slots with idle slot columns, whose chunks are skipped, 32 all of them, 40
start a second utterance in a live column; ragged lengths end slots while their neighbours run on; one code frame on one service
wave's slot rows and three on the other's; the streamed case runs the resume kernels' priming step and h_in at every chunk; two calls
in a row on one handle; agent-scope stores (the words go out with sc1).  3 code frames = 960 sample steps per
call: both parities, 480 reuses of every word.

The word helpers themselves run in a probe (csrc/gate_probe.hip) against a NumPy restatement.  A hidden value the word cannot carry
(NaN, inf, |h| >= 2) ends the call in order: check() names it, without waiting for the hand-off timeout, the handle goes to the
launch path, and the repeated call gives what a handle on that path gives.
"""
import time

import numpy as np
import pytest
import torch

import decode_harness as H
from vectorquantizedcpc_amd import _lib, synth

pytestmark = pytest.mark.gpu
vocoder = H.Handles()

HBIT, ABIT = np.uint32(1 << 30), np.uint32(1 << 31)


def inputs(B, Tc):
    return H.inputs(f"words/?{B}", B, Tc)


def both_paths(voc, z, spk, n_codes, **resident):
    return H.path_pair(voc, z, spk, {"xcd_slots": 32, "xcd": 1, **resident}, {"xcd": 0}, path=2, slots=min(z.shape[0], 32),
                       n_codes=n_codes, seed=13, utt_base=3)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [1, 9, 16, 17, 25, 32, 40])
def test_same_bits_as_the_launch_path(B, ragged):
    voc, _ = vocoder()
    Tc = 3
    z, spk = inputs(B, Tc)
    n_codes = H.ragged_sevens(B, Tc) if ragged else None
    resident, launch = both_paths(voc, z, spk, n_codes)
    H.assert_same_bits(resident, launch)
    H.assert_live(resident[1], n_codes or [Tc] * B)


@pytest.mark.parametrize("short", [0, 1])
def test_one_service_waves_slots_dead_for_two_thirds_of_the_call(short):
    # slot index b // 8: the even slots are wave 0's, the odd ones wave 1's
    voc, _ = vocoder()
    B, Tc = 32, 3
    z, spk = inputs(B, Tc)
    n_codes = [1 if (b // 8) % 2 == short else 3 for b in range(B)]
    resident, launch = both_paths(voc, z, spk, n_codes)
    H.assert_same_bits(resident, launch)
    H.assert_live(resident[1], n_codes)


def test_streamed_in_chunks_of_one_frame_same_bits_as_one_call():
    voc, _ = vocoder()
    B, Tc = 20, 4
    z, spk = inputs(B, Tc)
    want = H.decode(voc, z, spk, path=2, seed=17, utt_base=5)
    got = H.streamed(voc, z, spk, H.FRAME, path=2, slots=(17, 32), chunks=Tc, seed=17, utt_base=5)      # ar_xcd_resume_kernel<4>
    H.assert_same_bits(got, want)
    H.assert_live(got[1], [Tc] * B)


@pytest.mark.parametrize("B", [1, 16, 32])
def test_two_calls_in_a_row_on_one_handle_give_equal_bits(B):
    # the launcher zeroes the exchange area: the second call's first step must not take the first call's last words for its own
    voc, _ = vocoder()
    z, spk = inputs(B, 3)
    got = [H.decode(voc, z, spk, path=2, seed=21, utt_base=1) for _ in range(2)]
    H.assert_same_bits(got[0], got[1])
    H.assert_live(got[0][1], [3] * B)


def test_agent_scope_stores_same_bits():
    voc, _ = vocoder()
    z, spk = inputs(32, 3)
    resident, launch = both_paths(voc, z, spk, None, xcd_agent_stores=1)
    H.assert_same_bits(resident, launch)
    H.assert_live(resident[1], [3] * 32)


# ---- the word helpers on the GPU

def _probe(bits, is_a):
    """(2 parities, 4 rows, n) uint32: word, fits, parity read back (2: both or none accepted), value bits."""
    lib = _lib.load()
    d_bits = torch.from_numpy(bits.view(np.int32)).cuda()
    d_out = torch.full((2, 4, len(bits)), -1, dtype=torch.int32, device="cuda")
    _lib.check(lib.vqcpc_probe_words(d_bits.data_ptr(), len(bits), is_a, d_out.data_ptr(), _lib.current_stream()))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32)


def _assert_words(bits, is_a, fit):
    bit, shift = (ABIT, 31) if is_a else (HBIT, 30)
    got = _probe(bits, is_a)
    assert np.array_equal((bits & bit) == 0, np.full(len(bits), fit))
    for par in (0, 1):
        word, fits, parity, value = got[par]
        assert np.array_equal(word, (bits & ~bit) | np.uint32(par << shift))
        assert np.array_equal(fits, np.full(len(bits), 1 if fit else 0, np.uint32))
        assert np.array_equal(parity, np.full(len(bits), par, np.uint32))
        assert np.array_equal(value, bits & ~bit)
        if fit:
            assert np.array_equal(value, bits)                       # the value round-trips bit for bit


def _f32_bits(*values):
    return np.array(values, np.float32).view(np.uint32)


def test_hidden_words_round_trip_every_256th_pattern_below_two():
    below_two = np.arange(0, 1 << 30, 256, dtype=np.uint32)            # +0 .. just under 2.0, denormals included
    edges = np.concatenate([_f32_bits(0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38),
                            np.array([0x3FFFFFFF, 0xBFFFFFFF, 0x007FFFFF, 0x807FFFFF, 0x00800000], np.uint32)])   # largest below 2, denormal ends
    for sign in (np.uint32(0), ABIT):
        _assert_words(np.concatenate([below_two | sign, edges]), 0, True)


def test_hidden_values_that_do_not_fit_are_reported():
    wide = np.arange(1 << 30, 1 << 31, 4096, dtype=np.uint32)           # 2.0 .. NaN
    edges = np.concatenate([_f32_bits(2.0, -2.0, np.inf, -np.inf, 3.0e38, 1e9), np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32)])
    _assert_words(np.concatenate([wide, wide | ABIT, edges]), 0, False)


def test_activation_words_round_trip_every_256th_pattern_from_zero_to_inf():
    pos = np.arange(0, 0x7F800000 + 1, 256, dtype=np.uint32)             # +0 .. +inf
    assert pos[-1] == 0x7F800000
    edges = np.concatenate([_f32_bits(0.0, 1.0, 1e-45, 1.1754942e-38, 3.4028235e38, np.inf), np.array([0x007FFFFF, 0x7F7FFFFF], np.uint32)])
    _assert_words(np.concatenate([pos, edges]), 1, True)
    _assert_words(np.concatenate([pos[::16] | ABIT, _f32_bits(-0.0, -1.0, -np.inf)]), 1, False)      # a sign bit is reported, not carried


# ---- the range path: the kernel's own orderly exit

def test_a_hidden_state_that_does_not_fit_ends_the_call_and_the_rerun_is_the_launch_paths():
    sd = synth.vocoder_state_dict()
    sd["rnnms.ar.rnn.bias_hh_l0"] = sd["rnnms.ar.rnn.bias_hh_l0"].clone()
    sd["rnnms.ar.rnn.bias_hh_l0"][5 * 28 + 3] = float("nan")           # gate r of unit 3 of worker 5
    z, spk = H.inputs("words/?nan", 20, 2)
    H.decode(vocoder()[0], z[:, :1].contiguous(), spk, path=2, seed=9)      # a process that has never decoded pays for that first, not below
    voc, _ = vocoder(fresh=True, sd=sd)
    voc.set_option("xcd", 1)
    voc.set_option("xcd_timeout_ms", 10000)                            # what a call that waited for the timeout would take
    t0 = time.perf_counter()
    voc.generate(z, spk, seed=9, utt_base=0, return_mulaw=True, async_=True)
    with pytest.raises(RuntimeError, match=r"hidden state.*call #1 of this handle|call #1 of this handle.*hidden state"):
        voc.check()
    took = time.perf_counter() - t0
    print(f"range abort: {took * 1e3:.1f} ms")
    assert took < 1.0
    assert voc.last_path() == 2
    got = H.decode(voc, z, spk, path=0, seed=9, utt_base=0)           # the handle has fallen back
    ref, _ = vocoder(fresh=True, sd=sd)
    ref.set_option("xcd", 0)
    want = H.decode(ref, z, spk, path=0, seed=9, utt_base=0)
    assert torch.equal(got[1], want[1])
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
