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

import decode_harness as H

pytestmark = pytest.mark.gpu
vocoder = H.Handles()


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("B", [17, 25, 32, 40])
def test_same_bits_as_the_launch_path(B, ragged):
    voc, _ = vocoder()
    Tc = 3
    z, spk = H.inputs(f"halves/?{B}", B, Tc)
    n_codes = H.ragged_sevens(B, Tc) if ragged else None
    # 17..32 slots: four per XCD, ar_xcd_kernel<4>
    resident, launch = H.path_pair(voc, z, spk, {"xcd_slots": 32, "xcd": 1}, {"xcd": 0}, path=2, slots=min(B, 32), n_codes=n_codes,
                                   seed=13, utt_base=3)
    H.assert_same_bits(resident, launch)
    H.assert_live(resident[1], n_codes or [Tc] * B)


def test_streamed_in_chunks_of_one_frame_same_bits_as_one_call():
    voc, _ = vocoder()
    B, Tc = 20, 4
    z, spk = H.inputs(f"halves/?{B}", B, Tc)
    want = H.decode(voc, z, spk, path=2, seed=17, utt_base=5)
    got = H.streamed(voc, z, spk, H.FRAME, path=2, slots=(17, 32), chunks=Tc, seed=17, utt_base=5)      # ar_xcd_resume_kernel<4>
    H.assert_same_bits(got, want)
    H.assert_live(got[1], [Tc] * B)
