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

import decode_harness as H

pytestmark = pytest.mark.gpu
vocoder = H.Handles()


def inputs(B, Tc):
    return H.inputs(f"gates/?{B}", B, Tc)


def both_paths(voc, z, spk, n_codes):
    return H.path_pair(voc, z, spk, {"xcd_slots": 32, "xcd": 1}, {"xcd": 0}, path=2, slots=min(z.shape[0], 32), n_codes=n_codes,
                       seed=13, utt_base=3)


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
    # nothing a call leaves behind (LDS words, exchange area) may start the next call's polls on stale data
    voc, _ = vocoder()
    z, spk = inputs(B, 3)
    got = [H.decode(voc, z, spk, path=2, seed=21, utt_base=1) for _ in range(2)]
    H.assert_same_bits(got[0], got[1])
    H.assert_live(got[0][1], [3] * B)
