"""-m gpu: the per-XCD resident decoders in their four-slot form (ar_xcd_kernel<4>, all four matrix-pipe columns live) draw by draw
against the C oracle.  32 utterances put four decode slots on each of the 8 XCDs (slot s on XCD s % 8); the checked rows cover slots
0..3 of XCD 0 and of XCD 7.  Same criteria as test_gpu_xcd.py::test_draw_by_draw_against_the_oracle: a draw that differs from the
oracle's is within 2e-5 of the oracle's best Gumbel-max score on the GPU's own history, >= 99.9 % of draws are exact, and the
waveform is the mu-law table of the drawn samples.
"""
import pytest

import decode_harness as H
import oracle

pytestmark = pytest.mark.gpu

B, TC, STEPS, SEED, UTT_BASE = 32, 2, 480, 13, 11
ROWS = (0, 8, 16, 24, 7, 15, 23, 31)


def test_four_slots_draw_by_draw_against_the_oracle():
    voc, sd = H.new_vocoder()
    voc.set_option("xcd", 1)
    z, spk = H.inputs("xcd4/o?", B, TC, device="cpu")
    wav, mu = H.decode(voc, z.cuda(), spk.cuda(), path=2, seed=SEED, utt_base=UTT_BASE, max_steps=STEPS)
    stats = oracle.judge_draws(sd, z, spk, mu, seed=SEED, utt_ids=range(UTT_BASE, UTT_BASE + B), rows=ROWS, steps=STEPS, wav=wav)
    assert sum(e for _, e in stats) >= 0.999 * sum(n for n, _ in stats)
