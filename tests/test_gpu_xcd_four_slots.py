"""-m gpu: the per-XCD resident decoders in their four-slot form (ar_xcd_kernel<4>, all four matrix-pipe columns live) draw by draw
against the C oracle.  32 utterances put four decode slots on each of the 8 XCDs (slot s on XCD s % 8); the checked rows cover slots
0..3 of XCD 0 and of XCD 7.  Same criteria as test_gpu_xcd.py::test_draw_by_draw_against_the_oracle: a draw that differs from the
oracle's is within 2e-5 of the oracle's best Gumbel-max score on the GPU's own history, >= 99.9 % of draws are exact, and the
waveform is the mu-law table of the drawn samples.
"""
import numpy as np
import pytest

import oracle
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu

B, TC, STEPS, SEED, UTT_BASE = 32, 2, 480, 13, 11
ROWS = (0, 8, 16, 24, 7, 15, 23, 31)


def test_four_slots_draw_by_draw_against_the_oracle():
    sd = synth.vocoder_state_dict()
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(sd)
    voc = voc.to("cuda").eval()
    voc.set_option("xcd", 1)
    z = synth.randint("xcd4/oz", (B, TC), 512)
    spk = synth.randint("xcd4/os", (B,), 102)
    wav, mu = voc.generate(z.cuda(), spk.cuda(), seed=SEED, utt_base=UTT_BASE, return_mulaw=True, max_steps=STEPS)
    voc.check()
    assert voc.last_path() == 2
    wav, mu = wav.cpu().numpy(), mu.cpu().numpy()
    exact = total = 0
    for b in ROWS:
        s_gpu = mu[b, :STEPS]
        inputs = np.concatenate([[128], s_gpu[:-1]])
        r = oracle.vocoder_generate(sd, z[b].numpy(), int(spk[b]), seed=SEED, utterance=UTT_BASE + b, n_steps=STEPS,
                                    inputs=inputs, want_logits=True)
        for t in np.nonzero(r["samples"] != s_gpu)[0]:
            pick, sc = oracle.sample_from_logits(r["logits"][t], SEED, UTT_BASE + b, int(t))
            assert sc[pick] - sc[int(s_gpu[t])] <= 2e-5, (b, int(t))
        exact += int((r["samples"] == s_gpu).sum())
        total += STEPS
        assert np.array_equal(wav[b, :STEPS], np.array([oracle.mulaw_decode(int(s)) for s in s_gpu], np.float32))
        assert not wav[b, STEPS:].any()
    assert exact >= 0.999 * total
