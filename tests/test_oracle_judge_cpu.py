"""oracle.judge_draws, the one statement of the draw rule every decoder test and smoke() rely on, can say no.  The decode judged is
the C oracle's own free run of one utterance (48 steps): accepted as it is, refused with one draw replaced by the runner-up where
the runner-up is farthest behind, with one waveform sample altered, and with one sample behind the end."""
import numpy as np
import pytest

import oracle
from vectorquantizedcpc_amd import synth

STEPS, SEED, UTT = 48, 13, 3


@pytest.fixture(scope="module")
def run():
    sd = synth.vocoder_state_dict()
    z, spk = synth.randint("h/z", (1, 1), 512), synth.randint("h/s", (1,), 102)
    r = oracle.vocoder_generate(sd, z[0].numpy(), int(spk[0]), seed=SEED, utterance=UTT, n_steps=STEPS, want_logits=True)
    mu, wav = np.zeros((1, 320), np.int64), np.zeros((1, 320), np.float32)
    mu[0, :STEPS], wav[0, :STEPS] = r["samples"], r["wav"]

    def judge(mu, wav):
        return oracle.judge_draws(sd, z, spk, mu, seed=SEED, utt_ids=[UTT], rows=[0], steps=STEPS, wav=wav)
    return judge, mu, wav, r["logits"]


def test_the_oracles_own_run_is_exact(run):
    judge, mu, wav, _ = run
    assert judge(mu, wav) == [(STEPS, STEPS)]
    assert judge(mu, None) == [(STEPS, STEPS)]


def test_a_runner_up_draw_is_refused_by_row_and_step(run):
    judge, mu, wav, logits = run
    scores = np.sort(np.stack([oracle.sample_from_logits(logits[t], SEED, UTT, t)[1] for t in range(STEPS)]), axis=1)
    gaps = scores[:, -1] - scores[:, -2]
    t = int(gaps.argmax())
    assert gaps[t] > 1e-3                                  # far outside the 2e-5 tie window
    sc = oracle.sample_from_logits(logits[t], SEED, UTT, t)[1]
    bad = mu.copy()
    bad[0, t] = np.argsort(sc)[-2]
    assert bad[0, t] != mu[0, t]
    with pytest.raises(AssertionError, match=rf"row 0, step {t}:"):
        judge(bad, None)


def test_a_wrong_waveform_or_a_sample_behind_the_end_is_refused(run):
    judge, mu, wav, _ = run
    bad = wav.copy()
    bad[0, 17] = np.nextafter(bad[0, 17], np.float32(2.0))
    with pytest.raises(AssertionError, match="row 0: the waveform"):
        judge(mu, bad)
    bad = wav.copy()
    bad[0, STEPS] = 1e-3
    with pytest.raises(AssertionError, match="row 0: samples behind the end"):
        judge(mu, bad)
