"""-m gpu: the matrix-core per-XCD resident decoders (csrc/ar_xcm.hip: 16 decode slots per XCD, the default decode path
between 69 and 511 utterances in flight).

Checked like the VALU form in test_gpu_xcd.py: (1) bit for bit against the launch-per-step kernels (`xcd` = 0), which
test_gpu_vocoder.py checks against the oracles on their own; (2) draw by draw against the C oracle on the same history
(the parity-unpinned self-oracle, tolerance 2e-5 on the Gumbel-max score); (3) size-independent properties at configs[3]'s
single-GPU form (256 x 32 000 through 128 slots): an utterance alone equals itself in the batch, fewer slots give the same
samples; (4) the abort path of its in-kernel hand-offs.
"""
import pytest
import torch

import decode_harness as H
import oracle
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu
vocoder = H.Handles()


def _both_paths(voc, z, spk, **kw):
    return H.path_pair(voc, z, spk, {"xcd": -1, "xcm": 1}, {"xcd": 0, "xcm": 0}, path=3, **kw)


@pytest.mark.parametrize("B,Tc,ragged", [(1, 2, False), (7, 3, True), (16, 2, False), (17, 3, True), (40, 2, True), (128, 2, False),
                                         (150, 3, True)])
def test_same_samples_as_the_launch_path(B, Tc, ragged):
    voc, _ = vocoder()
    z, spk = H.inputs(f"xcm/?{B}", B, Tc)
    n_codes = H.ragged_countdown(B, Tc) if ragged else None
    xcm, launch = _both_paths(voc, z, spk, n_codes=n_codes, seed=13, utt_base=3)
    H.assert_same_bits(xcm, launch)
    H.assert_live(xcm[1], n_codes or [Tc] * B)


def _draws_against_the_oracle(B, Tc, steps, tag, seed, utt_base, rows):
    """(steps, exact draws) of ``rows`` of one call on the matrix-core decoders, every draw and the waveform judged by the C oracle."""
    voc, sd = vocoder()
    z, spk = H.inputs(tag, B, Tc, device="cpu")
    with H.options(voc, xcm=1):
        wav, mu = H.decode(voc, z.cuda(), spk.cuda(), path=3, seed=seed, utt_base=utt_base, max_steps=steps)
    return oracle.judge_draws(sd, z, spk, mu, seed=seed, utt_ids=range(utt_base, utt_base + B), rows=rows, steps=steps, wav=wav)


def test_draw_by_draw_against_the_oracle():
    # rows: slots on XCDs 0, 7, 0 (second local slot), 2
    stats = _draws_against_the_oracle(19, 2, 400, "xcm/o?", seed=13, utt_base=11, rows=(0, 7, 16, 18))
    assert sum(e for _, e in stats) >= 0.999 * sum(n for n, _ in stats)


def test_more_utterances_than_slots_and_alone_equals_in_batch():
    """Continuous batching: 200 ragged utterances through 128 decode slots and through 24 (three per XCD); every utterance
    equals the same utterance decoded alone (its sampling stream does not depend on the placement)."""
    voc, _ = vocoder()
    n, Tc = 200, 3
    z, spk = H.inputs("xcm/c?", n, Tc)
    n_codes = H.ragged_sevens(n, Tc)
    ids = list(range(100, 100 + n))
    with H.options(voc, xcm=1) as set_option:
        res = {}
        for slots in (128, 24):
            set_option("xcm_slots", slots)
            res[slots] = H.decode(voc, z, spk, path=3, n_codes=n_codes, seed=5, utt_ids=ids)
        H.assert_same_bits(res[128], res[24])
        set_option("xcm", 0)
        for i in (0, 77, 199):
            w1, m1 = voc.generate(z[i:i + 1, :n_codes[i]], spk[i:i + 1], seed=5, utt_ids=[ids[i]], return_mulaw=True)
            L = H.FRAME * n_codes[i]
            assert torch.equal(m1[0].cpu(), res[128][1][i, :L]) and torch.equal(w1[0].cpu(), res[128][0][i, :L])
            assert not res[128][1][i, L:].any()


def test_path_by_utterances_in_flight():
    """The default choice: VALU per-XCD decoders up to 68 utterances in flight, the matrix-core ones from 69 to 511, launches above."""
    voc, _ = vocoder()
    for B, want in ((32, 2), (68, 2), (69, 3), (130, 3), (400, 3), (520, 0)):
        z = synth.randint(f"xcm/pz{B}", (B, 1), 512).cuda()
        spk = torch.zeros(B, dtype=torch.long, device="cuda")
        voc.generate(z, spk, seed=1, max_steps=8)
        voc.check()
        assert voc.last_path() == want, (B, voc.last_path())
    with H.options(voc, slots=100):              # 600 utterances through 100 decode slots: 100 in flight
        z = synth.randint("xcm/pz600", (600, 1), 512).cuda()
        voc.generate(z, torch.zeros(600, dtype=torch.long, device="cuda"), seed=1, max_steps=8)
        voc.check()
        assert voc.last_path() == 3


def test_configs3_single_gpu_form_properties():
    """configs[3] on one GPU: 256 x 32 000 through the 128 slots (two utterances per slot, back to back): finite, in range, and
    three rows equal the same utterances decoded alone."""
    voc, _ = vocoder()
    z = synth.randint("xcm/bz", (256, 100), 512).cuda()
    spk = (torch.arange(256, device="cuda") % 102)
    wav, mu = voc.generate(z, spk, seed=13, utt_base=0, return_mulaw=True)
    voc.check()
    assert voc.last_path() == 3
    assert wav.shape == (256, 32000) and torch.isfinite(wav).all() and wav.abs().max() <= 1.0
    assert mu.min() >= 0 and mu.max() <= 255 and mu.unique().numel() > 32
    ms, n = voc.last_timing()
    print("256 x 32000 through 128 slots on the matrix-core per-XCD decoders: %.2f us per sample step, %.2f M samples/s"
          % (ms * 1e3 / n, 256 * 32000 / ms / 1e3))
    for i in (0, 129, 255):
        w1, m1 = voc.generate(z[i:i + 1], spk[i:i + 1], seed=13, utt_base=i, return_mulaw=True)
        voc.check()
        assert torch.equal(m1[0], mu[i]) and torch.equal(w1[0], wav[i])


def test_handoff_timeout_is_reported_by_the_same_call_and_the_rerun_is_right():
    """One worker skips a candidate publish: every wait behind it gives up after the (shortened) deadline, check() raises for
    THAT call, the handle falls back to launches, and the repeated call gives the samples of the undisturbed paths."""
    voc, _ = vocoder(fresh=True)
    B = 80
    z = synth.randint("xcm/ez", (B, 2), 512).cuda()
    spk = synth.randint("xcm/es", (B,), 102).cuda()
    voc.set_option("xcm", 1)
    voc.set_option("xcd_timeout_ms", 20)
    voc.set_option("xcd_debug_drop_step", 200)
    wav, mu = voc.generate(z, spk, seed=9, utt_base=0, return_mulaw=True, async_=True)
    with pytest.raises(RuntimeError, match="timed out"):
        voc.check()
    assert not bool((mu[0, 260:] != 0).any())            # the call that suffered it is incomplete (and said so)
    voc.set_option("xcd_debug_drop_step", -1)
    wav2, mu2 = voc.generate(z, spk, seed=9, utt_base=0, return_mulaw=True)      # the handle has fallen back
    voc.check()
    assert voc.last_path() == 0
    want = H.reference_bits(z, spk, seed=9, utt_base=0)
    assert torch.equal(mu2.cpu(), want[1]) and torch.equal(wav2.cpu(), want[0])
    voc3, _ = vocoder(fresh=True)
    voc3.set_option("xcm", 1)
    voc3.set_option("xcd_timeout_ms", 20)
    voc3.set_option("xcd_debug_drop_step", 100)
    with pytest.warns(UserWarning, match="decode repeated"):
        wav3 = voc3.generate(z, spk, seed=9, utt_base=0)
    assert torch.equal(wav3.cpu(), want[0])


def test_128_x_32000_bit_equal_to_the_launch_path():
    """128 utterances of 2 s through the 128 matrix-core slots: the same 4 096 000 samples as the launch-per-step kernels (one
    run each)."""
    voc, _ = vocoder()
    z = synth.randint("xcm/fz128", (128, 100), 512).cuda()
    spk = (torch.arange(128, device="cuda") % 102)
    xcm, launch = _both_paths(voc, z, spk, seed=13, utt_base=0)
    H.assert_same_bits(xcm, launch)


def test_2400_consecutive_steps_draw_by_draw_against_the_oracle():
    """2 400 consecutive steps of two utterances inside a batch of 80 on the matrix-core decoders, every draw checked against
    the C oracle on the same history (a late-step divergence cannot hide behind 400-step windows)."""
    for b, (n, exact) in zip((0, 79), _draws_against_the_oracle(80, 8, 2400, "xcm/l?", seed=21, utt_base=5, rows=(0, 79))):
        assert n - exact <= 0.001 * n, (b, n - exact)
