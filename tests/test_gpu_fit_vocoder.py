"""-m gpu: ``driver.fit_vocoder`` and ``cli fit-vocoder`` -- a 30-step fit of a small vocoder (size_h_rnn 512) on six synthetic
utterances lowers the loss by at least half of what the same loop does with the float64 reference and torch's Adam on the CPU
(tests/voc_fit_ref.py, recorded in tests/golden/voc_grad_pins.npz), ``nll`` and ``generate`` then use the new weights, and the
command line runs end to end."""
import json
import re

import numpy as np
import pytest
import torch

import nll_ref
import voc_fit_ref as F
import voc_grad_ref as R
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import cli, driver, io, synth

pytestmark = pytest.mark.gpu


def models():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict())
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(wave_ar=V.ConfWaveAR(size_h_rnn=F.HR))))
    voc.load_state_dict(F.vocoder_state_dict())
    return enc.cuda().eval(), voc.cuda().eval()


def test_fit_follows_the_float64_reference():
    enc, voc = models()
    waves, speakers = F.waves(), F.speakers()
    before = driver.score_vocoder(enc, voc, waves, None, speakers)[1]
    old = {k: v.detach().clone() for k, v in voc.state_dict().items()}
    z, spk = synth.randint("voc_fit/z", (2, 3), 512).cuda(), torch.tensor([3, 50], device="cuda")
    _, mu_old = voc.generate(z, spk, seed=13, utt_ids=[0, 1], return_mulaw=True, max_steps=200)
    handle = voc._handle.value
    handles = set()
    orig = voc._ar_fwd

    def watched(*a, **kw):
        handles.add(voc._handle.value)
        return orig(*a, **kw)

    voc._ar_fwd = watched
    try:
        r = driver.fit_vocoder(enc, voc, waves, None, speakers, steps=F.STEPS, lr=F.LR, max_batch=F.MAX_BATCH, clip_codes=F.CLIP, seed=F.SEED)
    finally:
        del voc._ar_fwd
    ref = R.pins()["fit_ref_losses"]
    dec, dec_ref = F.decrease(r["losses"]), F.decrease(ref)
    print(f"\nfit_vocoder: loss {r['losses'][0]:.6f} -> mean of the last five {np.mean(r['losses'][-5:]):.6f} (decrease {dec:.4f}); "
          f"float64 on the CPU {ref[0]:.6f} -> {ref[-5:].mean():.6f} (decrease {dec_ref:.4f})")
    assert r["steps"] == F.STEPS == len(r["losses"]) and r["batches"] == 2 and r["utterances"] == F.N_WAVES
    assert handles == {handle}                                        # no new native handle between the steps
    assert dec >= 0.5 * dec_ref
    # only rnnms.ar moved
    for k, v in voc.state_dict().items():
        assert torch.equal(v, old[k]) != k.startswith("rnnms.ar."), k
    # nll and generate use the new weights: the bits of a vocoder made from the fitted state dict
    after = driver.score_vocoder(enc, voc, waves, None, speakers)[1]
    assert after["loss"] < before["loss"] and after["n_scored"] == before["n_scored"]
    fresh = V.Vocoder(voc.conf)
    fresh.load_state_dict(voc.state_dict())
    fresh = fresh.cuda().eval()
    assert driver.score_vocoder(enc, fresh, waves, None, speakers)[1]["nll_sum"] == after["nll_sum"]
    _, mu_new = voc.generate(z, spk, seed=13, utt_ids=[0, 1], return_mulaw=True, max_steps=200)
    _, mu_fresh = fresh.generate(z, spk, seed=13, utt_ids=[0, 1], return_mulaw=True, max_steps=200)
    assert torch.equal(mu_new, mu_fresh) and not torch.equal(mu_new, mu_old)


def test_cli_fit_vocoder_end_to_end(tmp_path, capsys):
    root, wavs = tmp_path / "datasets" / "tiny", tmp_path / "wavs"
    root.mkdir(parents=True)
    wavs.mkdir()
    stems = ["S01_a", "S02_b", "S01_c"]
    for stem, w in zip(stems, nll_ref.waves(3, seed="voc_fit/cli")):
        io.save_wav(wavs / (stem + ".wav"), torch.from_numpy(w), 16000)
    (root / "speakers.json").write_text(json.dumps(["S02", "S01"]))
    (root / "test.json").write_text(json.dumps([["x", 0, 1, "tiny/" + stem] for stem in stems]))
    out = tmp_path / "vocoder.pt"
    assert cli.main(["fit-vocoder", "--dataset", str(root), "--in-dir", str(wavs), "--random-init", "--steps", "6", "--lr", "1e-3",
                     "--clip-codes", "1", "--out", str(out)]) == 0
    text = capsys.readouterr().out
    with capsys.disabled():
        print(text)
    losses = [float(v) for v in re.findall(r"vocoder loss:([0-9.]+) nats/sample", text)]
    assert len(losses) == 2 and losses[1] < losses[0] and "before the fit" in text and "after the fit" in text
    assert re.search(r"fitted rnnms.ar .* in 6 steps of Adam", text)
    sd = io.load_vocoder_checkpoint(out, expected=V.Vocoder(V.ConfVocoder()).state_dict())
    init = synth.vocoder_state_dict()
    assert list(sd) == list(init)
    for k, v in init.items():
        assert torch.equal(sd[k], v) != k.startswith("rnnms.ar."), k
    assert cli.main(["score-vocoder", "--dataset", str(root), "--in-dir", str(wavs), "--cpc-checkpoint", str(_enc_ckpt(tmp_path)),
                     "--vocoder-checkpoint", str(out)]) == 0         # score-vocoder reads the fitted checkpoint
    again = [float(v) for v in re.findall(r"vocoder loss:([0-9.]+) nats/sample", capsys.readouterr().out)]
    assert again == losses[1:]


def _enc_ckpt(tmp_path):
    p = tmp_path / "enc.pt"
    torch.save({"encoder": synth.encoder_state_dict()}, p)
    return p
