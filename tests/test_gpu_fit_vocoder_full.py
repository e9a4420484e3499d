"""-m gpu: ``driver.fit_vocoder`` with the conditioning parts named, at the shape of tests/test_gpu_fit_vocoder.py (a small vocoder,
size_h_rnn 512, six synthetic utterances): one fit of all three parts, and one of ``("embeddings", "prenet")`` alone -- the
sample-rate network frozen, so that any fall in the loss comes from the gradients of ``csrc/prenet_grad.hip`` only.  Each must
lower the loss, first step to the mean of the last five, by at least half of what the same loop does with the float64 reference and
torch's Adam on the CPU (tests/cond_grad_ref.py ``fit_reference_losses``, recorded in tests/golden/cond_grad_pins.npz, where the
generator also held each recorded decrease to several times the spread of its own last five steps)."""
import numpy as np
import pytest
import torch

import cond_grad_ref as R
import voc_fit_ref as F
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import driver, synth

pytestmark = pytest.mark.gpu


def models():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict())
    voc = V.Vocoder(V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(wave_ar=V.ConfWaveAR(size_h_rnn=F.HR))))
    voc.load_state_dict(F.vocoder_state_dict())
    return enc.cuda().eval(), voc.cuda().eval()


@pytest.mark.parametrize("run", list(R.FIT_RUNS))
def test_fit_follows_the_float64_reference(run):
    train, steps, lr = R.FIT_RUNS[run]
    enc, voc = models()
    waves, speakers = F.waves(), F.speakers()
    before = driver.score_vocoder(enc, voc, waves, None, speakers)[1]
    old = {k: v.detach().clone() for k, v in voc.state_dict().items()}
    handle = voc._handle.value
    handles = set()
    orig = voc._cond_fwd

    def watched(*a, **kw):
        handles.add(voc._handle.value)
        return orig(*a, **kw)

    voc._cond_fwd = watched
    try:
        r = driver.fit_vocoder(enc, voc, waves, None, speakers, steps=steps, lr=lr, max_batch=F.MAX_BATCH, clip_codes=F.CLIP, seed=F.SEED,
                               train=train)
    finally:
        del voc._cond_fwd
    ref = R.pins()[f"fit_{run}_losses"]
    dec, dec_ref = F.decrease(r["losses"]), F.decrease(ref)
    print(f"\nfit_vocoder train={train}: loss {r['losses'][0]:.6f} -> mean of the last five {np.mean(r['losses'][-5:]):.6f} (decrease "
          f"{dec:.4f}); float64 on the CPU {ref[0]:.6f} -> {ref[-5:].mean():.6f} (decrease {dec_ref:.4f})")
    assert r["steps"] == steps == len(r["losses"]) and r["batches"] == 2 and r["utterances"] == F.N_WAVES
    assert handles == {handle}                                        # no new native handle between the steps
    assert dec >= 0.5 * dec_ref
    # exactly the named parts moved
    part_of = lambda k: "ar" if k.startswith("rnnms.ar.") else "prenet" if k.startswith("rnnms.prenet.") else "embeddings"
    for k, v in voc.state_dict().items():
        assert torch.equal(v, old[k]) != (part_of(k) in train), k
    # nll uses the new weights: the bits of a vocoder made from the fitted state dict
    after = driver.score_vocoder(enc, voc, waves, None, speakers)[1]
    assert after["loss"] < before["loss"] and after["n_scored"] == before["n_scored"]
    fresh = V.Vocoder(voc.conf)
    fresh.load_state_dict(voc.state_dict())
    fresh = fresh.cuda().eval()
    assert driver.score_vocoder(enc, fresh, waves, None, speakers)[1]["nll_sum"] == after["nll_sum"]


def test_frozen_parts_and_error_paths():
    enc, voc = models()
    waves, speakers = F.waves()[:2], F.speakers()[:2]
    with pytest.raises(ValueError, match="train must name each of"):
        driver.fit_vocoder(enc, voc, waves, None, speakers, steps=1, train=("ar", "prenet", "prenet"))
    with pytest.raises(ValueError, match="train must name each of"):
        driver.fit_vocoder(enc, voc, waves, None, speakers, steps=1, train=("mel",))
    for p in voc._part_params("embeddings"):
        p.requires_grad_(False)
    with pytest.raises(ValueError, match="requires a gradient"):
        driver.fit_vocoder(enc, voc, waves, None, speakers, steps=1, clip_codes=1, train=("embeddings",))
    # a table that requires no gradient is not asked for and does not move, the prenet beside it does
    old = {k: v.detach().clone() for k, v in voc.state_dict().items()}
    r = driver.fit_vocoder(enc, voc, waves, None, speakers, steps=2, clip_codes=1, train=("embeddings", "prenet"))
    assert r["steps"] == 2
    for k, v in voc.state_dict().items():
        assert torch.equal(v, old[k]) != k.startswith("rnnms.prenet."), k
