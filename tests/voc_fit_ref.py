"""Shared by the ``fit_vocoder`` tests (plain module, not a conftest): the small fit the GPU test runs, and the same loop on the CPU
with the float64 reference of tests/voc_grad_ref.py and torch's Adam -- the codes from the CPU oracle's encoder on the float32
emulation of the mel front end, the cuts and the buckets from the driver's own host functions.  ``tools/gen_voc_grad_golden.py``
records its per-step losses as ``fit_ref_losses`` in tests/golden/voc_grad_pins.npz.

The GPU fit must lower the loss, first step to the mean of the last five, by at least HALF of what this loop does: Adam's first
steps are nearly sign steps, so small gradient differences between fp32 and float64 (and a code the two front ends may place
differently) move the path but not the trend.
"""
import numpy as np
import torch

import nll_ref
import voc_grad_ref as R
from vectorquantizedcpc_amd import driver, synth

HR, N_WAVES, STEPS, LR, CLIP, MAX_BATCH, SEED, UP = 512, 6, 30, 1e-3, 2, 3, 13, 160


def waves():
    return nll_ref.waves(N_WAVES)


def speakers():
    return [(7 * i + 3) % 102 for i in range(N_WAVES)]


def vocoder_state_dict():
    return synth.vocoder_state_dict(size_h_rnn=HR)


def decrease(losses):
    """First step to the mean of the last five."""
    losses = np.asarray(losses, np.float64)
    return float(losses[0] - losses[-5:].mean())


def reference_losses():
    """The per-step losses of the float64 loop (about a minute on the CPU: the generator runs it, the tests read the pins)."""
    import oracle
    from oracle import f64_ref, mel_fp32
    ws, spk, esd, sd = waves(), speakers(), synth.encoder_state_dict(), vocoder_state_dict()
    idx = [torch.from_numpy(np.asarray(oracle.encoder_encode(esd, mel_fp32.wave_to_mel(w)[None])["indices"][0])) for w in ws]
    audio = [torch.from_numpy(driver.mulaw_classes(w)) for w in ws]
    n_codes = [int(i.numel()) for i in idx]
    keep = [driver.scored_samples(a.numel(), nc, UP) for a, nc in zip(audio, n_codes)]
    idx, audio, n_codes, keep = driver.training_cuts(idx, audio, n_codes, keep, UP, CLIP, SEED)
    model = f64_ref.F64Vocoder(sd, upsample=UP)
    batches = []
    for ids in driver.make_buckets(keep, [0] * len(keep), MAX_BATCH, 0.25):
        z = driver._pad_batch([idx[i] for i in ids], "cpu", torch.int64, min_len=1)
        a = driver._pad_batch([audio[i] for i in ids], "cpu", torch.int64, min_len=1)
        cond = model.condition(z, torch.tensor([spk[i] for i in ids]), [n_codes[i] for i in ids])     # the prenet is frozen
        batches.append((a, cond, [keep[i] - 1 for i in ids]))
    p = {k: sd["rnnms.ar." + n].detach().double().clone().requires_grad_(True) for k, n in zip(R.KEYS, R.SD_NAMES)}
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    losses = []
    for step in range(STEPS):
        a, cond, slen = batches[step % len(batches)]
        opt.zero_grad(set_to_none=True)
        loss = R.loss_of(p, cond, a, slen, UP)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.asarray(losses, np.float64)
