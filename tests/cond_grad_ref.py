"""Shared by the conditioning-gradient tests (plain module, not a conftest): the cases and the float64 reference of
``vqcpc_vocoder_cond_fwd`` / ``_bwd`` (``csrc/prenet_grad.hip``), of the whole-vocoder chain behind ``Vocoder.vocoder_gradients`` and of
``driver.fit_vocoder`` with the conditioning parts named.

Reference: torch's own modules in float64 -- two ``nn.Embedding``, ``repeat_interleave(2)`` over time, ``torch.cat`` and
``nn.GRU(num_layers=2, bidirectional=True, batch_first=True)`` loaded from the state dict -- run PER UTTERANCE on its own
``2 n_codes[b]`` frames, so that a ragged batch is by construction its utterances one at a time.  The eighteen tensors are leaves.
Loss = ``sum(cond * G)`` over the utterances' frames for a seeded upstream ``G``.  It runs once in float64 and once in fp32 on the
CPU; tests/golden/cond_grad_pins.npz (``tools/gen_cond_grad_golden.py``) pins the float64 run and holds ``e_ref``, the fp32 run's
distance from it, per tensor.  tests/test_cond_grad_cpu.py holds its forward to ``oracle.f64_ref.F64Vocoder.condition``.

Chain: the end-to-end loss is ``voc_grad_ref.loss_of`` -- the float64 sample loop of the vocoder-gradient tests -- fed by this module's
differentiable conditioning, on three cases of tests/voc_grad_ref.py; all 27 tensors are leaves.

Pins and judge, per tensor: tests/grad_judge.py.
"""
import os

import numpy as np
import torch
import torch.nn as nn

import grad_judge
import voc_grad_ref as VR
from oracle import f64_ref
from vectorquantizedcpc_amd import synth

# Vocoder.COND_KEYS: the two tables, then w_ih, w_hh, b_ih, b_hh, each [layer][direction]
KEYS = ("code_embedding.weight", "speaker_embedding.weight") + tuple(
    f"rnnms.prenet.{k}_l{layer}{suf}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for layer in range(2) for suf in ("", "_reverse"))
AR_NAMES = tuple("rnnms.ar." + n for n in VR.SD_NAMES)
ALL27 = KEYS + AR_NAMES
PINS = os.path.join(grad_judge.GOLD, "cond_grad_pins.npz")
POSITIONS = "cond_grad/{name}/{tensor}/pins"
N_CODES, N_SPK = 512, 102

# name -> sizes (dz, ds, C = dim_voc_latent), batch (B, Tc), code counts (None = all), weight set, indices ("random" or one code for
# every position), speakers (None = seeded), upstream ("dense", or (b, frame): non-zero in that frame of that utterance alone)
_D = dict(dz=64, ds=64, C=256, n_codes=None, weights="default", idx="random", spk=None, upstream="dense")
CASES = {
    "ref_sizes": dict(_D, B=2, Tc=16),
    # distinct code counts, and one utterance with no code at all: the smallest count the scoring entry accepts
    "ragged": dict(_D, B=6, Tc=6, n_codes=[2, 5, 3, 4, 6, 0]),
    "b1": dict(_D, B=1, Tc=4),
    "b17": dict(_D, B=17, Tc=3),                                     # a second 16-column batch tile with one column
    "hp64": dict(_D, C=128, B=3, Tc=5),
    "hp256": dict(_D, C=512, B=3, Tc=5),
    "dz_ne_ds": dict(_D, dz=96, ds=32, B=3, Tc=5),
    "stressed": dict(_D, B=2, Tc=8, weights="stressed"),             # saturated gates
    "one_code": dict(_D, B=3, Tc=5, idx=77, spk=[7, 30, 7], n_codes=[5, 4, 3]),
    "sparse_upstream": dict(_D, B=3, Tc=5, upstream=(1, 6), n_codes=[5, 4, 5]),
    # 2 300 rows: three slabs of 1024, the last ragged; 1 400 steps
    "long": dict(_D, B=2, Tc=700, n_codes=[700, 450]),
}
ALL_CASES = list(CASES)
CHAIN_CASES = ("ragged", "chunks", "h512")                           # of tests/voc_grad_ref.py

_cases, _refs, _chain = {}, {}, {}


def state_dict(c):
    sd = synth.vocoder_state_dict(dim_i_embedding=c["dz"], dim_speaker_embedding=c["ds"], dim_voc_latent=c["C"], size_h_rnn=512)
    return f64_ref.stressed(sd) if c["weights"] == "stressed" else sd


def load(name):
    """A case as a dict: its sizes, ``sd`` (fp32 state dict), ``z`` (B, Tc), ``spk`` (B) int64, ``n_codes`` as a list, ``G``
    (B, 2 Tc, C) fp32 with zero rows past an utterance's frames.  Computed once and shared (treat as read-only)."""
    if name not in _cases:
        c = dict(CASES[name], name=name)
        B, Tc = c["B"], c["Tc"]
        c["sd"] = state_dict(c)
        c["z"] = (synth.randint(f"cond_grad/{name}/z", (B, Tc), N_CODES) if c["idx"] == "random"
                  else torch.full((B, Tc), int(c["idx"]), dtype=torch.int64))
        c["spk"] = synth.randint(f"cond_grad/{name}/s", (B,), N_SPK) if c["spk"] is None else torch.tensor(c["spk"], dtype=torch.int64)
        c["n_codes"] = [Tc] * B if c["n_codes"] is None else list(c["n_codes"])
        G = grad_judge.uniform(f"cond_grad/{name}/G", (B, 2 * Tc, c["C"]), 1.0)
        if c["upstream"] != "dense":
            b, f = c["upstream"]
            keep = torch.zeros_like(G)
            keep[b, f] = G[b, f]
            G = keep
        for b, n in enumerate(c["n_codes"]):
            G[b, 2 * n:] = 0.0
        c["G"] = G
        _cases[name] = c
    return _cases[name]


class Conditioning(nn.Module):
    """The conditioning path as torch's own modules, loaded from a vocoder state dict, in ``dtype``."""

    def __init__(self, sd, dtype=torch.float64):
        super().__init__()
        n_codes, dz = sd["code_embedding.weight"].shape
        n_spk, ds = sd["speaker_embedding.weight"].shape
        Hp = sd["rnnms.prenet.weight_hh_l0"].shape[1]
        self.code_embedding, self.speaker_embedding = nn.Embedding(n_codes, dz), nn.Embedding(n_spk, ds)
        self.rnnms = nn.Module()
        self.rnnms.prenet = nn.GRU(dz + ds, Hp, num_layers=2, batch_first=True, bidirectional=True)
        self.load_state_dict({k: sd[k] for k in KEYS})
        self.to(dtype)

    def forward(self, z, spk, n_codes):
        """A list of (2 n_codes[b], C) tensors: every utterance alone on its own frames."""
        out = []
        for b, n in enumerate(n_codes):
            if n == 0:
                out.append(torch.zeros(0, 2 * self.rnnms.prenet.hidden_size, dtype=self.code_embedding.weight.dtype))
                continue
            ze = self.code_embedding(z[b, :n]).repeat_interleave(2, dim=0)
            x = torch.cat((ze, self.speaker_embedding(spk[b])[None, :].expand(2 * n, -1)), dim=1)
            out.append(self.rnnms.prenet(x[None])[0][0])
        return out

    def grads(self):
        p = dict(self.named_parameters())
        return {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in KEYS}


def _np(d):
    return {k: v.detach().numpy().astype(np.float64) for k, v in d.items()}


def grads(name, dtype=torch.float64):
    """The reference in ``dtype`` on the CPU: dict over ``KEYS`` plus ``cond`` (B, 2 Tc, C), numpy float64."""
    c = load(name)
    m = Conditioning(c["sd"], dtype)
    cond = m(c["z"], c["spk"], c["n_codes"])
    G = c["G"].to(dtype)
    loss = sum((x * G[b, :x.shape[0]]).sum() for b, x in enumerate(cond))
    if loss.requires_grad:
        loss.backward()
    dense = torch.zeros(c["B"], 2 * c["Tc"], c["C"], dtype=dtype)
    for b, x in enumerate(cond):
        dense[b, :x.shape[0]] = x.detach()
    return _np(dict(m.grads(), cond=dense))


def grads64(name):
    if name not in _refs:
        _refs[name] = grads(name)
    return _refs[name]


def chain_grads(name, dtype=torch.float64):
    """The end-to-end reference of case ``name`` of tests/voc_grad_ref.py in ``dtype``: the gradients of its mean NLL with respect to
    all 27 tensors (dict over ``ALL27``) plus ``loss``, numpy float64."""
    c = VR.load(name)
    m = Conditioning(c["sd"], dtype)
    p = {k: v.clone().requires_grad_(True) for k, v in VR.weights(c, dtype).items()}
    loss = VR.loss_of(p, m(c["z"], c["spk"], c["n_codes"]), c["audio"], c["slen"], c["up"])
    (loss * (1.0 if c["grad_loss"] is None else c["grad_loss"])).backward()
    out = m.grads()
    out.update({n: p[k].grad for k, n in zip(VR.KEYS, AR_NAMES)})
    out["loss"] = loss.detach()
    return _np(out)


def chain64(name):
    if name not in _chain:
        _chain[name] = chain_grads(name)
    return _chain[name]


def pins():
    return grad_judge.load_pins(PINS)


def judge(name, got, what):
    grad_judge.judge(grads64(name), pins(), name, got, what, KEYS)


def judge_chain(name, got, what):
    grad_judge.judge(chain64(name), pins(), "chain_" + name, got, what, ALL27)


# ------------------------------------------------------------------ the fit with the conditioning parts
FIT_RUNS = {"full": (("embeddings", "prenet", "ar"), 30, 1e-3), "cond": (("embeddings", "prenet"), 30, 1e-3)}       # train, steps, lr


def fit_reference_losses(train, steps, lr):
    """tests/voc_fit_ref.py's loop -- same utterances, codes, cuts and buckets -- with the conditioning differentiable: the parts
    ``train`` names step under one torch Adam in float64 on the CPU.  -> per-step losses."""
    import oracle
    import voc_fit_ref as F
    from oracle import mel_fp32
    from vectorquantizedcpc_amd import driver
    ws, spk, esd, sd = F.waves(), F.speakers(), synth.encoder_state_dict(), F.vocoder_state_dict()
    idx = [torch.from_numpy(np.asarray(oracle.encoder_encode(esd, mel_fp32.wave_to_mel(w)[None])["indices"][0])) for w in ws]
    audio = [torch.from_numpy(driver.mulaw_classes(w)) for w in ws]
    n_codes = [int(i.numel()) for i in idx]
    keep = [driver.scored_samples(a.numel(), nc, F.UP) for a, nc in zip(audio, n_codes)]
    idx, audio, n_codes, keep = driver.training_cuts(idx, audio, n_codes, keep, F.UP, F.CLIP, F.SEED)
    batches = []
    for ids in driver.make_buckets(keep, [0] * len(keep), F.MAX_BATCH, 0.25):
        z = driver._pad_batch([idx[i] for i in ids], "cpu", torch.int64, min_len=1)
        a = driver._pad_batch([audio[i] for i in ids], "cpu", torch.int64, min_len=1)
        batches.append((a, z, torch.tensor([spk[i] for i in ids]), [n_codes[i] for i in ids], [keep[i] - 1 for i in ids]))
    m = Conditioning(sd)
    p = {k: sd["rnnms.ar." + n].detach().double().clone().requires_grad_(True) for k, n in zip(VR.KEYS, VR.SD_NAMES)}
    named = dict(m.named_parameters())
    parts = {"ar": list(p.values()), "embeddings": [named[k] for k in KEYS[:2]], "prenet": [named[k] for k in KEYS[2:]]}
    opt = torch.optim.Adam([q for part in ("ar", "prenet", "embeddings") if part in train for q in parts[part]], lr=lr)
    losses = []
    for step in range(steps):
        a, z, s, ncs, slen = batches[step % len(batches)]
        opt.zero_grad(set_to_none=True)
        loss = VR.loss_of(p, m(z, s, ncs), a, slen, F.UP)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return np.asarray(losses, np.float64)
