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

``WIDE_CASES``: ten more cases (tests/test_gpu_cond_grad_wide.py) on the paths the eleven leave out -- Hp = 512, row counts on and two
past a slab edge, nine batch tiles, a tile without a frame, tables that are no multiple of a tile and widths that are no multiple
of 16, and the two ends of an 80-frame BPTT chain with one code row per position -- and ``CHAIN_WIDE``, two wide cases of
tests/voc_grad_ref.py for the chain; pinned in tests/golden/cond_grad_wide_pins.npz.  The two table gradients also have row pins for
``grad_judge.judge_rows``: ``e_ref`` per row is the larger of two fp32 CPU yardsticks that sum in different orders, ``nn.GRU`` and
``Conditioning(..., manual=True)``, a Python loop over the frames with ``f64_ref._gru_update`` that is held to ``nn.GRU`` within
1e-12 in float64 and carries the seeded fault ``("cut", n)``.
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
N_CODES, N_SPK = 512, 102                                           # the tables' rows unless a case says otherwise ("K", "n_spk")

# name -> sizes (dz, ds, C = dim_voc_latent), batch (B, Tc), code counts (None = all), weight set, indices ("random" or one code for
# every position), speakers (None = seeded), upstream ("dense", or (b, frame): non-zero in that frame of that utterance alone)
_D = dict(dz=64, ds=64, C=256, n_codes=None, weights="default", idx="random", spk=None, upstream="dense", K=N_CODES, n_spk=N_SPK, z_set=None)
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

# Past the eleven.  R = 2 sum(n_codes) rows; GRAD_SLAB = 1024 rows; a batch tile is 16 utterances; a table tile is 64 rows by 16
# columns.  K, n_spk: the tables' rows.  z_set: {(b, t): code} or "tail" -- z[1] = 100 + arange(40), one code row per position, and
# every other utterance's codes outside 100 .. 139.
_TAIL = dict(_D, B=3, Tc=40, n_codes=[40, 40, 17], z_set="tail")
WIDE_CASES = {
    "hp512": dict(_D, C=1024, B=17, Tc=4, n_codes=[1 + b % 4 for b in range(17)]),          # pre_bwd_step_kernel<24>, two tiles
    "slab_exact": dict(_D, C=128, B=16, Tc=32),                                             # R = 1024
    "slab_plus_two": dict(_D, C=128, B=19, Tc=27),                                          # R = 1026: the second slab holds two rows
    # nine tiles, two live columns in the last; every fifth utterance has no frame, the first of the batch included
    "b130": dict(_D, C=128, B=130, Tc=4, n_codes=[(3 * b) % 5 for b in range(130)]),
    "dead_tile": dict(_D, C=128, B=40, Tc=3, n_codes=[0 if 16 <= b < 32 else 3 for b in range(40)]),
    # F = 32; Nk = 100 and Nk = 1 against tiles of 64 rows; the last code row is named
    "tables_small": dict(_D, dz=16, ds=16, C=128, K=100, n_spk=1, B=3, Tc=5, z_set={(0, 0): 99}),
    # the code table's last column tile has 8 live columns; the speaker table starts at column 40
    "dz40_ds24": dict(_D, dz=40, ds=24, K=1024, n_spk=7, B=3, Tc=5, z_set={(0, 0): 1023}),
    "tail": dict(_TAIL, upstream=(1, 79)),                           # the forward directions' BPTT chain over 80 frames
    "head": dict(_TAIL, upstream=(1, 0)),                            # the reverse directions' chain
    "tail_stressed": dict(_TAIL, upstream=(1, 79), weights="stressed"),
}
ALL_WIDE = list(WIDE_CASES)
CHAIN_WIDE = ("straddle", "slab_plus_two")                           # of tests/voc_grad_ref.py; the second runs Hp = 512 inside the chain
WIDE_PINS = os.path.join(grad_judge.GOLD, "cond_grad_wide_pins.npz")
ROW_TENSORS = KEYS[:2]                                               # the two tables: judged per row as well

_cases, _refs, _chain = {}, {}, {}


def state_dict(c):
    sd = synth.vocoder_state_dict(size_i_codebook=c["K"], n_speakers=c["n_spk"], dim_i_embedding=c["dz"], dim_speaker_embedding=c["ds"],
                                  dim_voc_latent=c["C"], size_h_rnn=512)
    return f64_ref.stressed(sd) if c["weights"] == "stressed" else sd


def load(name):
    """A case as a dict: its sizes, ``sd`` (fp32 state dict), ``z`` (B, Tc), ``spk`` (B) int64, ``n_codes`` as a list, ``G``
    (B, 2 Tc, C) fp32 with zero rows past an utterance's frames.  Computed once and shared (treat as read-only)."""
    if name not in _cases:
        c = dict(CASES[name] if name in CASES else WIDE_CASES[name], name=name)
        B, Tc = c["B"], c["Tc"]
        c["sd"] = state_dict(c)
        c["z"] = (synth.randint(f"cond_grad/{name}/z", (B, Tc), c["K"]) if c["idx"] == "random"
                  else torch.full((B, Tc), int(c["idx"]), dtype=torch.int64))
        if c["z_set"] == "tail":
            z = c["z"].clone()
            z[(z >= 100) & (z < 100 + Tc)] += Tc                     # the other utterances name no code of 100 .. 100 + Tc - 1
            z[1] = 100 + torch.arange(Tc)
            c["z"] = z
        elif c["z_set"]:
            c["z"] = c["z"].clone()
            for (b, t), k in c["z_set"].items():
                c["z"][b, t] = k
        c["spk"] = synth.randint(f"cond_grad/{name}/s", (B,), c["n_spk"]) if c["spk"] is None else torch.tensor(c["spk"], dtype=torch.int64)
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
    """The conditioning path as torch's own modules, loaded from a vocoder state dict, in ``dtype``.

    ``manual=True``: a second statement of the bi-GRU on the same parameters -- per layer and direction ``gi = x W_ih^T + b_ih`` for
    all frames, then a Python loop over the frames with ``f64_ref._gru_update(gi[t], W_hh h + b_hh, h)``, the reverse direction
    from the last frame down.  In float64 it equals ``nn.GRU`` within 1e-12; in fp32 it sums in another order.  ``fault=("cut", n)``
    (manual only) detaches ``h`` in both layers and both directions at every frame more than ``n`` frames from frame 79: the chain
    of the back-propagation through time is dropped ``n`` frames from there, the forward keeps its value."""

    def __init__(self, sd, dtype=torch.float64, manual=False, fault=None):
        super().__init__()
        assert fault is None or (manual and fault[0] == "cut")
        self.manual, self.fault = manual, fault
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
            out.append(self._bigru(x) if self.manual else self.rnnms.prenet(x[None])[0][0])
        return out

    def _bigru(self, x):
        """The two bidirectional layers over one utterance's frames ``x`` (T, I), frame by frame."""
        g = self.rnnms.prenet
        T = x.shape[0]
        for layer in range(2):
            halves = []
            for suf in ("", "_reverse"):
                w_ih, w_hh, b_ih, b_hh = (getattr(g, f"{k}_l{layer}{suf}") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                gi = x @ w_ih.T + b_ih
                h = torch.zeros(g.hidden_size, dtype=x.dtype)
                hs = [None] * T
                for t in (range(T) if suf == "" else range(T - 1, -1, -1)):
                    h = f64_ref._gru_update(gi[t], w_hh @ h + b_hh, h)
                    if self.fault is not None and abs(t - 79) > self.fault[1]:
                        h = h.detach()
                    hs[t] = h
                halves.append(torch.stack(hs))
            x = torch.cat(halves, dim=1)
        return x

    def grads(self):
        p = dict(self.named_parameters())
        return {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in KEYS}


def _np(d):
    return {k: v.detach().numpy().astype(np.float64) for k, v in d.items()}


def grads(name, dtype=torch.float64, manual=False, fault=None):
    """The reference in ``dtype`` on the CPU: dict over ``KEYS`` plus ``cond`` (B, 2 Tc, C), numpy float64.  ``manual``, ``fault``:
    ``Conditioning``'s."""
    c = load(name)
    m = Conditioning(c["sd"], dtype, manual, fault)
    with grad_judge.one_thread():
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
    with grad_judge.one_thread():
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
    return grad_judge.load_pins(PINS, WIDE_PINS)


def judge(name, got, what):
    grad_judge.judge(grads64(name), pins(), name, got, what, KEYS)


def judge_rows(name, got, what):
    """The two table gradients of a wide case per code and per speaker (``grad_judge.judge_rows``)."""
    return grad_judge.judge_rows(grads64(name), pins(), name, got, what, ROW_TENSORS)


def named_rows(c):
    """(codes, speakers) whose rows of the table gradients are not zero: those the frames with a path to the upstream name."""
    live = [c["upstream"][0]] if c["upstream"] != "dense" else [b for b, n in enumerate(c["n_codes"]) if n]
    return (sorted({int(k) for b in live for k in c["z"][b, :c["n_codes"][b]]}), sorted({int(c["spk"][b]) for b in live}))


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
