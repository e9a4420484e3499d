"""Shared by the vocoder-gradient tests (plain module, not a conftest): the cases and the float64 reference of
``vqcpc_vocoder_ar_fwd`` / ``_bwd`` (``csrc/vocoder_grad.hip``).

Reference: the statements of ``oracle/f64_ref.py`` for the sample loop -- the tabled input half of the gates (``emb @ W_ih[:, :de]^T``
per class, ``cond @ W_ih[:, de:]^T + b_ih`` per frame), ``_gru_update`` (imported from there), fc1, ReLU, fc2, ``log_softmax``, gather
of ``audio[:, 1:]``, mean over every scored sample of the batch -- written with differentiable torch operations.  The nine tensors of
``rnnms.ar`` and ``cond`` are leaves; ``cond`` comes from ``F64Vocoder.condition`` of the matching dtype, as a constant.  It runs once in
float64 and once in fp32 on the CPU; tests/golden/voc_grad_pins.npz (``tools/gen_voc_grad_golden.py``) pins the float64 run and holds
``e_ref``, the fp32 run's distance from it, per tensor.  tests/test_voc_grad_cpu.py holds the float64 run to ``nn.Embedding`` +
``nn.GRU`` + ``nn.Linear`` + ``F.cross_entropy`` built from the same state dict.

Pins and judge, per tensor (the nine gradients and ``grad_cond``): tests/grad_judge.py.

``WIDE_CASES``: eight more cases (tests/test_gpu_voc_grad_wide.py) on the paths the twelve leave out -- frames cut by a chunk edge,
row counts on and two past a slab edge, utterances ending on, one past and one short of each chunk edge, a batch tile that scores
nothing, a call of one step, saturated gates across chunk edges; pinned in tests/golden/voc_grad_wide_pins.npz, where ``embedding``
(per class) and ``grad_cond`` (per utterance and frame) also have row pins for ``grad_judge.judge_rows``.  ``loss_of(..., fault=)``
seeds the two errors those paths invite, by autograd alone; tests/test_voc_grad_cpu.py shows that both judges catch them.
"""
import os

import numpy as np
import torch

import grad_judge
from oracle import f64_ref
from vectorquantizedcpc_amd import synth

KEYS = ("embedding", "w_ih", "w_hh", "b_ih", "b_hh", "fc1_weight", "fc1_bias", "fc2_weight", "fc2_bias")     # Vocoder.AR_KEYS
SD_NAMES = ("embedding.weight", "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0", "fc1.weight", "fc1.bias",
            "fc2.weight", "fc2.bias")
TENSORS = KEYS + ("grad_cond",)
PINS = os.path.join(grad_judge.GOLD, "voc_grad_pins.npz")
POSITIONS = "voc_grad/{name}/{tensor}/pins"

# name -> sizes (Hr, de, C = dim_voc_latent, up = upsampling_t), batch (B, Tc, L), per-utterance lengths and code counts (None = all),
# handle options, weight set, what the audio is ("random" or a class), upstream gradient.  Steps = max(lengths) - 1.
_D = dict(Hr=512, de=256, C=256, up=8, lengths=None, n_codes=None, options={}, weights="default", audio="random", grad_loss=None)
CASES = {
    # the reference's sizes: two frames of 160, five 64-step tiles of the head
    "ref_sizes": dict(_D, Hr=896, up=160, B=2, Tc=1, L=321),
    # ragged: row 0 scores nothing, row 1 ends exactly where its codes end, row 2 is cut in mid-frame, rows 3 and 4 in mid-tile (59
    # and 77 steps: no multiple of 64); distinct code counts
    "ragged": dict(_D, B=5, Tc=6, L=97, lengths=[1, 81, 30, 60, 78], n_codes=[2, 5, 3, 4, 6]),
    # three chunks of 160 steps, the last one partial (80 steps), utterance 1 ends inside the middle chunk, utterance 2 on its edge
    "chunks": dict(_D, B=3, Tc=25, L=401, lengths=[401, 251, 161], n_codes=[25, 16, 11], options={"tf_chunk_replays": 1}),
    "b1": dict(_D, B=1, Tc=5, L=81),
    "b17": dict(_D, B=17, Tc=3, L=49),                                              # a second 16-row tile with one row
    "b32_big": dict(_D, Hr=896, B=32, Tc=4, L=65, options={"big_min_tiles": 2}),    # ar_gru_big_kernel runs the forward
    "h512": dict(_D, Hr=512, de=32, C=128, B=3, Tc=5, L=81),
    "h1024": dict(_D, Hr=1024, de=32, C=128, B=3, Tc=5, L=81),
    "stressed": dict(_D, Hr=896, B=2, Tc=8, L=129, weights="stressed"),
    "const_audio": dict(_D, B=2, Tc=5, L=81, audio=77),                             # every other row of d embedding is +0
    "upstream": dict(_D, B=2, Tc=5, L=70, lengths=[70, 41], grad_loss=-2.75),
    # about 1 300 steps at the reference's sizes: three chunks of the default 640
    "long": dict(_D, Hr=896, up=160, B=2, Tc=5, L=1301, lengths=[1301, 900]),
}
ALL_CASES = list(CASES)
MODULE_CASES = ("ref_sizes", "b17")          # equal lengths: F.cross_entropy's own mean applies


def _chunk(ch):
    return {"steps_per_graph": ch, "tf_chunk_replays": 1}            # CH = their product: even, at least 2


# Past the twelve.  CH: the chunk, in steps; M = B CH rows per chunk; GRAD_SLAB = 1024 rows; a batch tile is 16 utterances.
WIDE_CASES = {
    # seven chunks of 16 steps, the last with 12; frames of 6 steps: the edges at 16, 32, 64 and 80 cut frames 2, 5, 10 and 13 (48 and
    # 96 fall between two frames); two batch tiles; de = 96
    "straddle": dict(_D, up=6, B=19, Tc=9, L=109, lengths=[109 - 5 * (b % 7) for b in range(19)], de=96, C=128, options=_chunk(16)),
    # a frame of 40 steps spans two and a half chunks; chunks wholly inside one frame
    "frame_over_chunks": dict(_D, up=40, B=3, Tc=2, L=150, lengths=[150, 97, 41], options=_chunk(16)),
    # utterances of 16, 17, 15, 32, 33, 31 and 48 steps: on, one past and one short of each chunk edge
    "edge_ends": dict(_D, B=7, Tc=3, L=49, lengths=[17, 18, 16, 33, 34, 32, 49], n_codes=[1, 2, 1, 2, 3, 2, 3], options=_chunk(16)),
    # M = 1024: one full slab, a full tile, every row live in both chunks
    "slab_exact": dict(_D, B=16, Tc=8, L=129, options=_chunk(64)),
    # M = 1026: rows 1024 and 1025 (utterance 18, steps 52 and 53 of a chunk) are live in the first two chunks; dim_voc_latent 1024
    "slab_plus_two": dict(_D, B=19, Tc=11, L=163, lengths=[163 - 9 * (b % 5) for b in range(19)], de=32, C=1024, options=_chunk(54)),
    # three tiles at NS = 48: the middle one scores nothing, the last has one live column; utterance 5 has no sample at all
    "h1024_tiles": dict(_D, Hr=1024, B=33, Tc=3, L=49, de=32, C=512,
                        lengths=[0 if b == 5 else 1 if 16 <= b < 32 else 49 for b in range(33)],
                        n_codes=[0 if 16 <= b < 32 else 3 for b in range(33)]),
    # longest = 1: the step kernel runs without its product; N = 2
    "one_step": dict(_D, B=4, Tc=1, L=2, lengths=[2, 1, 0, 2], n_codes=[1, 0, 0, 1]),
    # saturated gates across seven chunk edges
    "stressed_edges": dict(_D, Hr=896, B=2, Tc=8, L=129, weights="stressed", options=_chunk(16)),
}
ALL_WIDE = list(WIDE_CASES)
WIDE_PINS = os.path.join(grad_judge.GOLD, "voc_grad_wide_pins.npz")
ROW_TENSORS = ("embedding", "grad_cond")     # judged per row as well: per class, per (utterance, frame)
FAULTS = ("carry", "straddle")


def chunk_of(c):
    """The chunk of a case in steps, as the library forms it: ``tf_chunk_replays * steps_per_graph`` (defaults 4 and 160)."""
    return c["options"].get("tf_chunk_replays", 4) * c["options"].get("steps_per_graph", 160)

_cases, _refs = {}, {}


def state_dict(c):
    sd = synth.vocoder_state_dict(dim_voc_latent=c["C"], size_i_embed_ar=c["de"], size_h_rnn=c["Hr"])
    return f64_ref.stressed(sd) if c["weights"] == "stressed" else sd


def load(name):
    """A case as a dict: its sizes, ``sd`` (fp32 state dict), ``audio`` (B, L), ``z`` (B, Tc), ``spk`` (B) int64, ``lengths``
    and ``n_codes`` as lists.  Computed once and shared (treat as read-only)."""
    if name not in _cases:
        c = dict(CASES[name] if name in CASES else WIDE_CASES[name], name=name)
        B, Tc, L = c["B"], c["Tc"], c["L"]
        c["sd"] = state_dict(c)
        c["audio"] = (synth.randint(f"voc_grad/{name}/a", (B, L), 256) if c["audio"] == "random"
                      else torch.full((B, L), int(c["audio"]), dtype=torch.int64))
        c["z"] = synth.randint(f"voc_grad/{name}/z", (B, Tc), 512)
        c["spk"] = synth.randint(f"voc_grad/{name}/s", (B,), 102)
        c["lengths"] = [L] * B if c["lengths"] is None else list(c["lengths"])
        c["n_codes"] = [Tc] * B if c["n_codes"] is None else list(c["n_codes"])
        c["slen"] = [max(n - 1, 0) for n in c["lengths"]]
        _cases[name] = c
    return _cases[name]


def weights(c, dtype=torch.float64):
    """The nine tensors of ``rnnms.ar`` as a dict over ``KEYS``."""
    return {k: c["sd"]["rnnms.ar." + n].detach().to(dtype) for k, n in zip(KEYS, SD_NAMES)}


def condition(c, dtype=torch.float64):
    """``F64Vocoder.condition`` of the case in ``dtype``: a list of (2 n_codes[b], C) tensors."""
    return f64_ref.F64Vocoder(c["sd"], upsample=c["up"], dtype=dtype).condition(c["z"], c["spk"], c["n_codes"])


def loss_of(p, cond, audio, slen, up, fault=None, ch=None):
    """The teacher-forced mean NLL from the nine tensors ``p`` (dict over ``KEYS``) and the conditioning rows ``cond`` (list): the
    sample loop of ``F64Vocoder.logits``, differentiable, in the dtype of ``p``.

    ``fault`` (default None: the statements as they are) seeds an error of the backward over chunks of ``ch`` steps, by autograd alone;
    the loss keeps its value.  ``"carry"``: ``h`` is detached at every ``t % ch == 0`` -- nothing is carried across a chunk edge.
    ``"straddle"``: the conditioning term of the steps that lie behind a chunk edge inside their frame is detached -- a frame cut
    by an edge receives the share of its first chunk only."""
    assert fault is None or (fault in FAULTS and ch)
    emb, w_ih, w_hh, b_ih, b_hh = (p[k] for k in KEYS[:5])
    de, Hr = emb.shape[1], w_hh.shape[1]
    B, T = audio.shape[0], max(slen)
    emb_tab = emb @ w_ih[:, :de].T                                               # (n_cls, 3 Hr)
    ctab = torch.cat([c @ w_ih[:, de:].T + b_ih for c in cond] + [torch.zeros(1, 3 * Hr, dtype=emb.dtype)])   # one row per frame, a zero row
    base = np.concatenate([[0], np.cumsum([c.shape[0] for c in cond])])
    fidx = torch.full((B, T), int(base[-1]), dtype=torch.long)                   # steps that are not scored read the zero row
    for b in range(B):
        t = torch.arange(slen[b])
        fidx[b, :slen[b]] = int(base[b]) + t // up
        assert slen[b] == 0 or int(fidx[b, :slen[b]].max()) < int(base[b + 1]), "history longer than the conditioning covers"
    cterm = ctab[fidx]
    if fault == "straddle":
        t = torch.arange(T)
        cterm = torch.where(((t // up) * up < (t // ch) * ch)[None, :, None], cterm.detach(), cterm)
    gi = emb_tab[audio[:, :T]] + cterm                                           # (B, T, 3 Hr)
    w_hh_t = w_hh.T
    h = torch.zeros(B, Hr, dtype=emb.dtype)
    hs = []
    for t in range(T):
        if fault == "carry" and t % ch == 0:
            h = h.detach()
        h = f64_ref._gru_update(gi[:, t], torch.addmm(b_hh, h, w_hh_t), h)
        hs.append(h)
    hs = torch.stack(hs, dim=1)
    a = torch.relu(hs @ p["fc1_weight"].T + p["fc1_bias"])
    e = a @ p["fc2_weight"].T + p["fc2_bias"]
    nll = -torch.log_softmax(e, dim=-1).gather(-1, audio[:, 1:T + 1, None])[..., 0]
    mask = torch.arange(T)[None, :] < torch.tensor(slen)[:, None]
    return torch.where(mask, nll, torch.zeros_like(nll)).sum() / float(sum(slen))


def grads(name, dtype=torch.float64, fault=None):
    """The reference in ``dtype`` on the CPU: dict over ``TENSORS`` plus ``loss``, numpy float64.  ``grad_cond`` is (B, 2 Tc, C) with
    zero rows past an utterance's frames.  ``fault``: ``loss_of``'s, over the case's own chunk."""
    c = load(name)
    with grad_judge.one_thread():
        p = {k: v.clone().requires_grad_(True) for k, v in weights(c, dtype).items()}
        cond = [x.clone().requires_grad_(True) for x in condition(c, dtype)]
        loss = loss_of(p, cond, c["audio"], c["slen"], c["up"], fault, chunk_of(c) if fault else None)
        (loss * (1.0 if c["grad_loss"] is None else c["grad_loss"])).backward()
    out = {k: p[k].grad for k in KEYS}
    gc = torch.zeros(c["B"], 2 * c["Tc"], c["C"], dtype=dtype)
    for b, x in enumerate(cond):
        if x.shape[0]:
            gc[b, :x.shape[0]] = x.grad if x.grad is not None else 0.0
    out["grad_cond"] = gc
    out["loss"] = loss.detach()
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def grads64(name):
    if name not in _refs:
        _refs[name] = grads(name)
    return _refs[name]


def module_grads(name):
    """The same gradients from torch's own modules in float64: ``nn.Embedding`` + ``nn.GRU`` + two ``nn.Linear`` +
    ``F.cross_entropy`` built from the state dict (a case of ``MODULE_CASES``: equal lengths).  -> dict over ``TENSORS`` and ``loss``."""
    import torch.nn as nn
    c = load(name)
    w = weights(c)
    n_cls, de = w["embedding"].shape
    emb, rnn = nn.Embedding(n_cls, de).double(), nn.GRU(de + c["C"], c["Hr"], batch_first=True).double()
    fc1, fc2 = nn.Linear(c["Hr"], 256).double(), nn.Linear(256, n_cls).double()
    params = [emb.weight, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, fc1.weight, fc1.bias, fc2.weight, fc2.bias]
    with torch.no_grad():
        for dst, k in zip(params, KEYS):
            dst.copy_(w[k])
    cond = torch.stack(condition(c)).requires_grad_(True)                        # (B, 2 Tc, C): every utterance has all its codes
    x = c["audio"]
    series = torch.cat((emb(x[:, :-1]), cond.repeat_interleave(c["up"], dim=1)[:, :x.shape[1] - 1]), dim=2)
    e = fc2(torch.relu(fc1(rnn(series)[0])))
    loss = torch.nn.functional.cross_entropy(e.transpose(1, 2), x[:, 1:])
    loss.backward()
    out = {k: q.grad for k, q in zip(KEYS, params)}
    out.update(grad_cond=cond.grad, loss=loss.detach())
    return {k: v.numpy().astype(np.float64) for k, v in out.items()}


def pins():
    return grad_judge.load_pins(PINS, WIDE_PINS)


def judge(name, got, what):
    grad_judge.judge(grads64(name), pins(), name, got, what, TENSORS)


def judge_rows(name, got, what):
    """``embedding`` per class and ``grad_cond`` per utterance and frame of a wide case (``grad_judge.judge_rows``)."""
    return grad_judge.judge_rows(grads64(name), pins(), name, got, what, ROW_TENSORS)
