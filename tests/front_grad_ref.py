"""Shared by the front-end gradient tests (plain module, not a conftest): the cases, the float64 reference, the judge, and two fp32
numpy restatements that show on the CPU that the judge rests on nothing the GPU does.  It follows tests/ctx_grad_ref.py.

Reference: the torch modules ``model.py:43-55`` constructs -- ``nn.Conv1d(C, 512, 4, 2, 1, bias=False)`` and the ``nn.Sequential``
of LayerNorm / ReLU / Linear -- on the CPU in float64, with the loss ``sum(z_pre * G)`` for a seeded upstream ``G`` and gradients by
autograd.  ReLU makes the gradient piecewise, so the reference differentiates the branch the fp32 program took: the five ReLU masks
come from the project's CPU oracle's fp32 forward (``oracle.conv1d_k4s2`` / ``layernorm`` / ``linear``, the bits of the GPU's
stages) and are applied module by module in place of ``nn.ReLU``.  tests/golden/front_grad_pins.npz
(``tools/gen_front_grad_golden.py``) pins it and holds ``e_ref``, the same modules' own fp32 CPU error under the same masks, per
tensor, and per case the number of mask elements in which the float64 run's own ReLUs differ from the forced ones.

Pins and judge, per tensor: tests/grad_judge.py.

``chain``: the whole training step on a small batch -- the modules above, the VQ step with the code indices of the fp32 forward
forced (``model.py:147-150``), ``nn.LSTM`` and ``cpc_grad_ref.loss_torch`` with given negatives, ``loss = cpc + vq`` -- judged by
the same rule with ``e_ref`` from the same composition in torch fp32 on the CPU.

``WIDE_CASES`` (tests/golden/front_grad_wide_pins.npz, the same tool): fourteen more cases at the shapes where the kernels branch
-- a ragged last slab behind two whole ones, an odd slab count, one long utterance on the direct conv order, utterances of one output
frame, the smallest calls, ``in_channels`` 16 / 128 / 144 / 256 across slabs, a silent utterance, a loud batch and an upstream gradient
that is zero but for a few rows -- judged by the same rule (tests/test_gpu_front_grad_wide.py).

``FAULTS``: mistakes seeded into the restatements by a switch, which tests/test_front_grad_cpu.py shows the judge to notice.
"""
import os

import numpy as np
import torch

import cpc_grad_ref
import ctx_grad_ref
import grad_judge
import oracle
from grad_judge import U32  # noqa: F401  (the GPU tests' own bounds read it from here)
from vectorquantizedcpc_amd import synth

f32, f64 = np.float32, np.float64
LN_IDS, FC_IDS = (0, 3, 6, 9, 12), (2, 5, 8, 11)
# the 17 front-end tensors in the member order of vqcpc_encoder_front_weights, and their state_dict() names
KEYS = ["conv"] + [f"ln_g{i}" for i in range(5)] + [f"ln_b{i}" for i in range(5)] + [f"fc{i}" for i in range(4)] + ["out_w", "out_b"]
SD_NAMES = (["conv.weight"] + [f"encoder.{n}.weight" for n in LN_IDS] + [f"encoder.{n}.bias" for n in LN_IDS] +
            [f"encoder.{n}.weight" for n in FC_IDS] + ["encoder.14.weight", "encoder.14.bias"])
PINS = os.path.join(grad_judge.GOLD, "front_grad_pins.npz")
WIDE_PINS = os.path.join(grad_judge.GOLD, "front_grad_wide_pins.npz")
POSITIONS = "front_grad/{name}/{tensor}/pins"          # the seed of a tensor's pinned samples

# name -> B, T, in_channels, conv_mode, variant
CASES = {
    "one_tile": (1, 32, 80, 0, None),                  # 16 rows
    "partial_tile": (3, 42, 80, 0, None),              # 63 rows, utterance edges inside tiles
    "odd_T": (2, 35, 80, 0, None),                     # To = 17, the kept last frame
    "slab_exact": (16, 128, 80, 0, None),              # 1024 rows
    "slab_plus_one": (25, 82, 80, 0, None),            # 1025 rows, one row in the second slab
    "train": (64, 128, 80, 0, None),                   # 4096 rows
    "c16": (2, 40, 16, 0, None),                       # smallest in_channels
    "c256": (2, 40, 256, 0, None),                     # 4C > 512, layered schedule only
    "small_variance": (3, 42, 80, 0, "small_variance"),   # conv weight x 1e-3: LayerNorm's eps decides rstd
    "dead_units": (3, 42, 80, 0, "dead_units"),        # one LayerNorm's beta = -3: columns whose dgamma, dbeta are exactly zero
    "zero_upstream": (3, 42, 80, 0, "zero_upstream"),  # G == 0: everything +0
    "partial_tile_m1": (3, 42, 80, 1, None),           # the two conv orders, asked for by name
    "partial_tile_m2": (3, 42, 80, 2, None),
    "odd_T_m1": (2, 35, 80, 1, None),
    "odd_T_m2": (2, 35, 80, 2, None),
}
ALL_CASES = list(CASES)
SMALL_CASES = [n for n in ALL_CASES if CASES[n][0] * (CASES[n][1] // 2) <= 64]      # what the numpy restatements run
DEAD_LN = 2                                            # dead_units: encoder.6.bias

# the same row format; GRAD_SLAB = 1024 rows, tiles of 16 rows, VQCPC_CONV_AUTO takes the direct order where C * T > 20480
WIDE_CASES = {
    "tail37": (5, 834, 80, 0, None),                   # 2085 rows: three slabs, the last of two whole tiles and one of 5 rows
    "one_long": (1, 4100, 80, 0, None),                # 2050 rows: B = 1 on the direct order by AUTO, slab edges inside one utterance, last slab 2 rows
    "T2": (130, 2, 80, 0, None),                       # To = 1: 130 rows, nine tiles, taps 0 and 3 read only padding
    "T2_m1": (130, 2, 80, 1, None),                    # the same data, the im2col order by name at B > 1
    "T3_m2": (67, 3, 80, 2, None),                     # To = 1 with a third frame: tap 3 live
    "r1": (1, 2, 80, 0, None),                         # one row: the smallest call
    "r17": (1, 34, 80, 0, None),                       # 17 rows: a second tile of one row
    "c16_slabs": (9, 230, 16, 0, None),                # 1035 rows: 4C = 64 across two slabs
    "c128_m1": (3, 42, 128, 1, None),                  # 4C = 512, the last width of the fused schedule
    "c144_slabs": (9, 230, 144, 0, None),              # 4C = 576 > 512, two slabs
    "c256_slabs_m2": (9, 230, 256, 2, None),           # the widest conv, two slabs, the direct order by name
    "silent": (4, 42, 80, 0, "silent"),                # mel[1] = 0: rows whose x_0 is 0, variance 0, rstd = 1 / sqrt(eps)
    "loud": (3, 42, 80, 0, "loud"),                    # mel x 50
    "sparse_G": (9, 230, 80, 0, "sparse"),             # G zero but for rows 0 and 1030 .. 1034, as a loss over a few frames hands it over
}
ALL_WIDE = list(WIDE_CASES)
WIDE_SMALL = [n for n in ALL_WIDE if WIDE_CASES[n][0] * ((WIDE_CASES[n][1] - 2) // 2 + 1) <= 130]   # what kernel_order32 runs of them
SPARSE_ROWS = (0, 1030, 1031, 1032, 1033, 1034)
CHAIN = "chain"

_cases, _fwd, _refs = {}, {}, {}


def _u(name, shape, bound):
    return grad_judge.uniform("front_grad/" + name, shape, bound)


def _base(name):
    """The data a case shares with its conv-order variants."""
    return name[:-3] if name.endswith(("_m1", "_m2")) else name


def load(name):
    """A case as a dict: sizes, ``mel`` (B, C, T) and upstream ``G`` (B, To, 64) as fp32 torch tensors, ``w`` = the 17 front-end
    tensors by ``KEYS``.  Computed once and shared (treat as read-only)."""
    if name not in _cases:
        B, T, C, mode, variant = CASES[name] if name in CASES else WIDE_CASES[name]
        base = _base(name)
        To = (T - 2) // 2 + 1
        sd = synth.encoder_state_dict(in_channels=C, ln_affine="random")
        w = {k: sd[n].clone() for k, n in zip(KEYS, SD_NAMES)}
        if variant == "small_variance":
            w["conv"] = w["conv"] * 1e-3
        if variant == "dead_units":
            w[f"ln_b{DEAD_LN}"] = torch.full_like(w[f"ln_b{DEAD_LN}"], -3.0)
        G = _u(base + "/G", (B, To, 64), 1.0)
        if variant == "zero_upstream":
            G = torch.zeros_like(G)
        if variant == "sparse":
            keep = torch.zeros(B * To, 1)
            keep[list(SPARSE_ROWS)] = 1.0
            G = (G.reshape(B * To, 64) * keep).reshape(B, To, 64)
        mel = synth.mel("front_grad/" + base, B, T, n_mels=C)
        if variant == "silent":
            mel[1] = 0.0
        if variant == "loud":
            mel = mel * 50.0
        _cases[name] = dict(name=name, B=B, T=T, C=C, To=To, R=B * To, mode=mode, mel=mel, G=G, w=w)
    return _cases[name]


def forward32_of(mel, w, mode):
    """The project's CPU oracle's fp32 forward: x[l] (R, 512) entering LN_l, a[l] leaving its ReLU, z_pre (R, 64)."""
    x = oracle.conv1d_k4s2(mel, w["conv"], mode).reshape(-1, 512)
    xs, acts = [], []
    for l in range(5):
        a = oracle.layernorm(x, w[f"ln_g{l}"], w[f"ln_b{l}"], relu=True)
        xs.append(x)
        acts.append(a)
        if l < 4:
            x = oracle.linear(a, w[f"fc{l}"])
    return dict(x=xs, a=acts, z_pre=oracle.linear(acts[4], w["out_w"], w["out_b"]))


def forward32(name):
    if name not in _fwd:
        g = load(name)
        _fwd[name] = forward32_of(g["mel"].numpy(), g["w"], g["mode"])
    return _fwd[name]


def masks(name):
    """The five ReLU masks (R, 512) bool the fp32 program took."""
    return [a > 0 for a in forward32(name)["a"]]


def modules(w, dtype):
    """``model.py:43-55`` as the reference constructs it, holding ``w``."""
    C = w["conv"].shape[1]
    conv = torch.nn.Conv1d(C, 512, 4, 2, 1, bias=False)
    block = lambda: [torch.nn.Linear(512, 512, bias=False), torch.nn.LayerNorm(512), torch.nn.ReLU(True)]
    seq = torch.nn.Sequential(torch.nn.LayerNorm(512), torch.nn.ReLU(True), *[m for _ in range(4) for m in block()], torch.nn.Linear(512, 64))
    sd = dict(zip(SD_NAMES, (w[k] for k in KEYS)))
    conv.load_state_dict({"weight": sd["conv.weight"]})
    seq.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
    return conv.to(dtype), seq.to(dtype)


def params_of(conv, seq):
    ps = dict(conv.named_parameters(prefix="conv"))
    ps.update(seq.named_parameters(prefix="encoder"))
    return [ps[n] for n in SD_NAMES]


def front_torch(conv, seq, mel, forced):
    """z_pre (B, To, 64) with the ReLUs replaced by the forced masks, module by module.  -> (z_pre, mask elements in which this
    run's own ReLUs would have differed)."""
    h = conv(mel).transpose(1, 2)
    differ, l = 0, 0
    for m in seq:
        if isinstance(m, torch.nn.ReLU):
            mk = torch.from_numpy(forced[l]).reshape(h.shape)
            differ += int(((h > 0) != mk).sum())
            h = h * mk.to(h.dtype)
            l += 1
        else:
            h = m(h)
    return h, differ


def torch_grads(name, dtype=torch.float64):
    """The modules on the CPU in ``dtype`` under the fp32 program's masks: dict of the 17 gradients (numpy float64), ``differ``."""
    g = load(name)
    conv, seq = modules(g["w"], dtype)
    z, differ = front_torch(conv, seq, g["mel"].to(dtype), masks(name))
    (z * g["G"].to(dtype)).sum().backward()
    out = {k: p.grad.numpy().astype(f64) for k, p in zip(KEYS, params_of(conv, seq))}
    out["differ"] = differ
    return out


def grads64(name):
    if name not in _refs:
        _refs[name] = chain_grads(torch.float64) if name == CHAIN else torch_grads(name)
    return _refs[name]


def pins():
    return grad_judge.load_pins(PINS, WIDE_PINS)


def bound(name, tensor):
    return grad_judge.bound(pins(), name, tensor)


def tensors(name):
    """The keys of a case's reference that are tensors (``differ`` is a count)."""
    return [k for k in grads64(name) if k != "differ"]


def judge(name, got, what, keys=None):
    grad_judge.judge(grads64(name), pins(), name, got, what, keys or tensors(name))


# ------------------------------------------------------------------ vq_bwd: the float64 formula
def vq_bwd64(z_pre, z_q, grad_z_st, grad_loss):
    """``grad_z_st + grad_loss * (0.5 / (n_rows * z_dim)) * (z_pre - z_q)`` in float64 (either term may be None)."""
    n = z_pre.size
    out = np.zeros(z_pre.shape, f64)
    if grad_z_st is not None:
        out = out + grad_z_st.astype(f64)
    if grad_loss is not None:
        out = out + float(grad_loss) * (0.5 / n) * (z_pre.astype(f64) - z_q.astype(f64))
    return out


# ------------------------------------------------------------------ the whole step (chain)
CHAIN_SHAPE = dict(Spk=2, Utt=2, T=42, n_pred=4, Neg=3, c_dim=256)
CHAIN_KEYS = KEYS + ["w_ih", "w_hh", "b_ih", "b_hh", "W", "b"]
FIT_STEPS, FIT_LR = 6, 0.1        # at lr 0.1 the float64 composition's own loss falls at every one of the 6 steps (1.5365 -> 1.3899); found
                                  # on the CPU with that composition alone, and asserted where it is used
RNN_NAMES = ("rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0")


def chain_case():
    """2 speakers x 2 utterances of 42 mel frames (21 units), 2 prediction steps in use, 3 negatives drawn by ``synth.cpc_negatives``
    and handed over as arrays; encoder weights ``synth.encoder_state_dict(ln_affine="random", codebook="data")``."""
    if CHAIN not in _cases:
        s = CHAIN_SHAPE
        N, To, K = s["Spk"] * s["Utt"], (s["T"] - 2) // 2 + 1, s["n_pred"] // 2
        sd = synth.encoder_state_dict(ln_affine="random", codebook="data", c_dim=s["c_dim"])
        cpc_sd = synth.cpc_state_dict(n_prediction_steps=s["n_pred"], c_dim=s["c_dim"])
        utt, seq = synth.cpc_negatives(13, 0, K, s["Spk"], s["Utt"], s["Neg"], To - K)
        g = dict(s, name=CHAIN, N=N, B=N, C=80, To=To, R=N * To, K=K, L=To - K, mode=0, sd=sd, cpc_sd=cpc_sd, utt=utt, seq=seq,
                 mel=synth.mel("front_grad/chain", N, s["T"]), w={k: sd[n] for k, n in zip(KEYS, SD_NAMES)}, E=sd["codebook.embedding"])
        g.update(dict(zip(("w_ih", "w_hh", "b_ih", "b_hh"), (sd[n] for n in RNN_NAMES))))
        g["W"] = torch.stack([cpc_sd[f"predictors.{k}.weight"] for k in range(K)]).contiguous()
        g["b"] = torch.stack([cpc_sd[f"predictors.{k}.bias"] for k in range(K)]).contiguous()
        g["rows"] = cpc_grad_ref.row_index(dict(K=K, Spk=s["Spk"], Utt=s["Utt"], Neg=s["Neg"], L=To - K, T=To, N=N, utt=utt, seq=seq))
        _cases[CHAIN] = g
    return _cases[CHAIN]


def chain_forced(w, E, mel):
    """The decisions of the fp32 program for the front-end tensors ``w`` and codebook ``E``: (ReLU masks, code indices (R,), the
    smallest margin between the best and the second-best code)."""
    fw = forward32_of(mel.numpy(), w, 0)
    _, idx, d_best, d_second = oracle.vq_encode(fw["z_pre"], E.numpy())
    return [a > 0 for a in fw["a"]], idx.reshape(-1), float((d_second - d_best).min())


def chain_loss(g, p, dtype, forced=None):
    """``cpc + vq`` of the composition with the tensors ``p`` (dict by ``CHAIN_KEYS``, of ``dtype``).  ``forced``: (masks, indices),
    or None = this run's own ReLUs and argmin.  -> (loss, cpc loss, vq loss, indices used, smallest margin between the best and
    the second-best code or None)."""
    mel = g["mel"].to(dtype)
    h = torch.nn.functional.conv1d(mel, p["conv"], None, 2, 1).transpose(1, 2)
    for l in range(5):
        h = torch.nn.functional.layer_norm(h, (512,), p[f"ln_g{l}"], p[f"ln_b{l}"], 1e-5)
        h = h * torch.from_numpy(forced[0][l]).reshape(h.shape).to(dtype) if forced else torch.relu(h)
        h = torch.nn.functional.linear(h, p[f"fc{l}"]) if l < 4 else torch.nn.functional.linear(h, p["out_w"], p["out_b"])
    z_pre, E = h, g["E"].to(dtype)
    margin = None
    if forced:
        idx = torch.from_numpy(forced[1])
    else:
        flat = z_pre.detach().reshape(-1, 64)
        dist = torch.addmm((E ** 2).sum(1) + (flat ** 2).sum(1, keepdim=True), flat, E.t(), alpha=-2.0, beta=1.0)      # model.py:126-130
        idx = torch.argmin(dist, dim=-1)
        two = torch.topk(dist, 2, dim=-1, largest=False).values
        margin = float((two[:, 1] - two[:, 0]).min())
    q = E[idx].reshape(z_pre.shape)
    vq = 0.25 * torch.nn.functional.mse_loss(z_pre, q)
    z = z_pre + (q - z_pre).detach()
    m = torch.nn.LSTM(64, g["c_dim"], batch_first=True).to(dtype)
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    c = torch.func.functional_call(m, dict(zip(names, (p[k] for k in ("w_ih", "w_hh", "b_ih", "b_hh")))), (z,))[0]
    cpc = cpc_grad_ref.loss_torch(z, c, p["W"], p["b"], g["rows"])[0]
    return cpc + vq, cpc, vq, idx.numpy(), margin


def chain_params(g, dtype):
    src = dict(g["w"], **{k: g[k] for k in CHAIN_KEYS[17:]})
    return {k: src[k].to(dtype).clone().requires_grad_(True) for k in CHAIN_KEYS}


def chain_grads(dtype=torch.float64):
    """Gradients of the composition under the fp32 program's masks and indices: numpy float64 by ``CHAIN_KEYS`` (the two LSTM
    biases receive the same values: ``b_rnn``)."""
    g = chain_case()
    p = chain_params(g, dtype)
    mk, idx, _ = chain_forced(g["w"], g["E"], g["mel"])
    chain_loss(g, p, dtype, (mk, idx))[0].backward()
    out = {k: p[k].grad.numpy().astype(f64) for k in CHAIN_KEYS}
    if dtype == torch.float64:
        assert np.allclose(out["b_ih"], out["b_hh"], rtol=1e-9, atol=1e-12)
    return out


# ------------------------------------------------------------------ fp32 restatements
FAULTS = ("mask_from_pre", "drop_means", "pad_rows_counted", "conv_edge", "skip_short_slab",     # seeded into reordered32 only
          "slab_tail_tiles", "ahead_group_dropped", "conv_tail")
fma = ctx_grad_ref.fma


def im2col(mel, To, fault=None):
    """(R, 4 C), column 4 c + tap: zero in the padding and for the frame an odd T leaves over.  ``fault`` "conv_edge": the tap
    before an utterance's first frame reads the last frame of the utterance before it; "conv_tail": a tap past an utterance's end
    reads the first frames of the utterance after it."""
    B, C, T = mel.shape
    cols = np.zeros((B, To, C, 4), f32)
    flat = mel.transpose(1, 0, 2).reshape(C, B * T)
    for tap in range(4):
        for tt in range(To):
            ti = 2 * tt + tap - 1
            if 0 <= ti < T:
                cols[:, tt, :, tap] = mel[:, :, ti]
            elif fault == "conv_edge" and ti < 0:
                cols[1:, tt, :, tap] = flat[:, np.arange(1, B) * T - 1].T
            elif fault == "conv_tail" and ti >= T:
                cols[:-1, tt, :, tap] = mel[1:, :, ti - T]
    return cols.reshape(B * To, 4 * C)


def row_stats(x):
    """mean and rstd of every row as fp32 (the forward's own values up to a rounding: judged by the bound, not by bits)."""
    x64 = x.astype(f64)
    mean = x64.mean(axis=1)
    var = ((x64 - mean[:, None]) ** 2).mean(axis=1)
    return mean.astype(f32)[:, None], (1.0 / np.sqrt(var.astype(f32).astype(f64) + f64(f32(1e-5)))).astype(f32)[:, None]


def chain_dot(A, Wt, kc=64):
    """(R, K) x (K, N) in the order of vq_gemm_chain: fma chains over k ascending, restarted every ``kc``, folded in order."""
    R, K = A.shape
    tot = None
    A64, W64 = A.astype(f64), Wt.astype(f64)
    for k0 in range(0, K, kc):
        acc, tmp = np.zeros((R, Wt.shape[1]), f32), np.empty((R, Wt.shape[1]), f64)
        for k in range(k0, k0 + kc):
            np.multiply(A64[:, k, None], W64[None, k], out=tmp)
            tmp += acc
            acc[...] = tmp
        tot = acc if tot is None else tot + acc
    return tot


def ln_bwd_kernel_order(da, x, a, gamma):
    """front_ln_bwd_kernel + front_ln_slab_kernel + front_sum_parts_kernel: (dy, dbeta, dgamma)."""
    R = da.shape[0]
    mean, rstd = row_stats(x)
    xh = (x - mean) * rstd
    dn = np.where(a > 0, da, f32(0))
    dxh = dn * gamma[None]
    lanes = lambda v: v.reshape(R, 2, 64, 4)                          # column = 256 h + 4 lane + k
    s1, s2 = np.zeros((R, 64), f32), np.zeros((R, 64), f32)
    p2 = dxh * xh
    for h in range(2):
        for k in range(4):
            s1 = s1 + lanes(dxh)[:, h, :, k]
            s2 = s2 + lanes(p2)[:, h, :, k]
    for d in (1, 2, 4, 8, 16, 32):
        s1 = s1 + s1[:, np.arange(64) ^ d]
        s2 = s2 + s2[:, np.arange(64) ^ d]
    m1, m2 = s1[:, :1] * f32(1.0 / 512.0), s2[:, :1] * f32(1.0 / 512.0)
    dy = rstd * ((dxh - m1) - xh * m2)
    tiles = (R + 15) // 16
    pad = lambda v: np.concatenate([v, np.zeros((tiles * 16 - R, 512), f32)]).reshape(tiles, 4, 4, 512)   # [tile, wave, j]
    out = []
    for v in (dn, dn * xh):
        t = pad(v)
        w = np.zeros((tiles, 4, 512), f32)
        for j in range(4):
            w = w + t[:, :, j]
        part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        total = np.zeros(512, f32)
        for t0 in range(0, tiles, 64):
            acc = np.zeros((4, 512), f32)
            for t_ in range(t0, min(t0 + 64, tiles)):
                acc[t_ & 3] = acc[t_ & 3] + part[t_]
            total = total + ((acc[0] + acc[1]) + (acc[2] + acc[3]))
        out.append(total)
    assert dy.dtype == f32 and out[0].dtype == f32
    return dy, out[0], out[1]


def ln_bwd_reordered(da, x, a, gamma, fault=None):
    """Another order: numpy's own sums.  Faults: see ``reordered32``."""
    R = da.shape[0]
    mean, rstd = row_stats(x)
    xh = (x - mean) * rstd
    dn = np.where((x if fault == "mask_from_pre" else a) > 0, da, f32(0))
    dxh = dn * gamma[None]
    m1 = dxh.sum(axis=1, keepdims=True) / f32(512)
    m2 = (dxh * xh).sum(axis=1, keepdims=True) / f32(512)
    dy = rstd * dxh if fault == "drop_means" else rstd * (dxh - m1 - xh * m2)
    cb, cg = dn, dn * xh
    if fault == "pad_rows_counted":                                  # the last tile's padding carries row 0
        extra = [0] * (-R % 16)
        cb, cg = np.concatenate([cb, cb[extra]]), np.concatenate([cg, cg[extra]])
    if fault == "slab_tail_tiles":                                   # the last slab's tiles past its last whole group of four are left out
        r0 = (R - 1) // 1024 * 1024
        kept = r0 + ((R - r0 + 15) // 16) // 4 * 64
        cb, cg = cb[:kept], cg[:kept]
    tree = ctx_grad_ref._tree
    dbeta = np.zeros(512, f32) + tree([cb[r:r + 64].sum(axis=0) for r in range(0, cb.shape[0], 64)])
    dgamma = np.zeros(512, f32) + tree([cg[r:r + 64].sum(axis=0) for r in range(0, cg.shape[0], 64)])
    return dy.astype(f32), dbeta, dgamma


def backward32(name, ln_bwd, wdot, colsum, dot, fault=None):
    """The backward over the oracle's fp32 forward, its four kinds of sums handed in: dict of the 17 gradients, fp32."""
    g, fw = load(name), forward32(name)
    w = {k: v.numpy() for k, v in g["w"].items()}
    G = g["G"].numpy().reshape(g["R"], 64)
    R = g["R"]
    summed = R - R % 1024 if fault == "skip_short_slab" and R % 1024 < 16 else R
    if fault == "ahead_group_dropped":
        summed = R - R % 64
    out = {"out_w": wdot(G[:summed], fw["a"][4][:summed]), "out_b": colsum(G[:summed])}
    d = dot(G, w["out_w"])
    for l in range(4, -1, -1):
        d, out[f"ln_b{l}"], out[f"ln_g{l}"] = ln_bwd(d, fw["x"][l], fw["a"][l], w[f"ln_g{l}"])
        if l == 0:
            cols = im2col(g["mel"].numpy(), g["To"], fault)
            out["conv"] = wdot(d[:summed], cols[:summed]).reshape(512, g["C"], 4)
        else:
            out[f"fc{l - 1}"] = wdot(d[:summed], fw["a"][l - 1][:summed])
            d = dot(d, w[f"fc{l - 1}"])
    assert all(v.dtype == f32 for v in out.values())
    return out


def kernel_order32(name):
    """fp32 numpy in the kernels' documented orders (csrc/front_grad.hip)."""
    return backward32(name, ln_bwd_kernel_order, ctx_grad_ref.slab_dot, ctx_grad_ref.slab_colsum, chain_dot)


def reordered32(name, fault=None):
    """fp32 numpy in orders that are NOT the kernels': 16-wide k chunks for the products, 64-row chunks and an adjacent-pair tree for
    the sums over rows, numpy's sums inside a row.  ``fault`` (one of ``FAULTS``) seeds a mistake a kernel could make:
    "mask_from_pre" takes the ReLU mask from the rows entering the LayerNorm; "drop_means" leaves the two mean terms of the
    LayerNorm backward out; "pad_rows_counted" counts the padded rows of the last 16-row tile (as copies of row 0) in dgamma and
    dbeta; "conv_edge" lets the conv's first tap read across an utterance edge; "skip_short_slab" leaves a last slab of fewer than
    16 rows out of the weight and bias sums."""
    tree = ctx_grad_ref._tree
    wdot = lambda A, X: np.zeros((A.shape[1], X.shape[1]), f32) + tree([A[r:r + 64].T @ X[r:r + 64] for r in range(0, A.shape[0], 64)])
    colsum = lambda A: np.zeros(A.shape[1], f32) + tree([A[r:r + 64].sum(axis=0) for r in range(0, A.shape[0], 64)])
    ln = lambda da, x, a, gamma: ln_bwd_reordered(da, x, a, gamma, fault)
    return backward32(name, ln, wdot, colsum, ctx_grad_ref.chunk_dot, fault)


def chain_sgd(dtype, steps, lr):
    """``steps`` of plain SGD on all 23 tensors of the composition with the codebook frozen, on the CPU in ``dtype``, every step on
    this run's own ReLUs and argmin.  -> (losses cpc + vq, the code indices of every step, final tensors float64, the smallest VQ
    margin over the steps)."""
    g = chain_case()
    p = chain_params(g, dtype)
    losses, picked, margin = [], [], float("inf")
    for _ in range(steps):
        loss, _, _, idx, m = chain_loss(g, p, dtype)
        margin = min(margin, m)
        grads = torch.autograd.grad(loss, [p[k] for k in CHAIN_KEYS])
        losses.append(float(loss.detach()))
        picked.append(idx)
        with torch.no_grad():
            for k, gr in zip(CHAIN_KEYS, grads):
                p[k] -= lr * gr
    return losses, picked, {k: v.detach().numpy().astype(f64) for k, v in p.items()}, margin
