"""Shared by tests/test_adam_cpu.py and tests/test_gpu_adam.py (plain module, not a conftest): the numpy fp32 restatement of the
update ``include/vqcpc_optim.h`` states, the cases, and the float64 / fp32 ``torch.optim.Adam`` runs on the CPU that judge it.

The restatement (``scalars``, ``update``): every operation one numpy float32 operation -- correctly rounded, never fused -- in the
header's order; the six scalars formed in Python floats (doubles) and rounded to float32 once each.  ``vqcpc_adam_step`` must
give ITS bits; it and the kernel are both held to ``torch.optim.Adam`` in float64 by the project's judge (tests/grad_judge.py):
``max |x - x64| <= 4 max(e_ref, 2^-24 max |x64|)`` with ``e_ref`` the error of ``torch.optim.Adam`` in fp32 on the CPU.

A case is a list of tensors (``numels``), hyper-parameters, a first update number with the state it starts from, and per update the
kind and scale of every gradient.  Gradients are ``+-scale * U[0.05, 1)`` (or exactly 0), so that g * g and v stay normal fp32
numbers: denormals are not part of the contract.
"""
import functools
import math

import numpy as np
import torch

from vectorquantizedcpc_amd import synth

CHUNK = 4096          # VQCPC_ADAM_CHUNK: the elements one workgroup covers
TABLE = 72            # VQCPC_ADAM_TABLE: the tensors one launch covers
REF_BETAS = (0.9, 0.999)
LR, EPS = 4e-4, 1e-8
KEYS = ("p", "exp_avg", "exp_avg_sq")


def _case(numels, steps, scale=1.0, betas=REF_BETAS, lr=LR, first=1, kinds=None):
    """``kinds``: update number (1-based within the case) -> "half" (half of the elements exactly 0) or "zero"; the rest "dense"."""
    return {"numels": list(numels), "steps": steps, "scale": scale, "betas": betas, "lr": lr, "eps": EPS, "first": first,
            "kinds": dict(kinds or {})}


PREDICTORS = [n for _ in range(12) for n in (64 * 256, 64)]
CASES = {
    "vector_and_tail": _case([1, 3, 4, 5], 3),                                               # vector body against the scalar tail
    "around_a_chunk": _case([CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3], 3, scale=1e-3),   # a tensor's last workgroup
    "empty_between": _case([5, 0, 7], 1),
    "second_launch": _case([2 + i % 5 for i in range(TABLE + 1)], 3, scale=1e3),             # TABLE + 1 tensors: two launches
    "predictors": _case(PREDICTORS, 20, scale=1e-3, kinds={7: "half", 20: "zero"}),          # warm state, then an all-zero gradient
    "scale_1e-6": _case([1000, 37], 3, scale=1e-6),
    "scale_1e-3": _case([1000, 37], 3, scale=1e-3),
    "scale_1": _case([1000, 37], 3, scale=1.0, kinds={2: "half"}),
    "scale_1e3": _case([1000, 37], 3, scale=1e3),
    "loaded_at_10000": _case([CHUNK + 1, 6], 3, first=10000),                                # a first call on a loaded state
    "lr_zero": _case([9, 260], 3, lr=0.0),
    "betas_0_0.5": _case([CHUNK + 1, 3], 20, betas=(0.0, 0.5), kinds={11: "half"}),
}


def _u(seed, n):
    return synth.uniform01(seed, n).astype(np.float64)


def params(name):
    """The seeded fp32 parameters of a case, U(-1, 1), one flat array per tensor."""
    return [((_u(f"adam/{name}/p{i}", n) * 2.0 - 1.0)).astype(np.float32) for i, n in enumerate(CASES[name]["numels"])]


def start_state(name):
    """(exp_avg, exp_avg_sq) a case starts from: zeros at ``first == 1``, else a seeded warm state of the gradients' scale."""
    c = CASES[name]
    if c["first"] == 1:
        return [np.zeros(n, np.float32) for n in c["numels"]], [np.zeros(n, np.float32) for n in c["numels"]]
    s = c["scale"]
    m = [((_u(f"adam/{name}/m{i}", n) * 2.0 - 1.0) * 0.1 * s).astype(np.float32) for i, n in enumerate(c["numels"])]
    v = [((0.05 + 0.95 * _u(f"adam/{name}/v{i}", n)) * 0.3 * s * s).astype(np.float32) for i, n in enumerate(c["numels"])]
    return m, v


def grads(name, k):
    """The gradients of update ``k`` (1-based within the case), one flat fp32 array per tensor."""
    c = CASES[name]
    kind = c["kinds"].get(k, "dense")
    out = []
    for i, n in enumerate(c["numels"]):
        if kind == "zero":
            out.append(np.zeros(n, np.float32))
            continue
        mag = (0.05 + 0.95 * _u(f"adam/{name}/g{i}/{k}", n)) * c["scale"]
        g = np.where(_u(f"adam/{name}/s{i}/{k}", n) < 0.5, -mag, mag)
        if kind == "half":
            g[::2] = 0.0
        out.append(g.astype(np.float32))
    return out


# ------------------------------------------------------------------------------------------------------ the restatement
def scalars(lr, beta1, beta2, eps, t):
    """The six fp32 scalars of update number ``t``: formed in double, rounded once each."""
    f = np.float32
    return {"w1": f(1.0 - beta1), "c2": f(beta2), "w2": f(1.0 - beta2), "rb": f(math.sqrt(1.0 - beta2 ** float(t))), "e": f(eps),
            "ss": f(lr / (1.0 - beta1 ** float(t)))}


def update(p, g, m, v, k):
    """One update of fp32 arrays, in place, in the header's order of operations."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == np.float32
    m[...] = m + (g - m) * k["w1"]
    v[...] = v * k["c2"] + (g * g) * k["w2"]
    d = np.sqrt(v) / k["rb"] + k["e"]
    p[...] = p - k["ss"] * (m / d)
    assert d.dtype == np.float32


def _snapshot(p, m, v):
    return {"p": [a.copy() for a in p], "exp_avg": [a.copy() for a in m], "exp_avg_sq": [a.copy() for a in v]}


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's ``{"p", "exp_avg", "exp_avg_sq"}`` (lists of flat fp32 arrays) after every update of the case.  Shared: read-only."""
    c = CASES[name]
    p, (m, v) = params(name), start_state(name)
    out = []
    with np.errstate(all="raise", under="ignore"):
        for k in range(1, c["steps"] + 1):
            sc = scalars(c["lr"], *c["betas"], c["eps"], c["first"] + k - 1)
            for pi, gi, mi, vi in zip(p, grads(name, k), m, v):
                update(pi, gi, mi, vi, sc)
            out.append(_snapshot(p, m, v))
    return out


# ------------------------------------------------------------------------------------------------------ torch runs
def loaded_state_dict(opt, name, dtype, device):
    """The state dict that puts ``opt`` (over the case's tensors, in order) at the case's start state: update ``first - 1`` done."""
    c = CASES[name]
    m, v = start_state(name)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(c["first"] - 1)), "exp_avg": torch.from_numpy(m[i]).to(device, dtype),
                       "exp_avg_sq": torch.from_numpy(v[i]).to(device, dtype)} for i in range(len(m))}
    return sd


def run_torch(name, dtype=torch.float64, device="cpu", optimizer=torch.optim.Adam, after_step=None):
    """The case through ``optimizer`` (torch's, or ``optim.Adam`` on the GPU) in ``dtype`` on ``device`` -> snapshots like
    ``restated``'s, as numpy arrays of ``dtype``.  ``after_step(k, ps, opt)``: called after update ``k``."""
    c = CASES[name]
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(device, dtype)) for a in params(name)]
    opt = optimizer(ps, lr=c["lr"], betas=c["betas"], eps=c["eps"])
    if c["first"] != 1:
        opt.load_state_dict(loaded_state_dict(opt, name, dtype, device))
    out = []
    for k in range(1, c["steps"] + 1):
        for p, g in zip(ps, grads(name, k)):
            p.grad = torch.from_numpy(g).to(device, dtype)
        opt.step()
        if after_step is not None:
            after_step(k, ps, opt)
        out.append({"p": [p.detach().cpu().numpy().copy() for p in ps],
                    "exp_avg": [opt.state[p]["exp_avg"].cpu().numpy().copy() for p in ps],
                    "exp_avg_sq": [opt.state[p]["exp_avg_sq"].cpu().numpy().copy() for p in ps]})
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 snapshots, fp32 snapshots) of ``torch.optim.Adam`` on the CPU, after every update.  Shared: read-only."""
    return run_torch(name, torch.float64), run_torch(name, torch.float32)


def judge_snapshot(name, k, got, ref64, ref32, what, KEYS=KEYS):
    """The project's judge over one snapshot: per key, all tensors of the case as one tensor.  Prints each figure, then asserts.
    -> the largest err / bound."""
    import grad_judge as J
    cat = lambda xs: np.concatenate([np.asarray(x).reshape(-1) for x in xs])      # noqa: E731
    ref = {key: cat(ref64[key]) for key in KEYS}
    pins, tag = {}, f"{name}@{k}"
    for key in KEYS:
        pins[f"{tag}_{key}_e_ref"] = float(np.abs(cat(ref32[key]).astype(np.float64) - ref[key]).max())
        pins[f"{tag}_{key}_max"] = float(np.abs(ref[key]).max())
    mine = {key: cat(got[key]) for key in KEYS}
    J.judge(ref, pins, tag, mine, what, KEYS)
    return max(float(np.abs(mine[key].astype(np.float64) - ref[key]).max()) / J.bound(pins, tag, key) for key in KEYS if ref[key].any())
