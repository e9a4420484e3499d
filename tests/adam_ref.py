"""Shared by tests/test_adam_cpu.py, test_adam_wide_cpu.py, test_gpu_adam.py and test_gpu_adam_wide.py (plain module, not a
conftest): the numpy fp32 restatement of the update ``include/vqcpc.h`` states, the cases, the float64 / fp32
``torch.optim.Adam`` runs on the CPU that judge it, and the arena of canaries the GPU tests carve a call's buffers from.

The restatement (``scalars``, ``update``): every operation one numpy float32 operation -- correctly rounded, never fused -- in the
header's order; the six scalars formed in Python floats (doubles) and rounded to float32 once each.  ``vqcpc_adam_step`` must
give ITS bits; it and the kernel are both held to ``torch.optim.Adam`` in float64 by the project's judge (tests/grad_judge.py):
``max |x - x64| <= 4 max(e_ref, 2^-24 max |x64|)`` with ``e_ref`` the error of ``torch.optim.Adam`` in fp32 on the CPU.

A case is a list of tensors (``numels``), hyper-parameters, a first update number with the state it starts from, and per update the
kind and scale of every gradient.  Gradients are ``+-scale * U[0.05, 1)`` (or exactly 0), so that g * g and v stay normal fp32
numbers: denormals are not part of the contract.  ``CASES`` are the twelve the kernel went in with; ``WIDE`` are the ones read off
the code afterwards (a full table of mixed sizes, a second launch behind empty tensors, every last-chunk loop count and tail,
``eps``, betas and ``lr`` at their edges, ``-0.0`` gradients, a ladder of gradient scales from the contract's floor to the largest
whose square is finite); ``OTHER`` holds arrays for single tests and is not run through the judge.  Every helper takes a name of
any of the three.
"""
import functools
import math

import numpy as np
import torch

from vectorquantizedcpc_amd import _lib, synth

CHUNK = 4096          # VQCPC_ADAM_CHUNK: the elements one workgroup covers
TABLE = 72            # VQCPC_ADAM_TABLE: the tensors one launch covers
REF_BETAS = (0.9, 0.999)
LR, EPS = 4e-4, 1e-8
KEYS = ("p", "exp_avg", "exp_avg_sq")


def _case(numels, steps, scale=1.0, betas=REF_BETAS, lr=LR, first=1, kinds=None, eps=EPS, per_tensor=False):
    """``kinds``: update number (1-based within the case) -> "half" (half of the elements exactly 0), "negzero" (the same, every
    second zero ``-0.0``) or "zero"; the rest "dense".  ``scale``: one number, or a list with one per tensor.  ``per_tensor``: the
    judge takes every tensor on its own (``judge_snapshot``)."""
    assert not isinstance(scale, list) or len(scale) == len(numels)
    return {"numels": list(numels), "steps": steps, "scale": scale, "betas": betas, "lr": lr, "eps": eps, "first": first,
            "kinds": dict(kinds or {}), "per_tensor": per_tensor}


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


# ------------------------------------------------------------------------------------------------------ past the twelve
MIXED = [[1, CHUNK, CHUNK + 1, 3, 2 * CHUNK + 2, 1025, 257 * 4 + 3, 2][i % 8] for i in range(TABLE)]   # 1, 1, 2, 1, 3, 1, 1, 1 workgroups
LADDER = [2e-14] + [10.0 ** e for e in range(-13, 20)]           # 0.05 * 2e-14 = 1e-15, the contract's floor; (1e19)^2 is finite
_SMALL = [CHUNK + 3, 37]
WIDE = {
    "full_table_mixed": _case(MIXED, 2, scale=1e-3),                                         # the tensor search over an irregular prefix
    "two_launches_mixed": _case([0] + MIXED[:40] + [0, 0] + MIXED[40:] + [0] + [3 * CHUNK + 1, 5, CHUNK - 1, 0], 2),
    "tails": _case([2, 6, 7, 1023, 1025, 1026, 1027, 1029, 2050, 4095, 4092, 4089], 2),    # the last chunk's loop count and tail
    "eps_1e-3": _case(_SMALL, 3, scale=1e-3, eps=1e-3),
    "eps_0": _case(_SMALL, 3, scale=1e-3, eps=0.0),                                          # dense gradients only: 0 / 0 otherwise
    "beta2_0": _case(_SMALL, 3, betas=(0.9, 0.0)),
    "betas_near_1": _case(_SMALL, 3, betas=(0.999, 0.999999)),
    "lr_1": _case(_SMALL, 3, lr=1.0),
    "negzero": _case(_SMALL, 3, kinds={1: "negzero", 3: "negzero"}),
    "ladder_cold": _case([1029] * len(LADDER), 3, scale=list(LADDER), per_tensor=True),
    "ladder_loaded": _case([1029] * len(LADDER), 3, scale=list(LADDER), first=50000, per_tensor=True),
}
OTHER = {
    "nonfinite": _case([CHUNK + 7], 2, first=50000),             # tests/test_gpu_adam_wide.py writes inf, NaN and 3e19 into its gradients
}


def case(name):
    """The case ``name`` of ``CASES``, ``WIDE`` or ``OTHER``."""
    for cases in (CASES, WIDE, OTHER):
        if name in cases:
            return cases[name]
    raise KeyError(name)


def scale_of(c, i):
    """The gradient scale of tensor ``i`` of the case ``c``."""
    return c["scale"][i] if isinstance(c["scale"], list) else c["scale"]


def launches(numels, table=None):
    """The split of a tensor list into launches as ``adam_fill`` makes it (below the grid limit): per launch the numels of its
    tensors, empty ones skipped, ``table`` (``TABLE``) tensors at the most."""
    table = TABLE if table is None else table
    live = [n for n in numels if n]
    return [live[i:i + table] for i in range(0, len(live), table)]


def _u(seed, n):
    return synth.uniform01(seed, n).astype(np.float64)


def params(name):
    """The seeded fp32 parameters of a case, U(-1, 1), one flat array per tensor."""
    return [((_u(f"adam/{name}/p{i}", n) * 2.0 - 1.0)).astype(np.float32) for i, n in enumerate(case(name)["numels"])]


def start_state(name):
    """(exp_avg, exp_avg_sq) a case starts from: zeros at ``first == 1``, else a seeded warm state of the gradients' scale."""
    c = case(name)
    if c["first"] == 1:
        return [np.zeros(n, np.float32) for n in c["numels"]], [np.zeros(n, np.float32) for n in c["numels"]]
    m = [((_u(f"adam/{name}/m{i}", n) * 2.0 - 1.0) * 0.1 * scale_of(c, i)).astype(np.float32) for i, n in enumerate(c["numels"])]
    v = [((0.05 + 0.95 * _u(f"adam/{name}/v{i}", n)) * 0.3 * scale_of(c, i) * scale_of(c, i)).astype(np.float32)
         for i, n in enumerate(c["numels"])]
    return m, v


def grads(name, k):
    """The gradients of update ``k`` (1-based within the case), one flat fp32 array per tensor."""
    c = case(name)
    kind = c["kinds"].get(k, "dense")
    out = []
    for i, n in enumerate(c["numels"]):
        if kind == "zero":
            out.append(np.zeros(n, np.float32))
            continue
        mag = (0.05 + 0.95 * _u(f"adam/{name}/g{i}/{k}", n)) * scale_of(c, i)
        g = np.where(_u(f"adam/{name}/s{i}/{k}", n) < 0.5, -mag, mag)
        if kind in ("half", "negzero"):
            g[::2] = 0.0
        if kind == "negzero":
            g[2::4] = -0.0
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
    c = case(name)
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
    c = case(name)
    m, v = start_state(name)
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(c["first"] - 1)), "exp_avg": torch.from_numpy(m[i]).to(device, dtype),
                       "exp_avg_sq": torch.from_numpy(v[i]).to(device, dtype)} for i in range(len(m))}
    return sd


def run_torch(name, dtype=torch.float64, device="cpu", optimizer=torch.optim.Adam, after_step=None):
    """The case through ``optimizer`` (torch's, or ``optim.Adam`` on the GPU) in ``dtype`` on ``device`` -> snapshots like
    ``restated``'s, as numpy arrays of ``dtype``.  ``after_step(k, ps, opt)``: called after update ``k``."""
    c = case(name)
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


def judge_snapshot(name, k, got, ref64, ref32, what, KEYS=KEYS, per_tensor=None):
    """The project's judge over one snapshot: per key, all tensors of the case as one tensor -- or, with ``per_tensor`` (default:
    what the case ``name`` says, False for a name that is no case), every tensor on its own, so that a tensor many decades below
    the case's largest is held to its own size.  Prints each figure, then asserts.  -> the largest err / bound."""
    if per_tensor is None:
        per_tensor = any(name in cases and cases[name]["per_tensor"] for cases in (CASES, WIDE, OTHER))
    if per_tensor:
        one = lambda snap, i: {key: [snap[key][i]] for key in KEYS}                # noqa: E731
        return max(judge_snapshot(f"{name}#{i}", k, one(got, i), one(ref64, i), one(ref32, i), what, KEYS, False)
                   for i in range(len(ref64[KEYS[0]])))
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


# ------------------------------------------------------------------------------------------------------ the arena of the GPU tests
CANARY = 64
PATTERN = 0x7FA5C3E1          # a NaN payload: arithmetic on it would not give it back


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


class Arena:
    """One device allocation that holds a copy of every fp32 array of ``arrays``, each at the next 16-byte offset, with ``CANARY``
    floats of ``PATTERN`` before and after it."""

    def __init__(self, arrays):
        words = sum(2 * CANARY + (a.size + 3) // 4 * 4 for a in arrays)
        self.host = np.full(words, PATTERN, np.uint32)
        self.spans, at = [], 0
        for a in arrays:
            at += CANARY
            self.host[at:at + a.size] = a.view(np.uint32)
            self.spans.append((at, a.size))
            at += (a.size + 3) // 4 * 4 + CANARY
        assert at == words
        self.dev = torch.from_numpy(self.host.view(np.int32)).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def ptr(self, i):
        assert (self.spans[i][0] * 4) % 16 == 0
        return self.dev.data_ptr() + 4 * self.spans[i][0]

    def read(self):
        return self.dev.cpu().numpy().view(np.uint32)

    def array(self, words, i):
        at, n = self.spans[i]
        return words[at:at + n].view(np.float32)

    def canaries_intact(self, words):
        mask = np.ones(words.size, bool)
        for at, n in self.spans:
            mask[at:at + n] = False
        return bool((words[mask] == PATTERN).all()) and int(mask.sum()) >= 2 * CANARY * len(self.spans)


def arena_case(name, k=1, gs=None):
    """The buffers of update ``k`` of a case -- p, g, m, v of every tensor with elements -- in one arena, and the call's table.
    ``gs``: gradients to take in place of the case's."""
    ps, (ms, vs), gs = params(name), start_state(name), grads(name, k) if gs is None else gs
    arrays = [a for quad in zip(ps, gs, ms, vs) for a in quad if a.size]
    arena = Arena(arrays)
    n = len(arrays) // 4
    table = (_lib.AdamTensor * n)(*[_lib.AdamTensor(arena.ptr(4 * i), arena.ptr(4 * i + 1), arena.ptr(4 * i + 2), arena.ptr(4 * i + 3),
                                                    arrays[4 * i].size) for i in range(n)])
    return arena, table, n, arrays


def hyper(name, k=1, **kw):
    c = case(name)
    h = dict(lr=c["lr"], beta1=c["betas"][0], beta2=c["betas"][1], eps=c["eps"], step=c["first"] + k - 1)
    h.update(kw)
    return _lib.AdamHyper(**h)
