"""Shared by the context-LSTM gradient tests (plain module, not a conftest): the cases, the float64 reference, the judge, and two
fp32 numpy restatements that show on the CPU that the judge rests on nothing the GPU does.

Reference: ``torch.nn.LSTM(D, H, batch_first=True).double()`` on the CPU -- what ``model.py:57`` constructs -- with the loss
``sum(c * G)`` for a seeded upstream ``G`` and gradients by autograd.  tests/golden/ctx_grad_pins.npz
(``tools/gen_ctx_grad_golden.py``) pins it and holds ``e_ref``, the same module's own fp32 CPU error, per tensor.

Pins and judge, per tensor (c, z, W_ih, W_hh, b): tests/grad_judge.py.

``WIDE_CASES`` (tests/golden/ctx_grad_wide_pins.npz, the same tool): twelve more cases at D = 64 -- nine utterance tiles, row counts
on and one past a slab edge, three tiles at H = 512, thirteen slabs at H = 64, 3 000 steps, the forward suite's ``stressed`` weight
set, and upstream gradients that are zero but for late steps, as ``CPCLoss`` hands them over.  They are judged by that rule and
by ``judge_steps``: the same rule per time step for ``c`` and ``dz``, ``max_{b,d} |G[:, t] - G64[:, t]| <= 4 max(e_ref[t], 2^-24
max |G64[:, t]|)`` with ``e_ref[t]`` the fp32 CPU error of that step, so that a step whose values are orders of magnitude below the
tensor's largest is held to its own size; a step whose float64 values are all zero must come back zero.  ``FAULTS``: mistakes
seeded into the restatements by a switch, which tests/test_ctx_grad_cpu.py shows the judges to notice.

``chain``: the composition ``cpc_grad_ref.loss_torch`` o ``nn.LSTM`` on the CPC fixture ``small_odd`` (its ``z``, index arrays and
predictors; a seeded LSTM), judged by the same rule with ``e_ref`` from the same composition in torch fp32 on the CPU.
"""
import os

import numpy as np
import torch

import cpc_grad_ref
import grad_judge
from grad_judge import U32

f32, f64 = np.float32, np.float64
TENSORS = ("c", "z", "W_ih", "W_hh", "b")
GRADS = TENSORS[1:]
PINS = os.path.join(grad_judge.GOLD, "ctx_grad_pins.npz")
WIDE_PINS = os.path.join(grad_judge.GOLD, "ctx_grad_wide_pins.npz")
POSITIONS = "ctx_grad/{name}/{tensor}/pins"    # the seed of a tensor's pinned samples
STEP_TENSORS = ("c", "z")                      # (B, T, .): judged per time step as well, on the wide cases

# name -> B, T, D, H, weight scale
CASES = {
    "partial_tile": (3, 5, 64, 256, 1),        # a partly filled tile
    "two_tiles": (17, 33, 64, 256, 1),         # two tiles, the second nearly empty; 561 rows, no multiple of any chunk
    "train": (64, 70, 64, 256, 1),             # the train shape
    "long_one": (1, 300, 64, 256, 1),          # long scan, one utterance
    "saturated": (16, 70, 64, 256, 4),         # saturated gates
    "h64": (5, 20, 32, 64, 1),                 # smallest H
    "h128": (33, 12, 64, 128, 1),              # another H
    "h512": (2, 9, 64, 512, 1),                # largest H
    "t1": (4, 1, 64, 256, 1),                  # T = 1: dW_hh must be exactly zero
}
ALL_CASES = list(CASES)

# name -> B, T, H, stressed weights, upstream gradient ("dense", "last" = zero except t = T - 1, or the first t that is zero); D = 64
WIDE_CASES = {
    "b130": (130, 40, 256, False, "dense"),           # nine tiles, 2 live columns in the last; 5200 rows: six slabs, 80 rows in the last
    "slab_exact": (16, 64, 256, False, "dense"),      # 1024 rows: one full slab, a full tile
    "slab_plus_one": (25, 41, 256, False, "dense"),   # 1025 rows: the second slab holds one row
    "h512_tiles": (33, 40, 512, False, "dense"),      # three tiles at NS = 32
    "h64_slabs": (130, 100, 64, False, "dense"),      # smallest H, 13 slabs
    "long": (2, 3000, 256, False, "dense"),           # 3000 steps of BPTT
    "long_stressed": (2, 3000, 256, True, "dense"),   # saturated gates, a long carry chain
    "b17_stressed": (17, 500, 256, True, "dense"),    # the same across a tile edge
    "tail": (3, 60, 256, False, "last"),              # max |dz[t]| from 0.24 down to 1.7e-13
    "tail_stressed": (3, 200, 256, True, "last"),     # max |dz[t]| from 1.76 down to 1.5e-4
    "tail_h64": (18, 60, 64, False, "last"),          # the same at H = 64, two tiles
    "cpc_shaped": (8, 70, 256, False, 64),            # zero for t >= 64: what CPCLoss (K = 6) hands over
}
ALL_WIDE = list(WIDE_CASES)
CHAIN = "chain"                                # the composition with CPCLoss on small_odd

_cases, _refs = {}, {}


def _u(name, shape, bound):
    return grad_judge.uniform("ctx_grad/" + name, shape, bound)


def lstm_weights(name, D, H, scale=1):
    """Seeded ``nn.LSTM`` parameters, U(+-1 / sqrt(H)) as it initialises them, times ``scale``."""
    k = scale / np.sqrt(H)
    return {"w_ih": _u(name + "/w_ih", (4 * H, D), k), "w_hh": _u(name + "/w_hh", (4 * H, H), k),
            "b_ih": _u(name + "/b_ih", (4 * H,), k), "b_hh": _u(name + "/b_hh", (4 * H,), k)}


def load(name):
    """A case as a dict of fp32 torch tensors: ``z`` (B, T, D), ``w_ih`` ``w_hh`` ``b_ih`` ``b_hh``, upstream ``G`` (B, T, H), and its
    sizes.  Computed once and shared (treat as read-only)."""
    if name not in _cases and name in WIDE_CASES:
        _cases[name] = _load_wide(name)
    if name not in _cases:
        B, T, D, H, scale = CASES[name]
        g = dict(name=name, B=B, T=T, D=D, H=H, scale=scale, z=_u(name + "/z", (B, T, D), 1.0), G=_u(name + "/G", (B, T, H), 1.0))
        g.update(lstm_weights(name, D, H, scale))
        _cases[name] = g
    return _cases[name]


def _load_wide(name):
    B, T, H, stress, upstream = WIDE_CASES[name]
    D = 64
    G = _u(name + "/G", (B, T, H), 1.0)
    if upstream == "last":
        G[:, :T - 1] = 0.0
    elif upstream != "dense":
        G[:, upstream:] = 0.0
    g = dict(name=name, B=B, T=T, D=D, H=H, scale=1, z=_u(name + "/z", (B, T, D), 1.0), G=G)
    g.update(lstm_weights(name, D, H))
    if stress:                                 # oracle/f64_enc_ref.py: stressed
        for k in ("w_ih", "b_ih", "b_hh"):
            g[k] = g[k] * 8.0
        g["b_ih"][H:2 * H] += 3.0
    return g


def module(g, dtype=torch.float64):
    m = torch.nn.LSTM(g["D"], g["H"], batch_first=True)
    with torch.no_grad():
        for dst, src in ((m.weight_ih_l0, "w_ih"), (m.weight_hh_l0, "w_hh"), (m.bias_ih_l0, "b_ih"), (m.bias_hh_l0, "b_hh")):
            dst.copy_(g[src])
    return m.to(dtype)


def torch_grads(name, dtype=torch.float64):
    """``nn.LSTM`` on the CPU in ``dtype``: dict c, z, W_ih, W_hh, b as numpy float64."""
    g = load(name)
    m = module(g, dtype)
    z = g["z"].to(dtype).requires_grad_(True)
    c = m(z)[0]
    (c * g["G"].to(dtype)).sum().backward()
    if dtype == torch.float64:             # one mathematical quantity; torch sums it twice, in orders of its own
        assert torch.allclose(m.bias_ih_l0.grad, m.bias_hh_l0.grad, rtol=1e-9, atol=1e-12)
    out = {"c": c.detach(), "z": z.grad, "W_ih": m.weight_ih_l0.grad, "W_hh": m.weight_hh_l0.grad, "b": m.bias_ih_l0.grad}
    return {k: v.numpy().astype(f64) for k, v in out.items()}


def grads64(name):
    if name not in _refs:
        _refs[name] = chain_grads(torch.float64) if name == CHAIN else torch_grads(name)
    return _refs[name]


def pins():
    return grad_judge.load_pins(PINS, WIDE_PINS)


def bound(name, tensor):
    return grad_judge.bound(pins(), name, tensor)


def judge(name, got, what):
    ref = grads64(name)
    grad_judge.judge(ref, pins(), name, got, what, list(ref))


def step_max(a):
    """(B, T, n) -> (T,): the largest magnitude of every time step."""
    return np.abs(a).max(axis=(0, 2))


def judge_steps(name, got, what):
    """``c`` and ``dz`` of a wide case against float64 step by step: for every t, ``max_{b,d} |G[:, t] - G64[:, t]| <=
    4 max(e_ref[t], 2^-24 max |G64[:, t]|)``, and a step that is identically zero in float64 comes back zero.  Prints the worst
    ratio to the bound and its t, then asserts."""
    ref, p = grads64(name), pins()
    bad = []
    for k in STEP_TENSORS:
        if got.get(k) is None:
            continue
        a = np.asarray(got[k]).astype(f64)
        assert a.shape == ref[k].shape, (k, a.shape, ref[k].shape)
        top, e_ref = p[f"{name}_{k}_step_max"], p[f"{name}_{k}_step_e_ref"]
        limit = 4.0 * np.maximum(e_ref, U32 * top)
        zero = top == 0.0
        with np.errstate(invalid="ignore"):
            err = np.where(np.isfinite(a).all(axis=(0, 2)), step_max(a - ref[k]), np.inf)
        ratio = np.where(zero, np.where(err == 0.0, 0.0, np.inf), err / np.where(zero, 1.0, limit))
        t = int(ratio.argmax())
        print(f"{what} {name} {k} per step: worst err / bound = {ratio[t]:.3f} at t = {t} (err {err[t]:.3g}, e_ref[t] {e_ref[t]:.3g}, "
              f"max|G64[:, t]| = {top[t]:.3g}); max|G64[:, t]| spans {top.min():.3g} .. {top.max():.3g}; {int(zero.sum())} zero steps")
        if not ratio[t] <= 1.0:
            bad.append((k, t, float(err[t]), float(limit[t])))
    assert not bad, bad


# ------------------------------------------------------------------ the composition with CPCLoss (small_odd)
def chain_case():
    """``small_odd`` of the CPC tests with a seeded LSTM in front of its ``c``: z, index arrays and predictors are the fixture's."""
    if CHAIN not in _cases:
        s = cpc_grad_ref.load("small_odd")
        g = dict(s, D=64, H=s["c_dim"], rows=cpc_grad_ref.row_index(s))
        g.update(lstm_weights(CHAIN, 64, s["c_dim"]))
        _cases[CHAIN] = g
    return _cases[CHAIN]


_chain_modules = {}
CHAIN_PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh", "W", "b")


def chain_loss(g, z, params):
    """``loss_torch(z, LSTM(z), W, b)`` in the dtype of ``params`` (dict of the six tensors).  -> (loss, c)."""
    m = _chain_modules.get(z.dtype)
    if m is None:
        m = _chain_modules[z.dtype] = torch.nn.LSTM(64, g["H"], batch_first=True).to(z.dtype)
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    c = torch.func.functional_call(m, dict(zip(names, (params[k] for k in CHAIN_PARAMS[:4]))), (z,))[0]
    return cpc_grad_ref.loss_torch(z, c, params["W"], params["b"], g["rows"])[0], c


def chain_params(g, dtype):
    return {k: g[k].to(dtype).clone().requires_grad_(True) for k in CHAIN_PARAMS}


def chain_grads(dtype=torch.float64):
    """Gradients of the composition with respect to the LSTM's tensors (and the value of c): numpy float64."""
    g = chain_case()
    p = chain_params(g, dtype)
    loss, c = chain_loss(g, g["z"].to(dtype), p)
    loss.backward()
    if dtype == torch.float64:
        assert torch.allclose(p["b_ih"].grad, p["b_hh"].grad, rtol=1e-9, atol=1e-12)
    out = {"c": c.detach(), "W_ih": p["w_ih"].grad, "W_hh": p["w_hh"].grad, "b": p["b_ih"].grad}
    return {k: v.numpy().astype(f64) for k, v in out.items()}


def chain_sgd(dtype, steps, lr):
    """``steps`` of plain SGD on the six tensors of the composition, on the CPU in ``dtype``.  -> (losses, final tensors float64)."""
    g = chain_case()
    p = chain_params(g, dtype)
    z, losses = g["z"].to(dtype), []
    for _ in range(steps):
        loss, _ = chain_loss(g, z, p)
        grads = torch.autograd.grad(loss, [p[k] for k in CHAIN_PARAMS])
        losses.append(float(loss.detach()))
        with torch.no_grad():
            for k, gr in zip(CHAIN_PARAMS, grads):
                p[k] -= lr * gr
    return losses, {k: v.detach().numpy().astype(f64) for k, v in p.items()}


# ------------------------------------------------------------------ fp32 restatements
def fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in float64, the sum is rounded to float64 and then to fp32 (a double rounding
    that differs from the hardware's single one in rare ties: these restatements are judged by the bound, not by bits)."""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def split_k_dot(A, Bm):
    """(M, K) x (K, N) in the order of the step kernels (csrc/context_grad.hip, seq_step.h): K over four waves, NS = K / 64
    super-steps of 16 k per wave; MFMA c of super-step s takes k = 16 (w NS + s) + 4 q + c, q = 0 .. 3 in order, into accumulator
    c mod 2; a wave's sum is a0 + a1, the waves are combined ((w0 + w1) + w2) + w3."""
    M, K = A.shape
    N = Bm.shape[1]
    NS = K // 64
    A5 = np.ascontiguousarray(A.astype(f64).reshape(M, 4, NS, 4, 4).transpose(2, 3, 4, 1, 0))[..., None]    # [s, q, c, w, m, 1]
    B5 = np.ascontiguousarray(Bm.astype(f64).reshape(4, NS, 4, 4, N).transpose(1, 2, 3, 0, 4))[:, :, :, :, None]   # [s, q, c, w, 1, n]
    acc, tmp = np.zeros((2, 4, M, N), f32), np.empty((4, M, N), f64)
    for s in range(NS):
        for c in range(4):
            for q in range(4):                                                 # fma(), without its temporaries
                np.multiply(A5[s, q, c], B5[s, q, c], out=tmp)
                tmp += acc[c & 1]
                acc[c & 1][...] = tmp
    w = acc[0] + acc[1]
    return ((w[0] + w[1]) + w[2]) + w[3]


def sigmoid32(v):
    return (f32(1) / (f32(1) + np.exp(-v))).astype(f32)


def forward32(g, dot):
    """The LSTM forward in fp32 numpy, the recurrent product by ``dot``: the input projection is ``bias + chain`` with the chain an
    fma chain over k ascending (vq_gemm_chain), the cell update as seq_step.h writes it (numpy's exp / tanh for libm's)."""
    (B, T, D), H = g["z"].shape, g["H"]
    z, w_ih, w_hh = g["z"].numpy(), g["w_ih"].numpy(), g["w_hh"].numpy()
    bias = g["b_ih"].numpy() + g["b_hh"].numpy()
    chain, tmp = np.zeros((B * T, 4 * H), f32), np.empty((B * T, 4 * H), f64)
    zr, w64 = z.reshape(B * T, D).astype(f64), w_ih.astype(f64)
    for k in range(D):
        np.multiply(zr[:, k, None], w64[None, :, k], out=tmp)
        tmp += chain
        chain[...] = tmp
    gi = (bias[None] + chain).reshape(B, T, 4 * H)
    gates, cell, tanhc, out = (np.zeros((B, T, n), f32) for n in (4 * H, H, H, H))
    h, cs = np.zeros((B, H), f32), np.zeros((B, H), f32)
    for t in range(T):
        a = gi[:, t] + dot(w_hh, np.ascontiguousarray(h.T)).T
        i, f, gg, o = sigmoid32(a[:, :H]), sigmoid32(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sigmoid32(a[:, 3 * H:])
        cs = f * cs + i * gg
        tc = np.tanh(cs)
        h = o * tc
        gates[:, t], cell[:, t], tanhc[:, t], out[:, t] = np.concatenate([i, f, gg, o], axis=1), cs, tc, h
    assert out.dtype == f32 and cell.dtype == f32
    return gates, cell, tanhc, out


FAULTS = ("drop_rec", "flush_small", "masked_reads_col0", "skip_short_slab")     # seeded into the restatements only: scan32, products32, reordered32
DROP_REC_STEPS, FLUSH_BELOW = 30, 1e-6


def scan32(g, gates, cell, tanhc, grad_c, dot, fault=None):
    """The backward scan in the order of ctx_bwd_step_kernel: dA (B, T, 4H) fp32.  ``fault``: "drop_rec" leaves the recurrent term
    out for t < T - 30; "flush_small" stores as zero every dA value below 1e-6 of the largest stored so far (the scan starts at the
    largest where the upstream gradient sits on the last step)."""
    B, T, H = grad_c.shape
    w_hh = g["w_hh"].numpy()
    w_hhT = np.ascontiguousarray(w_hh.T)
    dA = np.zeros((B, T, 4 * H), f32)
    carry = np.zeros((B, H), f32)
    one = f32(1)
    top = 0.0
    for t in range(T - 1, -1, -1):
        dh_rec = dot(w_hhT, np.ascontiguousarray(dA[:, t + 1].T)).T if t + 1 < T else np.zeros((B, H), f32)
        if fault == "drop_rec" and t < T - DROP_REC_STEPS:
            dh_rec = np.zeros((B, H), f32)
        i, f, gg, o = (gates[:, t, q * H:(q + 1) * H] for q in range(4))
        tc = tanhc[:, t]
        cp = cell[:, t - 1] if t > 0 else np.zeros((B, H), f32)
        dh = grad_c[:, t] + dh_rec
        do_ = dh * tc
        dct = (dh * o) * (one - tc * tc) + carry
        dA[:, t, :H] = (dct * gg) * (i * (one - i))
        dA[:, t, H:2 * H] = (dct * cp) * (f * (one - f))
        dA[:, t, 2 * H:3 * H] = (dct * i) * (one - gg * gg)
        dA[:, t, 3 * H:] = do_ * (o * (one - o))
        if fault == "flush_small":
            top = max(top, float(np.abs(dA[:, t]).max()))
            dA[:, t][np.abs(dA[:, t]) < FLUSH_BELOW * top] = 0.0
        carry = dct * f
    return dA


def slab_dot(A, X, slab=1024):
    """A^T X over the rows in the order of ctx_grad_w_kernel + ctx_grad_w_finish_kernel: slabs of 1024 rows added in slab order; in a
    slab MFMA (s, c) takes rows r0 + 16 s + 4 q + c, q = 0 .. 3 in order, into accumulator c mod 2; the two added at the end."""
    R, M = A.shape
    total = np.zeros((M, X.shape[1]), f32)
    A64, X64, tmp = A.astype(f64), X.astype(f64), np.empty((M, X.shape[1]), f64)
    for r0 in range(0, R, slab):
        acc = np.zeros((2, M, X.shape[1]), f32)
        for s in range((min(slab, R - r0) + 15) // 16):
            for c in range(4):
                for q in range(4):
                    r = r0 + 16 * s + 4 * q + c
                    if r < R:                                                  # fma(), without its temporaries
                        np.multiply(A64[r][:, None], X64[r][None, :], out=tmp)
                        tmp += acc[c & 1]
                        acc[c & 1][...] = tmp
        total = total + (acc[0] + acc[1])
    return total


def slab_colsum(A, slab=1024):
    """Column sums in the order of ctx_grad_b_kernel + the finish kernel: per slab, rows r0 + rg + 4 i into accumulator i mod 4,
    (a0 + a1) + (a2 + a3), the four row groups combined the same way."""
    R, M = A.shape
    total = np.zeros(M, f32)
    for r0 in range(0, R, slab):
        blk = np.zeros((slab, M), f32)
        blk[:min(slab, R - r0)] = A[r0:r0 + slab]
        blk = blk.reshape(slab // 16, 4, 4, M)                                 # r - r0 = 16 i' + 4 q + rg
        a = np.zeros((4, 4, M), f32)
        for i in range(slab // 16):
            a = a + blk[i]
        per_rg = (a[0] + a[1]) + (a[2] + a[3])
        total = total + ((per_rg[0] + per_rg[1]) + (per_rg[2] + per_rg[3]))
    return total


def products32(g, dA, out, wdot, colsum, dot, fault=None):
    """``fault`` "skip_short_slab": a last slab of fewer than 16 rows is left out of the weight and bias sums."""
    B, T, H4 = dA.shape
    H, D = H4 // 4, g["D"]
    A = dA.reshape(B * T, H4)
    h_prev = np.zeros_like(out)
    h_prev[:, 1:] = out[:, :-1]
    X = np.concatenate([g["z"].numpy().reshape(B * T, D), h_prev.reshape(B * T, H)], axis=1)
    summed = B * T - B * T % 1024 if fault == "skip_short_slab" and B * T % 1024 < 16 else B * T
    dW = wdot(A[:summed], X[:summed])
    res = {"W_ih": dW[:, :D], "W_hh": dW[:, D:], "b": colsum(A[:summed]), "z": dot(A, g["w_ih"].numpy()).reshape(B, T, D)}
    assert all(v.dtype == f32 for v in res.values())
    return res


def kernel_order32(name, grad_c=None):
    """fp32 numpy in the kernels' documented orders (csrc/context_grad.hip): dict c, z, W_ih, W_hh, b."""
    g = chain_case() if name == CHAIN else load(name)
    gates, cell, tanhc, out = forward32(g, split_k_dot)
    dA = scan32(g, gates, cell, tanhc, g["G"].numpy() if grad_c is None else grad_c, split_k_dot)
    return dict(products32(g, dA, out, slab_dot, slab_colsum, split_k_dot), c=out)


def chunk_dot(A, Bm):
    """Another order: 16-wide k chunks, each a BLAS product, added in order."""
    out = np.zeros((A.shape[0], Bm.shape[1]), f32)
    for k in range(0, A.shape[1], 16):
        out = out + A[:, k:k + 16] @ Bm[k:k + 16]
    return out


def _tree(parts):
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def reordered32(name, fault=None):
    """fp32 numpy in orders that are NOT the kernels': 16-wide k chunks for the products, 64-row chunks and an adjacent-pair tree for
    the weight sums.

    ``fault`` (one of ``FAULTS``) seeds a mistake a kernel could make, to show that the judges notice it.  "masked_reads_col0": the
    columns b >= B of the last 16-utterance tile carry utterance 0 where the kernels put zeros.  Inside the scan that is invisible by
    construction (an output column depends on its own input column only, and the masked columns are not stored); it shows where the
    masked columns' rows enter a sum over rows, so the restatement runs the batch padded to whole tiles with copies of utterance 0,
    sums dW and db over all of it, and returns ``c`` and ``dz`` of the first B."""
    g = load(name)
    B = g["B"]
    if fault == "masked_reads_col0":
        pad = [0] * (-B % 16)
        g = dict(g, z=torch.cat([g["z"], g["z"][pad]]), G=torch.cat([g["G"], g["G"][pad]]))
    gates, cell, tanhc, out = forward32(g, chunk_dot)
    dA = scan32(g, gates, cell, tanhc, g["G"].numpy(), chunk_dot, fault)
    # added to a zeroed gradient, as an accumulating .grad is
    wdot = lambda A, X: np.zeros((A.shape[1], X.shape[1]), f32) + _tree([A[r:r + 64].T @ X[r:r + 64] for r in range(0, A.shape[0], 64)])
    colsum = lambda A: np.zeros(A.shape[1], f32) + _tree([A[r:r + 64].sum(axis=0) for r in range(0, A.shape[0], 64)])
    res = dict(products32(g, dA, out, wdot, colsum, chunk_dot, fault), c=out)
    res["c"], res["z"] = res["c"][:B], res["z"][:B]
    return res
