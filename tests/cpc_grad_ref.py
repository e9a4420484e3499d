"""Shared by the CPC gradient tests (plain module, not a conftest): the cases, the float64 reference of the gradients, the
judge, and a differently ordered fp32 backward that shows on the CPU that the judge rests on nothing the GPU does.

Cases: the four recorded fixtures of tests/test_cpc_cpu.py (the reference's own draws), the six cases of tests/cpc_cases.py and
``long`` (L = 1099: 68 full tiles and one with 11 live anchors, more destination rows than any LDS tile of the dz pass holds).

Reference: ``grads64`` -- the forward restated in torch float64 from the two index arrays and differentiated by autograd.
tests/golden/cpc_grad_pins.npz (``tools/gen_cpc_grad_golden.py``) pins it to the reference project's ``CPCLoss(...).double()``
with the same draws replayed and ``loss.backward()``, and holds ``e_ref``, the reference's own fp32 error per tensor.

Pins and judge, per tensor (z, c, W, b): tests/grad_judge.py.
"""
import os

import numpy as np
import torch

import cpc_cases
import grad_judge
import test_cpc_cpu

TENSORS = ("z", "c", "W", "b")
PINS = os.path.join(grad_judge.GOLD, "cpc_grad_pins.npz")
POSITIONS = "cpc_grad/{name}/{tensor}"         # the seed of a tensor's pinned samples

# name -> Spk, Utt, Neg, T, n_prediction_steps, c_dim, n_codes, runs, wscale (the row format of cpc_cases.CASES)
LONG = {"long": (1, 2, 2, 1100, 2, 64, 512, True, 1)}
FIXTURES = list(test_cpc_cpu.FULL_CASES)
ALL_CASES = FIXTURES + list(cpc_cases.CASES) + list(LONG)

_cases, _g64 = {}, {}


def load(name):
    """A case as a dict: sizes, ``sd``, fp32 ``z`` ``c`` (torch), ``utt`` ``seq`` (int64 torch), ``W`` (K, 64, C) and ``b`` (K, 64)
    stacked.  Computed once and shared (treat as read-only)."""
    if name in _cases:
        return _cases[name]
    if name in FIXTURES:
        f = test_cpc_cpu.load_case(name)
        sd, z, c = test_cpc_cpu.case_inputs(f, name)
        g = {k: f[k] for k in ("n_pred", "Spk", "Utt", "Neg", "c_dim", "T", "K", "N", "L")}
        g.update(name=name, J=1 + f["Neg"], sd=sd, z=z, c=c, utt=torch.from_numpy(f["utt"]), seq=torch.from_numpy(f["seq"]))
    else:
        if name in LONG:
            Spk, Utt, Neg, T, n_pred, c_dim, n_codes, runs, wscale = LONG[name]
            K = n_pred // 2
            g = dict(name=name, Spk=Spk, Utt=Utt, Neg=Neg, T=T, T0=T, n_pred=n_pred, c_dim=c_dim, n_codes=n_codes, runs=runs,
                     wscale=wscale, K=K, N=Spk * Utt, L=T - K, J=1 + Neg)
        else:
            g = cpc_cases.case(name)
        g["sd"] = cpc_cases.state_dict(g)
        g["z"], g["c"] = cpc_cases.inputs(g)
        g["utt"], g["seq"] = cpc_cases.negatives(g)
    g["W"] = torch.stack([g["sd"][f"predictors.{k}.weight"] for k in range(g["K"])]).contiguous()
    g["b"] = torch.stack([g["sd"][f"predictors.{k}.bias"] for k in range(g["K"])]).contiguous()
    _cases[name] = g
    return g


def row_index(g):
    """(K, N, J, L) int64: the row of ``z.reshape(N * T, 64)`` that pair (k, n, j, t) scores -- j = 0 the positive (n, t + k),
    j >= 1 negative j: (spk * Utt + utt_index[k, utt, j], seq_index[k, spk, utt, j, t] + k)."""
    K, Spk, Utt, Neg, L, T, N = g["K"], g["Spk"], g["Utt"], g["Neg"], g["L"], g["T"], g["N"]
    utt, seq = g["utt"].numpy(), g["seq"].numpy()
    rows = np.empty((K, N, 1 + Neg, L), np.int64)
    spk = np.arange(Spk).reshape(Spk, 1, 1, 1)
    for k in range(1, K + 1):
        rows[k - 1, :, 0] = np.arange(N)[:, None] * T + np.arange(L) + k
        rows[k - 1, :, 1:] = ((spk * Utt + utt[k - 1][None, :, :, None]) * T + seq[k - 1] + k).reshape(N, Neg, L)
    return rows


def loss_torch(z, c, W, b, rows):
    """The objective from the row index, in the dtype of its arguments: step k predicts ``W_k c + b_k`` at the first L frames,
    scores it against the 1 + Neg rows of each anchor (dot product / 8) and takes the cross entropy against entry 0; the loss is
    the mean over steps of the mean over anchors.  -> (loss, step losses)."""
    K, N, J, L = rows.shape
    zf = z.reshape(-1, z.shape[-1])
    steps = []
    for k in range(K):
        wc = torch.nn.functional.linear(c[:, :L], W[k], b[k])                          # (N, L, 64)
        zr = zf[torch.from_numpy(rows[k])]                                             # (N, J, L, 64)
        f = (zr * wc[:, None] / 8.0).sum(-1)
        steps.append((torch.logsumexp(f, dim=1) - f[:, 0]).mean())
    steps = torch.stack(steps)
    return steps.mean(), steps


def grads64(name):
    """Float64 gradients of a case by autograd on ``loss_torch``: dict z, c, W, b (numpy float64), ``loss``, ``step_loss``."""
    if name not in _g64:
        g = load(name)
        leaves = [g[k].double().requires_grad_(True) for k in TENSORS]
        loss, steps = loss_torch(*leaves, row_index(g))
        loss.backward()
        _g64[name] = dict({k: t.grad.numpy() for k, t in zip(TENSORS, leaves)}, loss=float(loss.detach()), step_loss=steps.detach().numpy())
    return _g64[name]


def pins():
    return grad_judge.load_pins(PINS)


def bound(name, tensor):
    return grad_judge.bound(pins(), name, tensor)


def judge(name, got, what):
    grad_judge.judge(grads64(name), pins(), name, got, what, TENSORS)


def reordered32(name):
    """An fp32 numpy backward in orders that are NOT the kernels': Wc from two interleaved accumulators over the input channels,
    scores from four chains (d mod 4), softmax by numpy's own sums, dWc by a sequential sum over j, dW / db from partials of 16
    rows added in order, dc one matrix product per step, dz scattered row by row in (k, n, j, t) order."""
    g = load(name)
    f32 = np.float32
    K, N, L, T, C, J = g["K"], g["N"], g["L"], g["T"], g["c_dim"], g["J"]
    z, c, W, b = (g[k].numpy().astype(f32) for k in TENSORS)
    rows = row_index(g)
    zf = z.reshape(N * T, 64)
    dz, dc = np.zeros_like(zf), np.zeros_like(c)
    dW, db = np.zeros_like(W), np.zeros_like(b)
    count = f32(K * N * L)
    for k in range(K):
        cl = c[:, :L]
        a0, a1 = np.zeros((N, L, 64), f32), np.zeros((N, L, 64), f32)
        for ch in range(0, C, 2):
            a0 += cl[:, :, ch, None] * W[k, :, ch]
            a1 += cl[:, :, ch + 1, None] * W[k, :, ch + 1]
        wc = (a0 + a1) + b[k]
        zr = zf[rows[k]]                                                               # (N, J, L, 64)
        prod = zr * wc[:, None]
        chains = np.zeros((N, J, L, 4), f32)
        for q in range(16):
            chains += prod[..., 4 * q:4 * q + 4]
        f = ((chains[..., 0] + chains[..., 1]) + (chains[..., 2] + chains[..., 3])) * f32(0.125)
        e = np.exp(f - f.max(axis=1, keepdims=True))
        gk = e / e.sum(axis=1, keepdims=True)
        gk[:, 0] -= f32(1)
        gk = gk / count
        assert gk.dtype == f32
        dwc = np.zeros((N, L, 64), f32)
        for j in range(J):
            dwc += gk[:, j, :, None] * zr[:, j]
        dwc *= f32(0.125)
        A, B = dwc.reshape(N * L, 64), cl.reshape(N * L, C)
        for r in range(0, N * L, 16):
            dW[k] += A[r:r + 16].T @ B[r:r + 16]
            db[k] += A[r:r + 16].sum(axis=0)
        dc[:, :L] += dwc @ W[k]
        np.add.at(dz, rows[k].reshape(-1), ((gk[..., None] * wc[:, None]) * f32(0.125)).reshape(-1, 64))
    out = {"z": dz.reshape(N, T, 64), "c": dc, "W": dW, "b": db}
    assert all(v.dtype == f32 for v in out.values())
    return out
