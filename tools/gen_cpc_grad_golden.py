#!/usr/bin/env python3
"""Generate tests/golden/cpc_grad_pins.npz from the REFERENCE's own ``CPCLoss`` and autograd (runs in the build container only).

For every case of tests/cpc_grad_ref.py -- the four recorded fixtures, the cases of tests/cpc_cases.py and ``long`` -- the
reference's ``CPCLoss`` runs in fp32 and as ``.double()`` with the case's draws replayed through ``gen_cpc_golden.Tap`` (raw
sequence draw r = (seq - t) mod L), followed by ``loss.backward()``.  Per case and tensor (z, c, W, b; W and b are the first K
predictors' gradients stacked, the other K stay ``None``) the file holds DATA only:

    <case>_<tensor>_e_ref     max |G_ref32 - G_ref64|: the reference's own fp32 error, the yardstick of the judge
    <case>_<tensor>_max       max |G_ref64|
    <case>_<tensor>_sums      [sum G_ref64, sum G_ref64^2]
    <case>_<tensor>_samples   G_ref64 at the 64 positions ``grad_judge.sample_positions`` draws from ``cpc_grad_ref.POSITIONS``
    <case>_loss64             the float64 loss

Usage:  python tools/gen_cpc_grad_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gen_golden import GOLD, import_reference  # noqa: E402
from gen_cpc_golden import MAX_BYTES, Tap  # noqa: E402


def reference_grads(model, g, double):
    """The reference's loss and gradients on case ``g`` with its draws replayed."""
    cpc = model.CPCLoss(model.ConfCPC(g["n_pred"], g["Spk"], g["Utt"], g["Neg"], 64, g["c_dim"]))
    cpc.load_state_dict(g["sd"])
    z, c = g["z"].clone(), g["c"].clone()
    if double:
        cpc, z, c = cpc.double(), z.double(), c.double()
    z.requires_grad_(True)
    c.requires_grad_(True)
    raw = []
    for k in range(g["K"]):
        raw += [g["utt"][k].clone(), torch.remainder(g["seq"][k] - torch.arange(g["L"]), g["L"])]
    with Tap(raw) as tap:
        loss, _ = cpc(z, c)
    assert not tap.replay
    loss.backward()
    K = g["K"]
    assert all(p.weight.grad is None and p.bias.grad is None for p in cpc.predictors[K:])
    return {"z": z.grad.numpy(), "c": c.grad.numpy(), "W": torch.stack([p.weight.grad for p in cpc.predictors[:K]]).numpy(),
            "b": torch.stack([p.bias.grad for p in cpc.predictors[:K]]).numpy(), "loss": float(loss.detach())}


def main():
    import cpc_grad_ref as R
    import grad_judge
    torch.set_num_threads(1)
    model = import_reference()
    print("reference imported from", model.__file__, "| torch", torch.__version__)
    out = {}
    for name in R.ALL_CASES:
        g = R.load(name)
        r32, r64 = reference_grads(model, g, False), reference_grads(model, g, True)
        mine = R.grads64(name)
        out[f"{name}_loss64"] = np.array(r64["loss"])
        out.update(grad_judge.pin_entries(name, r64, r32, R.POSITIONS, R.TENSORS))
        line = [f"{name}: loss64 {r64['loss']:.9f}"]
        for k in R.TENSORS:
            assert r32[k].dtype == np.float32 and r64[k].dtype == np.float64
            e_ref, top = float(out[f"{name}_{k}_e_ref"]), float(out[f"{name}_{k}_max"])
            line.append(f"d{k}: e_ref {e_ref:.3g} ({e_ref / top:.3g} of max|G| = {top:.3g}), restatement differs by "
                        f"{np.abs(mine[k] - r64[k]).max():.3g}")
        print("  ".join(line))
    path = os.path.join(GOLD, "cpc_grad_pins.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < MAX_BYTES, os.path.getsize(path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
