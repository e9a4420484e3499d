#!/usr/bin/env python3
"""HIP-event times of the CPC gradients: ``vqcpc_cpc_grad`` asked for all four gradients, for dW / db only (a fit step), and for
each gradient alone (which launch dominates), against the forward-only ``vqcpc_cpc_score`` of the same build and against the
PyTorch eager composition of ``tools/cpc_times.py`` run forward + ``backward()`` in fp32 on the same GPU -- what a user would
otherwise run.  Work space bytes of the native call (the drop in free device memory across its first call, and the layout's own
sum) against the eager composition's peak allocation.

    python tools/cpc_grad_times.py [--out profiles/cpc_grad_times.txt] [--windows 20] [--window-ms 40]

Windows and alternation are those of ``tools/timing.py``, the table that of ``tools/cpc_times.py`` (median [min .. max] over the windows).
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vectorquantizedcpc_amd as V  # noqa: E402
from cpc_times import SHAPES, eager_cpc  # noqa: E402
from timing import measure  # noqa: E402
from vectorquantizedcpc_amd import _lib, synth  # noqa: E402


def up256(b):
    return (b + 255) & ~255


def layout_bytes(K, N, L, J, Utt, C, want_z, want_w):
    """The work space of one call as csrc/cpc_grad.hip lays it out (GW_SLAB = 1024)."""
    rows = up256(K * N * L * 64 * 4)
    total = rows
    if want_z:
        total += 2 * rows + up256(K * N * J * L * 4) + up256(K * N * (J - 1) * L * 4) + up256(K * Utt * (J - 1) * 4)
    if want_w:
        total += up256(K * ((N * L + 1023) // 1024) * 64 * (C + 16) * 4)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"CPC gradients, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}"]
    for label, (Spk, Utt, Neg, T, n_pred) in SHAPES.items():
        K, N, L, C = n_pred // 2, Spk * Utt, T - n_pred // 2, 256
        cpc = V.CPCLoss(V.ConfCPC(n_pred, Spk, Utt, Neg, 64, C))
        cpc.load_state_dict(synth.cpc_state_dict())
        cpc = cpc.to(dev).eval()
        z, c = (t.to(dev) for t in synth.cpc_inputs("times", N, T, runs=True))
        W = torch.stack([p.weight.detach() for p in cpc.predictors[:K]]).contiguous()
        b = torch.stack([p.bias.detach() for p in cpc.predictors[:K]]).contiguous()
        out = torch.empty(1 + 2 * K, device=dev)
        gz, gc, gW, gb = (torch.empty_like(t) for t in (z, c, W, b))
        h, stream = cpc._native(), _lib.current_stream()
        head = (out[0:].data_ptr(), out[1:].data_ptr(), out[1 + K:].data_ptr())

        def grad(*ptrs):
            def run():
                _lib.check(lib.vqcpc_cpc_grad(h, z.data_ptr(), c.data_ptr(), T, W.data_ptr(), b.data_ptr(), None, None, 13, 0, *head,
                                              *ptrs, stream))
            return run

        def score():
            _lib.check(lib.vqcpc_cpc_score(h, z.data_ptr(), c.data_ptr(), T, None, None, 13, 0, *head, None, None, stream))

        leaves = [t.clone().requires_grad_(True) for t in (z, c)] + [p.weight for p in cpc.predictors[:K]] + [p.bias for p in cpc.predictors[:K]]

        def eager():
            for t in leaves:
                t.grad = None
            loss, _ = eager_cpc(leaves[2:2 + K], leaves[2 + K:], leaves[0], leaves[1], Spk, Utt, Neg, K)
            loss.backward()

        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        grad(gz.data_ptr(), gc.data_ptr(), gW.data_ptr(), gb.data_ptr())()
        torch.cuda.synchronize()
        native_ws = free0 - torch.cuda.mem_get_info()[0]
        score()
        fwd = float(out[0])
        grad(None, None, gW.data_ptr(), gb.data_ptr())()
        assert float(out[0]) == fwd                                       # the grad call's loss is the score call's
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        eager()
        torch.cuda.synchronize()
        eager_peak = torch.cuda.max_memory_allocated() - base
        r = measure({"grad: dz, dc, dW, db": grad(gz.data_ptr(), gc.data_ptr(), gW.data_ptr(), gb.data_ptr()),
                     "grad: dW, db (a fit step)": grad(None, None, gW.data_ptr(), gb.data_ptr()),
                     "grad: dz alone": grad(gz.data_ptr(), None, None, None),
                     "grad: dc alone": grad(None, gc.data_ptr(), None, None),
                     "grad: nothing asked (forward + dWc tile)": grad(None, None, None, None),
                     "score: forward only": score,
                     "PyTorch eager forward + backward": eager}, args.windows, args.window_ms)
        lines.append(f"\n{label}: Spk x Utt = {Spk} x {Utt}, Neg {Neg}, T {T}, K {K}, C {C}")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:42s} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window")
        full, fit, fwd_ms, eg = (r[k][0] for k in ("grad: dz, dc, dW, db", "grad: dW, db (a fit step)", "score: forward only",
                                                   "PyTorch eager forward + backward"))
        tile = r["grad: nothing asked (forward + dWc tile)"][0]
        parts = {"forward + dWc tile": tile, "dW, db": fit - tile, "dz": r["grad: dz alone"][0] - tile, "dc": r["grad: dc alone"][0] - tile}
        top = max(parts, key=parts.get)
        lines.append(f"  eager / grad (all four) = {eg / full:.2f}x, eager / grad (dW, db) = {eg / fit:.2f}x; "
                     f"grad (all four) / score = {full / fwd_ms:.2f}x, grad (dW, db) / score = {fit / fwd_ms:.2f}x")
        lines.append("  by pass (differences of the medians above): " + ", ".join(f"{k} {v:.4f} ms" for k, v in parts.items())
                     + f" -- the largest is {top}")
        lines.append(f"  work space: native {native_ws / 2**20:.1f} MiB taken from the device at the first call (layout: "
                     f"{layout_bytes(K, N, L, 1 + Neg, Utt, C, True, True) / 2**20:.1f} MiB all four, "
                     f"{layout_bytes(K, N, L, 1 + Neg, Utt, C, False, True) / 2**20:.1f} MiB dW, db only); "
                     f"eager forward + backward peak {eager_peak / 2**20:.1f} MiB above its inputs")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
