#!/usr/bin/env python3
"""HIP-event times of CPC scoring: ``vqcpc_cpc_score`` (negatives drawn in the kernel, and from index tensors) against a
straightforward PyTorch eager restatement of ``CPCLoss.forward`` (``model.py:191-316``) on the same GPU -- what a user would
otherwise run -- and the share of a ``score`` pass that is ``Encoder.forward`` versus ``cpc``.

    python tools/cpc_times.py [--out profiles/cpc_times.txt] [--windows 20] [--window-ms 40]

Every variant and shape is warmed up; a window is as many back-to-back calls as fill ``--window-ms``; the variants take
turns window by window inside one process, and the table gives the median, minimum and maximum over the windows.  The
resource line of the kernels (``tools/kernel_resources.py``) closes the file.
"""
import argparse
import math
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vectorquantizedcpc_amd as V  # noqa: E402
from timing import measure  # noqa: E402
from vectorquantizedcpc_amd import _lib, synth  # noqa: E402

SHAPES = {"train_shape 8x8": (8, 8, 17, 70, 12), "8x larger 32x16": (32, 16, 17, 70, 12)}


def eager_cpc(weights, biases, z, c, Spk, Utt, Neg, K):
    """model.py:191-316 in eager PyTorch (predictor, positives, within-speaker negatives, scores, cross entropy + argmax), draws from torch's device generator."""
    N, T, D = z.shape
    L = T - K
    zs = z.reshape(Spk, Utt, T, D)
    ctx = c[:, :L]
    spk = torch.arange(Spk, device=z.device).view(-1, 1, 1, 1)
    t = torch.arange(L, device=z.device)
    labels = torch.zeros(N, L, dtype=torch.long, device=z.device)
    losses, accs = [], []
    for k in range(1, K + 1):
        shift = zs[:, :, k:L + k]
        wc = torch.nn.functional.linear(ctx, weights[k - 1], biases[k - 1]).view(Spk, Utt, L, D)
        utt = torch.randint(0, Utt, (Utt, Neg), device=z.device).view(1, Utt, Neg, 1)
        seq = torch.remainder(torch.randint(1, L, (Spk, Utt, Neg, L), device=z.device) + t, L)
        rows = torch.cat((shift.unsqueeze(2), shift[spk, utt, seq]), dim=2)
        f = torch.sum(rows * wc.unsqueeze(2) / math.sqrt(D), dim=-1).view(N, Neg + 1, L)
        losses.append(torch.nn.functional.cross_entropy(f, labels))
        accs.append((f.argmax(dim=1) == labels).float().mean())
    return torch.stack(losses).mean(), torch.stack(accs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    lines = [f"CPC scoring, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}"]
    for label, (Spk, Utt, Neg, T, n_pred) in SHAPES.items():
        K, N, L = n_pred // 2, Spk * Utt, T - n_pred // 2
        cpc = V.CPCLoss(V.ConfCPC(n_pred, Spk, Utt, Neg, 64, 256))
        cpc.load_state_dict(synth.cpc_state_dict())
        cpc = cpc.to(dev).eval()
        z, c = (t.to(dev) for t in synth.cpc_inputs("times", N, T, runs=True))
        utt, seq = (t.to(dev) for t in synth.cpc_negatives(13, 0, K, Spk, Utt, Neg, L))
        ws = [p.weight.detach() for p in cpc.predictors[:K]]
        bs = [p.bias.detach() for p in cpc.predictors[:K]]
        out = torch.empty(1 + 2 * K, device=dev)
        h, stream = cpc._native(), _lib.current_stream()
        tail = (out[0:].data_ptr(), out[1:].data_ptr(), out[1 + K:].data_ptr(), None, None, stream)

        def fused_protocol():
            _lib.check(lib.vqcpc_cpc_score(h, z.data_ptr(), c.data_ptr(), T, None, None, 13, 0, *tail))

        def fused_indices():
            _lib.check(lib.vqcpc_cpc_score(h, z.data_ptr(), c.data_ptr(), T, utt.data_ptr(), seq.data_ptr(), 13, 0, *tail))

        def eager():
            with torch.no_grad():
                eager_cpc(ws, bs, z, c, Spk, Utt, Neg, K)

        with torch.no_grad():
            want, _ = eager_cpc(ws, bs, z, c, Spk, Utt, Neg, K)
        fused_protocol()
        assert abs(float(out[0]) - float(want)) < 0.2, (float(out[0]), float(want))       # same objective, different draws
        r = measure({"fused, draws in the kernel": fused_protocol, "fused, index tensors": fused_indices,
                     "PyTorch eager restatement": eager}, args.windows, args.window_ms)
        flop = N * L * K * (2 * 256 * 64 + (1 + Neg) * 2 * 64)
        lines.append(f"\n{label}: Spk x Utt = {Spk} x {Utt}, Neg {Neg}, T {T}, K {K}  ({flop / 1e9:.2f} GFLOP)")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:30s} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window  {flop / med / 1e9:8.2f} TFLOP/s")
        base = r["PyTorch eager restatement"][0]
        lines.append(f"  eager / fused (draws in the kernel) = {base / r['fused, draws in the kernel'][0]:.2f}x, "
                     f"eager / fused (index tensors) = {base / r['fused, index tensors'][0]:.2f}x")
        if label.startswith("train_shape"):
            enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
            enc.load_state_dict(synth.encoder_state_dict(ln_affine="random", codebook="data"))
            enc = enc.to(dev).eval()
            mel = synth.mel("times", N, 2 * T).to(dev)
            ze, ce, _, _ = enc(mel)
            r2 = measure({"Encoder.forward": lambda: enc(mel), "CPCLoss.forward_detailed": lambda: cpc.forward_detailed(ze, ce)},
                         args.windows, args.window_ms)
            e, s = r2["Encoder.forward"][0], r2["CPCLoss.forward_detailed"][0]
            lines.append(f"  one score batch (Python calls): Encoder.forward {e:.4f} ms ({100 * e / (e + s):.1f} %), "
                         f"CPCLoss {s:.4f} ms ({100 * s / (e + s):.1f} %)")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", "cpc.hip")], capture_output=True, text=True)
    lines.append("\nkernel resources (tools/kernel_resources.py vectorquantizedcpc_amd/csrc/cpc.hip):")
    lines += ["  " + l for l in res.stdout.splitlines()]
    rem = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-c",
                          os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", "cpc.hip"), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
    lines.append("  LDS bytes per workgroup, in the same order: " + ", ".join(re.findall(r"LDS Size \[bytes/block\]: (\d+)", rem)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
