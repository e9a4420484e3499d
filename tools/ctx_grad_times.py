#!/usr/bin/env python3
"""HIP-event times of the context LSTM's gradients: ``vqcpc_encoder_context_fwd`` (the forward that keeps state),
``vqcpc_encoder_context_bwd`` asked for all four gradients and for the weights only (a ``fit_context`` step), next to the plain
``vqcpc_encoder_context`` of the same build, against ``torch.nn.LSTM`` forward + ``backward()`` in PyTorch eager fp32 on the same GPU
-- what a user would otherwise run.  Work space of the native calls (``vqcpc_encoder_workspace_bytes`` after them, plus the caller's
``saved`` buffer) against the eager module's peak allocation.

    python tools/ctx_grad_times.py [--out profiles/ctx_grad_times.txt] [--windows 20] [--window-ms 40]

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
from timing import measure  # noqa: E402
from vectorquantizedcpc_amd import synth  # noqa: E402

SHAPES = {"train_shape 64 x 70": (64, 70), "8x larger 512 x 70": (512, 70)}       # (B, T), z_dim 64 -> c_dim 256
NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"Context LSTM gradients, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}"]
    for label, (B, T) in SHAPES.items():
        enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
        enc.load_state_dict(synth.encoder_state_dict())
        enc = enc.to(dev).eval()
        z = synth.cpc_inputs("times", B, T, runs=True)[0].to(dev)
        G = synth.cpc_inputs("times/G", B, T, runs=True)[1].to(dev)
        ws = [getattr(enc.rnn, n).detach().contiguous() for n in NAMES]
        c, saved = enc._context_fwd(z, ws)
        enc._context_bwd(z, c, saved, G, ws[:2])
        torch.cuda.synchronize()
        native_ws, saved_bytes = enc.workspace_bytes(), saved.numel() * 4

        ref = torch.nn.LSTM(64, 256, batch_first=True).to(dev)
        ref.load_state_dict(enc.rnn.state_dict())
        zr = z.clone().requires_grad_(True)

        def eager(weights_only=False):
            def run():
                zr.grad = None
                for p in ref.parameters():
                    p.grad = None
                out = ref(z if weights_only else zr)[0]
                out.backward(G)
            return run

        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        eager()()
        torch.cuda.synchronize()
        eager_peak = torch.cuda.max_memory_allocated() - base
        assert float((ref(z)[0].detach() - c).abs().max()) < 1e-5                # the same network

        r = measure({"fwd (keeps state)": lambda: enc._context_fwd(z, ws),
                     "bwd: dz, dW_ih, dW_hh, db": lambda: enc._context_bwd(z, c, saved, G, ws[:2]),
                     "bwd: dW_ih, dW_hh, db (a fit step)": lambda: enc._context_bwd(z, c, saved, G, ws[:2], (False, True, True, True)),
                     "context: forward only": lambda: enc.context(z),
                     "torch.nn.LSTM eager forward + backward": eager(),
                     "torch.nn.LSTM eager, weights only": eager(True)}, args.windows, args.window_ms)
        lines.append(f"\n{label}: B {B}, T {T}, z_dim 64 -> c_dim 256 (one launch per step: {T} forward, {T} backward)")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:42s} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window")
        fwd, full, fit, eg, egw = (r[k][0] for k in ("fwd (keeps state)", "bwd: dz, dW_ih, dW_hh, db", "bwd: dW_ih, dW_hh, db (a fit step)",
                                                     "torch.nn.LSTM eager forward + backward", "torch.nn.LSTM eager, weights only"))
        lines.append(f"  eager / (fwd + bwd, all four) = {eg / (fwd + full):.2f}x, eager weights only / (fwd + bwd, weights only) = {egw / (fwd + fit):.2f}x; "
                     f"per step: fwd {1e3 * fwd / T:.2f} us, bwd {1e3 * fit / T:.2f} us (weights only, the products included)")
        lines.append(f"  work space: native {native_ws / 2**20:.1f} MiB on the handle + {saved_bytes / 2**20:.1f} MiB saved by the caller; "
                     f"eager forward + backward peak {eager_peak / 2**20:.1f} MiB above its inputs")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
