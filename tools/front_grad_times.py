#!/usr/bin/env python3
"""HIP-event times of the front end's gradients: ``vqcpc_encoder_front_fwd`` (the forward that keeps its rows),
``vqcpc_encoder_front_bwd`` asked for all 17 gradients, for the LayerNorm gradients alone (the whole chain of input-gradient
products, no weight product) and for the out layer alone, next to the plain ``vqcpc_encoder_stage(10)`` of the same build and one
whole ``driver.fit_encoder`` step (``forward_differentiable`` + ``CPCLoss`` + ``backward()`` + Adam) -- against the same modules'
forward + ``backward()`` in PyTorch eager fp32 on the same GPU, what a user would otherwise run.  Work space of the native calls
(``vqcpc_encoder_workspace_bytes`` after them, plus the caller's ``saved`` buffer) against the eager modules' peak allocation.

    python tools/front_grad_times.py [--out profiles/front_grad_times.txt] [--windows 20] [--window-ms 40]

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

SHAPES = {"train_shape 64 x 128 frames": (8, 8, 128), "8x larger 512 x 128 frames": (64, 8, 128)}     # speakers, utterances, mel frames
PEAK = 157.3e12                                          # fp32 MFMA, FLOP/s
LN_KEYS = tuple(range(1, 11))                            # positions of the ten LayerNorm tensors among the 17


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"Front-end gradients, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}"]
    for label, (S, U, T) in SHAPES.items():
        B, To = S * U, T // 2
        R = B * To
        flop = 2.0 * R * 512 * (4 * 80 + 4 * 512 + 64)               # the forward's multiply-adds; the backward does twice that
        sd = synth.encoder_state_dict(ln_affine="random", codebook="data")
        sd["codebook.ema_count"] = torch.full_like(sd["codebook.ema_count"], 50.0)      # a trained codebook's state
        sd["codebook.ema_weight"] = sd["codebook.embedding"] * 50.0
        enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
        enc.load_state_dict(sd)
        enc = enc.to(dev).train()
        cpc = V.CPCLoss(V.ConfCPC(12, S, U, 17, 64, 256))
        cpc.load_state_dict(synth.cpc_state_dict())
        cpc = cpc.to(dev)
        mel = synth.mel("times", B, T).to(dev)
        G = synth._uniform("times/G", (B, To, 64), 1.0, synth.SEED).to(dev)
        ws = [p.detach().contiguous() for p in enc._front_params(dev)]
        z_pre, saved = enc._front_fwd(mel, ws)
        enc._front_bwd(mel, saved, G, ws)
        torch.cuda.synchronize()
        native_ws, saved_bytes = enc.workspace_bytes(), saved.numel() * 4

        conv = torch.nn.Conv1d(80, 512, 4, 2, 1, bias=False).to(dev)
        conv.load_state_dict(enc.conv.state_dict())
        block = lambda: [torch.nn.Linear(512, 512, bias=False), torch.nn.LayerNorm(512), torch.nn.ReLU(True)]
        seq = torch.nn.Sequential(torch.nn.LayerNorm(512), torch.nn.ReLU(True), *[m for _ in range(4) for m in block()],
                                  torch.nn.Linear(512, 64)).to(dev)             # model.py:46-55
        seq.load_state_dict(enc.encoder.state_dict())
        params = list(conv.parameters()) + list(seq.parameters())

        def eager():
            for p in params:
                p.grad = None
            seq(conv(mel).transpose(1, 2)).backward(G)

        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        eager()
        torch.cuda.synchronize()
        eager_peak = torch.cuda.max_memory_allocated() - base
        assert float((seq(conv(mel).transpose(1, 2)).detach() - z_pre).abs().max()) < 1e-4      # the same network

        K = cpc.n_prediction_steps
        opt = torch.optim.Adam(list(enc.conv.parameters()) + list(enc.encoder.parameters()) + list(enc.rnn.parameters()) +
                               [p for m in cpc.predictors[:K] for p in m.parameters()], lr=1e-6)

        def step():
            opt.zero_grad(set_to_none=True)
            z, c, vq_loss, _ = enc.forward_differentiable(mel, adapt_codebook=True)
            loss, _ = cpc(z, c, seed=13, stream_id=0, differentiable=True)
            (loss + vq_loss).backward()
            opt.step()

        want = lambda keys: tuple(i in keys for i in range(17))
        r = measure({"front_fwd (keeps its rows)": lambda: enc._front_fwd(mel, ws),
                     "front_bwd: all 17 gradients": lambda: enc._front_bwd(mel, saved, G, ws),
                     "front_bwd: LayerNorm gradients only": lambda: enc._front_bwd(mel, saved, G, ws, want(LN_KEYS)),
                     "front_bwd: out layer only": lambda: enc._front_bwd(mel, saved, G, ws, want((15, 16))),
                     "stage 10: forward only": lambda: enc.stage(mel, 10),
                     "fit_encoder step (fwd, CPC, bwd, Adam)": step,
                     "torch eager front end forward + backward": eager}, args.windows, args.window_ms)
        lines.append(f"\n{label}: B {B}, T {T}, {R} rows; forward {flop / 1e9:.2f} GFLOP, backward twice that")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:42s} {med:8.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window")
        fwd, bwd, ln, top, st, stp, eg = (r[k][0] for k in r)
        lines.append(f"  fraction of the fp32 MFMA peak: front_fwd {flop / (fwd * 1e-3) / PEAK:.3f}, stage 10 {flop / (st * 1e-3) / PEAK:.3f}, "
                     f"front_bwd {2 * flop / (bwd * 1e-3) / PEAK:.3f}")
        lines.append(f"  front_bwd by parts: LayerNorm backward + input-gradient products {ln:.4f} ms, the weight products and their "
                     f"reducers {bwd - ln:.4f} ms (out layer alone {top:.4f} ms)")
        lines.append(f"  eager / (front_fwd + front_bwd) = {eg / (fwd + bwd):.2f}x; the whole step takes {stp:.4f} ms, {stp / eg:.2f}x the eager front end alone")
        lines.append(f"  work space: native {native_ws / 2**20:.1f} MiB on the handle + {saved_bytes / 2**20:.1f} MiB saved by the caller; "
                     f"eager forward + backward peak {eager_peak / 2**20:.1f} MiB above its inputs")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
