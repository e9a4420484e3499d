#!/usr/bin/env python3
"""Times of one codebook update (``vqcpc_encoder_vq_adapt``: VQ search + eval statistics + the EMA update of ``model.py:136-145``)
against the literal PyTorch composition of the reference on the same GPU, at 4 096 rows x 512 codes and 33 280 x 1 024.

    python tools/ema_times.py [--out profiles/ema_times.txt] [--windows 20] [--window-ms 20]

Variants, alternated window by window inside one process (HIP events, warmed up, median [min .. max] over the windows):
  hip adapt         the whole call through ``VQEmbeddingEMA.forward`` in training mode
  hip eval forward  ``VQEmbeddingEMA.forward`` in eval mode (search + statistics): adapt minus this = what the update adds
  torch 131-145     ``model.py:131-145`` as written (argmin of given distances, one_hot, embedding, the EMA update); the distances
                    of ``:126-129`` are computed once outside the timed region -- the yardstick
  torch forward     ``model.py:123-155`` as written, distances included
and the peak device memory the PyTorch composition allocates beside the work space the handle holds.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ema_ref  # noqa: E402
import vectorquantizedcpc_amd as V  # noqa: E402
from timing import measure  # noqa: E402
from vectorquantizedcpc_amd import synth  # noqa: E402

SHAPES = [(4096, 512), (33280, 1024)]


class TorchEMA:
    """The buffers and ``forward`` of the reference's module, composed from the same torch calls (``model.py:117-155``)."""

    def __init__(self, case, dev, decay=0.999, epsilon=1e-5):
        self.embedding, self.ema_count, self.ema_weight = (torch.from_numpy(case[k]).to(dev) for k in ("embedding", "ema_count", "ema_weight"))
        self.decay, self.epsilon, self.commitment_cost = decay, epsilon, 0.25

    def distances(self, x_flat):
        return torch.addmm(torch.sum(self.embedding ** 2, dim=1) + torch.sum(x_flat ** 2, dim=1, keepdim=True),
                           x_flat, self.embedding.t(), alpha=-2.0, beta=1.0)

    def update(self, x, x_flat, distances):                    # model.py:131-145
        M = self.embedding.size(0)
        indices = torch.argmin(distances.float(), dim=-1)
        encodings = F.one_hot(indices, M).float()
        quantized = F.embedding(indices, self.embedding)
        quantized = quantized.view_as(x)
        self.ema_count = self.decay * self.ema_count + (1 - self.decay) * torch.sum(encodings, dim=0)
        n = torch.sum(self.ema_count)
        self.ema_count = (self.ema_count + self.epsilon) / (n + M * self.epsilon) * n
        dw = torch.matmul(encodings.t(), x_flat)
        self.ema_weight = self.decay * self.ema_weight + (1 - self.decay) * dw
        self.embedding = self.ema_weight / self.ema_count.unsqueeze(-1)
        return quantized, encodings

    def forward(self, x):                                      # model.py:123-155
        x_flat = x.detach().reshape(-1, self.embedding.size(1))
        quantized, encodings = self.update(x, x_flat, self.distances(x_flat))
        loss = self.commitment_cost * F.mse_loss(x, quantized.detach())
        quantized = x + (quantized - x).detach()
        avg_probs = torch.mean(encodings, dim=0)
        perplexity = torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-10)))
        return quantized, loss, perplexity


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=20.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"codebook update, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, "
             "variants alternated", f"device: {torch.cuda.get_device_name(0)}"]
    for n_rows, n_emb in SHAPES:
        case = ema_ref.make_case(f"times_{n_rows}", n_emb, n_rows, "skewed", "warm")
        enc = V.Encoder(V.ConfEncoder(80, 512, n_emb, 64, 256))
        sd = synth.encoder_state_dict(n_embeddings=n_emb)
        sd.update({"codebook." + k: torch.from_numpy(case[k]) for k in ("embedding", "ema_count", "ema_weight")})
        enc.load_state_dict(sd)
        enc = enc.to(dev).eval()
        ev = V.Encoder(V.ConfEncoder(80, 512, n_emb, 64, 256))
        ev.load_state_dict(sd)
        ev = ev.to(dev).eval()
        enc.codebook.train()
        x = torch.from_numpy(case["x"]).to(dev)[None]
        ref, ref_u = TorchEMA(case, dev), TorchEMA(case, dev)
        x_flat = x.reshape(-1, 64)
        dist = ref_u.distances(x_flat)
        # one call of each from the same state: the buffers agree to the reference's own rounding
        with torch.no_grad():
            enc.codebook(x)
            ref.forward(x)
        err = [float(((a - b).abs().max() / b.abs().max())) for a, b in ((enc.codebook.ema_count, ref.ema_count),
                                                                         (enc.codebook.ema_weight, ref.ema_weight),
                                                                         (enc.codebook.embedding, ref.embedding))]
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            ref.forward(x)
        torch.cuda.synchronize()
        peak_fwd = torch.cuda.max_memory_allocated() - base
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        with torch.no_grad():
            ref_u.update(x, x_flat, dist)
        torch.cuda.synchronize()
        peak_upd = torch.cuda.max_memory_allocated() - base
        HIP, EVAL, T_UPD, T_FWD = "hip adapt (search + statistics + update)", "hip eval forward (search + statistics)", \
            "torch model.py:131-145 (distances given)", "torch model.py:123-155 (whole forward)"
        with torch.no_grad():
            r = measure({HIP: lambda: enc.codebook(x), EVAL: lambda: ev.codebook(x), T_UPD: lambda: ref_u.update(x, x_flat, dist),
                         T_FWD: lambda: ref.forward(x)}, args.windows, args.window_ms, probe=3, min_reps=1)
        lines.append(f"\n{n_rows} rows x {n_emb} codes (skewed use: {len(set(case['code'].tolist()))} codes in use, the largest owns "
                     f"{int(max(torch.bincount(torch.from_numpy(case['code'])).tolist()))} rows)")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:44s} {med:9.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window")
        lines.append(f"  update alone = adapt - eval forward (medians): {r[HIP][0] - r[EVAL][0]:.4f} ms")
        below = r[HIP][2] < r[T_UPD][1]
        lines.append(f"  hip adapt window [{r[HIP][1]:.4f} .. {r[HIP][2]:.4f}] lies {'wholly below' if below else 'NOT wholly below'} torch 131-145's "
                     f"[{r[T_UPD][1]:.4f} .. {r[T_UPD][2]:.4f}]; medians torch 131-145 / hip adapt = {r[T_UPD][0] / r[HIP][0]:.2f}x, "
                     f"torch forward / hip adapt = {r[T_FWD][0] / r[HIP][0]:.2f}x")
        lines.append(f"  device memory: handle work space {enc.workspace_bytes()} bytes (vqcpc_encoder_workspace_bytes after these calls; "
                     f"its parts before 16-byte padding: quantised rows {n_rows * 256}, int64 indices {n_rows * 8}, 16-bit indices "
                     f"{n_rows * 2}, counts {n_emb * 4}, histogram + partials {n_emb * 4 + 64 * 8 + 64}); torch peak beyond its "
                     f"inputs: {peak_upd} bytes for 131-145, {peak_fwd} for the whole forward")
        lines.append(f"  first call from the same state, hip against torch, largest difference / largest value: count {err[0]:.2e} "
                     f"weight {err[1]:.2e} embedding {err[2]:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
