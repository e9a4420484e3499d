#!/usr/bin/env python3
"""HIP-event times of the vocoder's gradients: ``vqcpc_vocoder_ar_fwd`` (the scoring scan that keeps h_t), ``vqcpc_vocoder_ar_bwd``
asked for all nine gradients and ``grad_cond``, and without ``grad_cond``, at the reference's training shape (., 5120 samples, 16
codes) -- against the same network's forward + ``backward()`` in PyTorch eager fp32 on the same GPU (``nn.Embedding`` + ``nn.GRU``
+ two ``nn.Linear`` + ``F.cross_entropy``), what a user would otherwise run.  Work space of the native calls
(``vqcpc_vocoder_workspace_bytes`` after them, plus the caller's ``saved`` buffer) against the eager modules' peak allocation.

    python tools/voc_grad_times.py [--out profiles/voc_grad_times.txt] [--windows 7] [--window-ms 40]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/voc_grad_times.py --trace-target 32

``--trace-target B``: nothing is timed; one warm-up and three ``ar_fwd`` + ``ar_bwd`` pairs at B utterances, for a kernel trace taken
in a run of its own (which launches the time of a call goes to: ``profiles/voc_grad_kernel_stats.csv``).

Windows and alternation are those of ``tools/timing.py`` (median [min .. max] over the windows); a call here takes tens to hundreds
of milliseconds, so a window is a few calls.
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

SHAPES = {"4 x 5120 samples, 16 codes": (4, 5120, 16), "32 x 5120 samples, 16 codes (the training batch)": (32, 5120, 16)}


def trace_target(dev, B, L=5120, Tc=16, pairs=3):
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    voc = voc.to(dev).eval()
    audio = synth.randint("voc_times/a", (B, L), 256).to(dev)
    z, spk = synth.randint("voc_times/z", (B, Tc), 512).to(dev), synth.randint("voc_times/s", (B,), 102).to(dev)
    call = voc._nll_call(audio, z, spk, None, None)
    ws = voc._ar_weights(voc._ar_params(), dev)
    for _ in range(1 + pairs):
        saved = voc._ar_fwd(call, ws)[4]
        voc._ar_bwd(call, saved, ws, cond_grad=True)
        torch.cuda.synchronize()
    voc.check()
    print(f"trace target: {1 + pairs} ar_fwd + ar_bwd pairs at B {B}, {L - 1} steps")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--trace-target", type=int, default=0, metavar="B")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_target:
        return trace_target(dev, args.trace_target)
    lines = [f"Vocoder gradients, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms or 3 calls, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}"]
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    voc = voc.to(dev).eval()
    for label, (B, L, Tc) in SHAPES.items():
        audio = synth.randint("voc_times/a", (B, L), 256).to(dev)
        z, spk = synth.randint("voc_times/z", (B, Tc), 512).to(dev), synth.randint("voc_times/s", (B,), 102).to(dev)
        call = voc._nll_call(audio, z, spk, None, None)
        ws = voc._ar_weights(voc._ar_params(), dev)
        nll_sum, n_scored, _, cond, saved = voc._ar_fwd(call, ws, want_cond=True)
        voc._ar_bwd(call, saved, ws, cond_grad=True)
        torch.cuda.synchronize()
        voc.check()
        native_ws, saved_bytes = voc.workspace_bytes(), saved.numel() * 4
        loss = float(nll_sum.sum() / n_scored.sum())

        ar = voc.rnnms.ar
        emb, rnn = torch.nn.Embedding(256, 256).to(dev), torch.nn.GRU(512, 896, batch_first=True).to(dev)
        fc1, fc2 = torch.nn.Linear(896, 256).to(dev), torch.nn.Linear(256, 256).to(dev)
        for dst, src in ((emb, ar.embedding), (rnn, ar.rnn), (fc1, ar.fc1), (fc2, ar.fc2)):
            dst.load_state_dict(src.state_dict())
        params = [p for m in (emb, rnn, fc1, fc2) for p in m.parameters()]
        series_c = cond.repeat_interleave(160, dim=1)[:, :L - 1].contiguous()

        def eager():
            for p in params:
                p.grad = None
            e = fc2(torch.relu(fc1(rnn(torch.cat((emb(audio[:, :-1]), series_c), dim=2))[0])))
            out = torch.nn.functional.cross_entropy(e.transpose(1, 2), audio[:, 1:])
            out.backward()
            return out

        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        eager_loss = float(eager().detach())
        torch.cuda.synchronize()
        eager_peak = torch.cuda.max_memory_allocated() - base
        assert abs(eager_loss - loss) < 1e-3, (eager_loss, loss)           # the same network

        r = measure({"ar_fwd (the scoring scan, keeps h_t)": lambda: voc._ar_fwd(call, ws),
                     "ar_bwd: nine gradients and grad_cond": lambda: voc._ar_bwd(call, saved, ws, cond_grad=True),
                     "ar_bwd: nine gradients": lambda: voc._ar_bwd(call, saved, ws),
                     "Vocoder.nll (forward only, the handle's copies)": lambda: voc.nll(audio, z, spk),
                     "torch eager forward + backward": eager}, args.windows, args.window_ms, probe=3, min_reps=3)
        steps = L - 1
        lines.append(f"\n{label}: B {B}, {steps} steps; loss {loss:.6f} (eager {eager_loss:.6f})")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:50s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {reps} calls / window")
        fwd, bwd, bwd9, nll, eg = (r[k][0] for k in r)
        lines.append(f"  per step: ar_fwd {fwd / steps * 1e3:.2f} us, ar_bwd {bwd / steps * 1e3:.2f} us (one launch per step in each)")
        lines.append(f"  eager / (ar_fwd + ar_bwd) = {eg / (fwd + bwd):.2f}x; ar_fwd / Vocoder.nll = {fwd / nll:.2f}x")
        lines.append(f"  work space: native {native_ws / 2**20:.1f} MiB on the handle + {saved_bytes / 2**20:.1f} MiB saved by the caller; "
                     f"eager forward + backward peak {eager_peak / 2**20:.1f} MiB above its inputs")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
