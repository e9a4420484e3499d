#!/usr/bin/env python3
"""HIP-event times and memory of vocoder scoring: (a) ``Vocoder.nll`` (the fused head of csrc/nll.hip after every chunk of the
teacher-forced scan) against (b) ``Vocoder.forward`` + ``F.cross_entropy`` on the GPU -- what a user had to write before, with
the (B, T_s, 256) energies in memory.

    python tools/vocoder_score_times.py [--out profiles/vocoder_score_times.txt] [--windows 10] [--window-ms 200]

Both variants are warmed up; a window is as many back-to-back calls as fill ``--window-ms`` (at least one); the variants take
turns window by window inside one process; the table gives the median, minimum and maximum over the windows.  Both calls
synchronise their stream (``check()``), as a user's call does.  Memory: ``torch.cuda.max_memory_allocated`` across one call (the
tensors torch allocates: inputs copies, outputs, the energies and F.cross_entropy's temporaries) and the handle's own
``workspace_bytes()`` after it, each variant on a fresh handle.  ``--resources`` appends tools/kernel_resources.py's lines for
csrc/nll.hip (compiles the file).
"""
import argparse
import os
import subprocess
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vectorquantizedcpc_amd as V  # noqa: E402
from timing import measure  # noqa: E402
from vectorquantizedcpc_amd import synth  # noqa: E402

SHAPES = {"training shape (32, 5119)": (32, 5120, 16), "32 whole utterances of 32 000 samples": (32, 32000, 100)}
FLOP_PER_SAMPLE = 2 * (896 * 256 + 256 * 256)


def fresh_vocoder(dev):
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    return voc.to(dev).eval()


def memory_of(fn, dev):
    """(peak bytes torch allocated across one call of fn(voc) above what was allocated before it, workspace_bytes() after)."""
    voc = fresh_vocoder(dev)
    voc.workspace_bytes()                                    # builds the handle: its weight copies are not counted below
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn(voc)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before, voc.workspace_bytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"Vocoder scoring, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, "
             "variants alternated", f"device: {torch.cuda.get_device_name(0)}"]
    for label, (B, L, Tc) in SHAPES.items():
        audio = synth.randint("score_times/a", (B, L), 256).to(dev)
        z = synth.randint("score_times/z", (B, Tc), 512).to(dev)
        spk = synth.randint("score_times/s", (B,), 102).to(dev)

        def fused(voc):
            return voc.nll(audio, z, spk).loss

        def composed(voc):
            return F.cross_entropy(voc(audio[:, :-1], z, spk).transpose(1, 2), audio[:, 1:])

        voc = fresh_vocoder(dev)
        la, lb = float(fused(voc)), float(composed(voc))
        assert abs(la - lb) < 1e-4, (la, lb)
        r = measure({"(a) Vocoder.nll": lambda: fused(voc), "(b) forward + F.cross_entropy": lambda: composed(voc)},
                    args.windows, args.window_ms, probe=1, min_reps=1)
        flop = B * (L - 1) * FLOP_PER_SAMPLE
        lines.append(f"\n{label}: B {B}, L {L}, Tc {Tc}; head {flop / 1e9:.1f} GFLOP; loss (a) {la:.6f} (b) {lb:.6f}")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:32s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {reps} calls / window")
        a, b = r["(a) Vocoder.nll"][0], r["(b) forward + F.cross_entropy"][0]
        lines.append(f"  (b) / (a) = {b / a:.3f}x   ((a) {'<=' if a <= b else '>'} (b))")
        del voc
        for name, fn in (("(a) Vocoder.nll", fused), ("(b) forward + F.cross_entropy", composed)):
            peak, ws = memory_of(fn, dev)
            lines.append(f"  {name:32s} torch peak {peak / 1e6:10.2f} MB, workspace_bytes {ws / 1e6:8.2f} MB")
    if args.resources:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                              os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", "nll.hip")], capture_output=True, text=True)
        lines.append("\nkernel resources (tools/kernel_resources.py vectorquantizedcpc_amd/csrc/nll.hip):")
        lines += ["  " + l for l in res.stdout.splitlines()]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
