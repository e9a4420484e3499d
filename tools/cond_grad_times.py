#!/usr/bin/env python3
"""HIP-event times of the conditioning path's gradients: ``vqcpc_vocoder_cond_fwd`` and ``vqcpc_vocoder_cond_bwd`` asked for all
eighteen gradients, at the reference's training shape (4 and 32 utterances of 16 codes) and at 32 whole utterances of 500 codes --
against the same path's forward + ``backward()`` in PyTorch eager fp32 on the same GPU (two ``nn.Embedding`` + ``nn.GRU(num_layers=2,
bidirectional=True)``), what a user would otherwise run.  Then the whole ``fit_vocoder`` step at the training shape -- forward,
backward, Adam -- with the conditioning parts frozen (``train=("ar",)``) and stepping (all three parts).

    python tools/cond_grad_times.py [--out profiles/cond_grad_times.txt] [--windows 7] [--window-ms 40]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cond_grad_times.py --trace-target 32 --trace-codes 500

``--trace-target B``: nothing is timed; one warm-up and three ``cond_fwd`` + ``cond_bwd`` pairs at B utterances of ``--trace-codes``
codes (default 16), for a kernel trace taken in a run of its own.

Windows and alternation are those of ``tools/timing.py`` (median [min .. max] over the windows).
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

SHAPES = {"4 x 16 codes": (4, 16), "32 x 16 codes (the training batch)": (32, 16), "32 x 500 codes (whole utterances)": (32, 500)}


def vocoder(dev):
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    return voc.to(dev).eval()


def trace_target(dev, B, Tc=16, pairs=3):
    voc = vocoder(dev)
    z, spk = synth.randint("cond_times/z", (B, Tc), 512).to(dev), synth.randint("cond_times/s", (B,), 102).to(dev)
    G = torch.randn(B, 2 * Tc, 256, device=dev)
    ws = voc._cond_weights(voc._cond_params(), dev)
    for _ in range(1 + pairs):
        _, saved = voc._cond_fwd(z, spk, None, ws)
        voc._cond_bwd(z, spk, None, saved, G, ws)
        torch.cuda.synchronize()
    voc.check()
    print(f"trace target: {1 + pairs} cond_fwd + cond_bwd pairs at B {B}, {2 * Tc} frames")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--trace-target", type=int, default=0, metavar="B")
    ap.add_argument("--trace-codes", type=int, default=16, metavar="Tc")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_target:
        return trace_target(dev, args.trace_target, args.trace_codes)
    lines = [f"Conditioning-path gradients, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms or 3 calls, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}"]
    voc = vocoder(dev)
    for label, (B, Tc) in SHAPES.items():
        z, spk = synth.randint("cond_times/z", (B, Tc), 512).to(dev), synth.randint("cond_times/s", (B,), 102).to(dev)
        G = torch.randn(B, 2 * Tc, 256, device=dev)
        ws = voc._cond_weights(voc._cond_params(), dev)
        cond, saved = voc._cond_fwd(z, spk, None, ws)
        voc._cond_bwd(z, spk, None, saved, G, ws)
        torch.cuda.synchronize()
        voc.check()

        ce, se = torch.nn.Embedding(512, 64).to(dev), torch.nn.Embedding(102, 64).to(dev)
        gru = torch.nn.GRU(128, 128, num_layers=2, batch_first=True, bidirectional=True).to(dev)
        ce.load_state_dict(voc.code_embedding.state_dict())
        se.load_state_dict(voc.speaker_embedding.state_dict())
        gru.load_state_dict(voc.rnnms.prenet.state_dict())
        params = [p for m in (ce, se, gru) for p in m.parameters()]

        def eager_fwd():
            x = torch.cat((ce(z).repeat_interleave(2, dim=1), se(spk)[:, None, :].expand(-1, 2 * Tc, -1)), dim=2)
            return gru(x)[0]

        def eager():
            for p in params:
                p.grad = None
            out = eager_fwd()
            (out * G).sum().backward()
            return out

        with torch.no_grad():
            assert float((eager_fwd() - cond).abs().max()) < 1e-4           # the same network
        r = measure({"cond_fwd (keeps the series and both layers' outputs)": lambda: voc._cond_fwd(z, spk, None, ws),
                     "cond_bwd: eighteen gradients": lambda: voc._cond_bwd(z, spk, None, saved, G, ws),
                     "Vocoder.condition (forward only, the handle's copies)": lambda: voc.condition(z, spk),
                     "torch eager forward + backward": eager}, args.windows, args.window_ms, probe=3, min_reps=3)
        steps = 2 * Tc
        lines.append(f"\n{label}: B {B}, {steps} frames")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:56s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {reps} calls / window")
        fwd, bwd, cnd, eg = (r[k][0] for k in r)
        lines.append(f"  per frame: cond_fwd {fwd / steps * 1e3:.2f} us, cond_bwd {bwd / steps * 1e3:.2f} us (two layers, one launch per step and layer in each)")
        lines.append(f"  eager / (cond_fwd + cond_bwd) = {eg / (fwd + bwd):.2f}x")

    # the whole fit step at the training shape
    B, L, Tc = 32, 5120, 16
    audio = synth.randint("cond_times/a", (B, L), 256).to(dev)
    z, spk = synth.randint("cond_times/z", (B, Tc), 512).to(dev), synth.randint("cond_times/s", (B,), 102).to(dev)
    steps_of = {}
    for label, train in (("train=('ar',): the conditioning path frozen", ("ar",)), ("train=('ar', 'prenet', 'embeddings')", V.Vocoder.TRAIN_PARTS)):
        v = vocoder(dev)
        opt = torch.optim.Adam([p for part in train for p in v._part_params(part)], lr=1e-5)

        def step(v=v, opt=opt, train=train):
            opt.zero_grad(set_to_none=True)
            loss = v.nll(audio, z, spk, differentiable=True, train=train).loss
            loss.backward()
            opt.step()

        step()
        steps_of[label] = step
    r = measure(steps_of, args.windows, args.window_ms, probe=3, min_reps=3)
    lines.append(f"\nthe whole fit_vocoder step (forward, backward, Adam), B {B}, {L - 1} sample steps, {2 * Tc} frames")
    for name, (med, lo, hi, reps) in r.items():
        lines.append(f"  {name:56s} {med:9.3f} ms  [{lo:.3f} .. {hi:.3f}]  {reps} calls / window")
    a, b = (r[k][0] for k in r)
    lines.append(f"  the conditioning parts add {b - a:.3f} ms = {100.0 * (b - a) / a:.1f} % of the step")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
