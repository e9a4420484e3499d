#!/usr/bin/env python3
"""HIP-event times of the optimizer step: one Adam update of the full encoder + predictors parameter set (what ``fit_encoder``
steps) and of the full vocoder set (what ``fit_vocoder(train=all three parts)`` steps), by three optimizers on the same GPU and the
same tensors --

* ``optim.Adam``: one ``vqcpc_adam_step`` call (``csrc/optim.hip``), one launch;
* ``torch.optim.Adam(params, lr=lr)``, as the fits construct it by default -- the figure to beat;
* ``torch.optim.Adam(params, lr=lr, fused=True)``, torch's own multi-tensor kernel, reported whichever way it falls --

then one whole ``fit_encoder`` step at the train shape (8 speakers x 8 utterances x 140 frames: forward, CPC, backward, update) with
each of the three.

    python tools/adam_times.py [--out profiles/adam_times.txt] [--windows 20] [--window-ms 40]

An update is timed as the fits run it: ``opt.step()`` back to back on one stream, events around a window, so the figure holds the
host's share (Python, launches) wherever the host is the slower side.  Windows and alternation are those of ``tools/timing.py``
(median [min .. max] over the windows, every variant warmed up).  The only speed condition of this step: the median of
``optim.Adam`` over a model is no greater than that of today's default ``torch.optim.Adam`` on the same tensors; the last line of
each table says whether it holds.
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
from vectorquantizedcpc_amd import optim, synth  # noqa: E402

OPTIMIZERS = {"optim.Adam (vqcpc_adam_step)": lambda ps, lr: optim.Adam(ps, lr=lr),
              "torch.optim.Adam (the fits' default)": lambda ps, lr: torch.optim.Adam(ps, lr=lr),
              "torch.optim.Adam(fused=True)": lambda ps, lr: torch.optim.Adam(ps, lr=lr, fused=True)}


def encoder_and_cpc(dev, S=8, U=8):
    sd = synth.encoder_state_dict(ln_affine="random", codebook="data")
    sd["codebook.ema_count"] = torch.full_like(sd["codebook.ema_count"], 50.0)      # a trained codebook's state
    sd["codebook.ema_weight"] = sd["codebook.embedding"] * 50.0
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(sd)
    cpc = V.CPCLoss(V.ConfCPC(12, S, U, 17, 64, 256))
    cpc.load_state_dict(synth.cpc_state_dict())
    return enc.to(dev).train(), cpc.to(dev)


def encoder_params(enc, cpc):
    return (list(enc.conv.parameters()) + list(enc.encoder.parameters()) + list(enc.rnn.parameters()) +
            [p for m in cpc.predictors[:cpc.n_prediction_steps] for p in m.parameters()])


def update_table(label, params, args, lines):
    """One update of copies of ``params`` with fixed gradients, by each optimizer."""
    steps = {}
    for name, make in OPTIMIZERS.items():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for i, p in enumerate(ps):
            p.grad = synth._uniform(f"adam_times/g{i}", tuple(p.shape), 1e-3, synth.SEED).to(p.device)
        steps[name] = make(ps, 1e-6).step
    r = measure(steps, args.windows, args.window_ms)
    n, elems = len(params), sum(p.numel() for p in params)
    lines.append(f"\n{label}: {n} tensors, {elems} elements, {28 * elems / 1e6:.1f} MB read and written per update")
    for name, (med, lo, hi, reps) in r.items():
        lines.append(f"  {name:40s} {med * 1e3:9.1f} us  [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]  {reps} calls / window")
    ours, default, fused = (r[k][0] for k in r)
    lines.append(f"  optim.Adam / default torch Adam = {ours / default:.3f}, / fused torch Adam = {ours / fused:.3f}; "
                 f"{28 * elems / (ours * 1e-3) / 1e12:.2f} TB/s at optim.Adam's median")
    lines.append(f"  speed condition (optim.Adam <= default torch Adam): {'holds' if ours <= default else 'DOES NOT HOLD'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"The optimizer step, HIP-event time per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, variants alternated",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}"]
    enc, cpc = encoder_and_cpc(dev)
    update_table("encoder + the 6 predictors the loss reads (fit_encoder's parameters)", encoder_params(enc, cpc), args, lines)
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    voc = voc.to(dev)
    update_table("vocoder (fit_vocoder's parameters, all three parts)", [p for part in V.Vocoder.TRAIN_PARTS for p in voc._part_params(part)], args, lines)

    # the whole fit_encoder step at the train shape, once per optimizer, each on a model of its own
    S, U, T = 8, 8, 140
    mel = synth.mel("adam_times", S * U, T).to(dev)
    steps = {}
    for name, make in OPTIMIZERS.items():
        e, c = encoder_and_cpc(dev, S, U)
        opt = make(encoder_params(e, c), 1e-6)

        def step(e=e, c=c, opt=opt):
            opt.zero_grad(set_to_none=True)
            z, ctx, vq_loss, _ = e.forward_differentiable(mel, adapt_codebook=True)
            loss, _ = c(z, ctx, seed=13, stream_id=0, differentiable=True)
            (loss + vq_loss).backward()
            opt.step()

        step()
        steps[name] = step
    r = measure(steps, args.windows, args.window_ms)
    lines.append(f"\none fit_encoder step (forward, CPC, backward, update), {S} speakers x {U} utterances x {T} frames")
    for name, (med, lo, hi, reps) in r.items():
        lines.append(f"  {name:40s} {med:9.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window")
    ours, default, fused = (r[k][0] for k in r)
    lines.append(f"  the default torch Adam step is {default - ours:+.4f} ms = {100.0 * (default - ours) / default:+.1f} % of its fit step longer than "
                 f"optim.Adam's; fused torch Adam {fused - ours:+.4f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
