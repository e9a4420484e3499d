#!/usr/bin/env python3
"""Host cost per call of the Python bindings: what the package adds in front of the C ABI (argument checks, the cached handle
lookup, output allocation, the ctypes call) on shapes so small that the kernels hide behind it.

    python tools/call_overhead.py [--tree DIR] [--calls 2000]

After warm-up, ``--calls`` back-to-back calls ending in one ``torch.cuda.synchronize()``, host clock, for each of
``Encoder.encode_indices`` on (1, 80, 32), ``CPCLoss.forward_detailed`` on the smallest fixture shape (``one_utt``: 1 x 1
utterances, 4 negatives, T 12, 1 step), ``Vocoder.condition`` on (1, 4) and ``wave_to_mel`` on 1 600 samples; prints us per
call.  ``--tree`` names another checkout (with its library built) whose package is measured instead of this one's, for an A/B of
two trees: run the two commands in turn, several times, and compare the medians against the spread of one tree's runs.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--calls", type=int, default=2000)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch

    import vectorquantizedcpc_amd as V
    from vectorquantizedcpc_amd import preprocess, synth

    dev = torch.device("cuda:0")
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict())
    enc = enc.to(dev).eval()
    cpc = V.CPCLoss(V.ConfCPC(2, 1, 1, 4, 64, 256))
    cpc.load_state_dict(synth.cpc_state_dict(n_prediction_steps=2))
    cpc = cpc.to(dev).eval()
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    voc = voc.to(dev).eval()

    mel = synth.mel("overhead", 1, 32).to(dev)
    z, c = (t.to(dev) for t in synth.cpc_inputs("overhead", 1, 12))
    codes = torch.tensor([[3, 1, 4, 1]], device=dev)
    spk = torch.tensor([5], device=dev)
    wave = (synth.mel("overhead/wave", 1, 20)[0].reshape(-1) - 0.5).to(dev)           # 1 600 samples in [-0.5, 0.5)
    calls = {"Encoder.encode_indices (1, 80, 32)": lambda: enc.encode_indices(mel),
             "CPCLoss.forward_detailed one_utt": lambda: cpc.forward_detailed(z, c),
             "Vocoder.condition (1, 4)": lambda: voc.condition(codes, spk),
             "wave_to_mel 1600 samples": lambda: preprocess.wave_to_mel(wave)}
    print(f"tree: {os.path.dirname(os.path.abspath(V.__file__))}   device: {torch.cuda.get_device_name(0)}   calls: {args.calls}")
    for name, fn in calls.items():
        for _ in range(200):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        print(f"{name:40s} {(time.perf_counter() - t0) / args.calls * 1e6:9.2f} us/call")


if __name__ == "__main__":
    main()
