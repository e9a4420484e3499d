#!/usr/bin/env python3
"""Streaming decode latency and cost: Vocoder.generate_stream against one generate() call on the same input.

    python tools/stream_latency.py [OUT.txt]

For B in {1, 32} utterances of 10 s (Tc = 100 codes, 32 000 samples) and chunks of 1 600, 3 200 and 16 000 samples: the time from
generate_stream() to the first chunk on the host, the whole streamed wall time (every chunk taken to the host as it comes)
against generate() + one copy to the host, and the per-chunk overhead (streamed - one-shot) / chunks.  Best of 3 (wall clock
around synchronised calls).  The prenet alone (Vocoder.condition) is timed too: the first chunk cannot come before it.
Where a stream's extra time goes: `open` = generate_stream() until its work is done (prenet, conditioning projection, the
stream's buffers); `loop+` = the chunks' decode loops (HIP events, vqcpc_vocoder_last_timing) summed, minus the one-shot loop;
the rest of (streamed - one-shot) is per-chunk host work: launches, copies, the synchronisation and check of every chunk.
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vectorquantizedcpc_amd as V  # noqa: E402
from vectorquantizedcpc_amd import synth  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def main():
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(synth.vocoder_state_dict())
    voc = voc.cuda().eval()
    lines = ["# tools/stream_latency.py: ms, best of 3; 10 s utterances (32 000 samples); every chunk copied to the host",
             f"# {torch.cuda.get_device_name(0)}",
             f"{'B':>3} {'chunk':>6} {'chunks':>6} {'prenet':>8} {'first':>8} {'streamed':>9} {'one-shot':>9} {'ratio':>6} "
             f"{'per-chunk':>9} {'open':>6} {'loop+':>6} path"]
    for B in (1, 32):
        z = synth.randint(f"lat/z{B}", (B, 100), 512).cuda()
        spk = synth.randint(f"lat/s{B}", (B,), 102).cuda()
        voc.generate(z, spk, seed=1, utt_base=0)                           # warm-up: graphs, buffers
        pre = min(wall(lambda: voc.condition(z, spk))[0] for _ in range(3))
        one = min(wall(lambda: voc.generate(z, spk, seed=1, utt_base=0).cpu())[0] for _ in range(3))
        one_loop = voc.last_timing()[0]
        for chunk in (1600, 3200, 16000):
            best_first, best_all, n = 1e9, 1e9, 0
            best_open = min(wall(lambda: voc.generate_stream(z, spk, chunk_samples=chunk, seed=1, utt_base=0).close())[0]
                            for _ in range(3))
            loops = 0.0
            for rep in range(3 + 1):                                       # rep 0: warm-up
                torch.cuda.synchronize()
                t = time.perf_counter()
                st = voc.generate_stream(z, spk, chunk_samples=chunk, seed=1, utt_base=0)
                first = next(st).cpu()
                t_first = time.perf_counter() - t
                n, loop = 1, voc.last_timing()[0]
                for w in st:
                    w.cpu()
                    loop += voc.last_timing()[0]
                    n += 1
                t_all = time.perf_counter() - t
                del first
                if rep and t_all < best_all:
                    loops = loop
                if rep:
                    best_first, best_all = min(best_first, t_first), min(best_all, t_all)
            lines.append(f"{B:3d} {chunk:6d} {n:6d} {pre * 1e3:8.2f} {best_first * 1e3:8.2f} {best_all * 1e3:9.2f} {one * 1e3:9.2f} "
                         f"{best_all / one:6.3f} {(best_all - one) / n * 1e3:9.3f} {best_open * 1e3:6.2f} {loops - one_loop:6.2f} {voc.last_path()}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
