#!/usr/bin/env python3
"""Rounds of the three exchange polls of the per-XCD resident decoder (csrc/ar_xcd.hip), per wave and sample step: the h_t sweep, the
a_t poll of the fc2 waves and the candidate poll of the service waves, worker 5 of XCD 0, mean over steps 256..383.  A round that
does not find every granule it looks for is a failed round: loads that L2 answered before the data existed.

Needs a debug build with -DVQCPC_XD_POLLS (and only that), e.g.
    tools/build_variant.sh polls "-DVQCPC_XD_POLLS" && python3 tools/xcd_polls.py --lib=build/exp/polls/libvqcpc_hip.so [utterances ...]
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vectorquantizedcpc_amd import _lib  # noqa: E402

_lib.LIB_PATH = os.path.join(ROOT, "build", "exp", "polls", "libvqcpc_hip.so")
for a in sys.argv[1:]:
    if a.startswith("--lib="):
        _lib.LIB_PATH = os.path.abspath(a[6:])
import vectorquantizedcpc_amd as V  # noqa: E402
from vectorquantizedcpc_amd import synth  # noqa: E402

STEPS = 128
voc = V.Vocoder(V.ConfVocoder())
voc.load_state_dict(synth.vocoder_state_dict())
voc = voc.cuda().eval()
voc.set_option("xcd", 1)
lib = _lib.load()
lib.vqcpc_debug_xd_polls.argtypes = [C.POINTER(C.c_uint)]
buf = (C.c_uint * (12 * 3 * 2))()
for B in [int(a) for a in sys.argv[1:] if a.isdigit()] or [1, 16, 32]:
    z = synth.randint("timeline", (B, 4), 512).cuda()
    spk = torch.zeros(B, dtype=torch.long, device="cuda")
    assert lib.vqcpc_debug_xd_polls(buf) == 0          # clears what an earlier call left
    voc.generate(z, spk, seed=13)
    voc.check()
    ms, n = voc.last_timing()
    assert lib.vqcpc_debug_xd_polls(buf) == 0
    r = np.array(buf, dtype=np.float64).reshape(12, 3, 2) / STEPS
    print(f"per-XCD decoders ({os.path.relpath(_lib.LIB_PATH, ROOT)}), {B} utterance(s): {ms * 1e3 / n:.2f} us per sample step over the call; "
          f"rounds per step, failed / all, worker 5 of XCD 0")
    print("  wave   h_t sweep      a_t poll       candidate poll")
    for w in range(12):
        print(f"  {w:4d}  " + "  ".join(f"{r[w, e, 0]:5.2f} / {r[w, e, 1]:5.2f}" if r[w, e, 1] else "    -        " for e in range(3)))
    tot = r.sum(axis=0)
    print("   all  " + "  ".join(f"{tot[e, 0]:5.2f} / {tot[e, 1]:5.2f}" for e in range(3)))
