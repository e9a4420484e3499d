"""The single-row resampler cases shared by tests/test_resample_cpu.py (the oracle agrees with itself under the float32 rule
on each) and tests/test_gpu_resample_f64.py (the kernel against the oracle on each)."""
import numpy as np

from oracle import zoo
from vectorquantizedcpc_amd import synth

RATE_PAIRS = [(44100, 16000), (48000, 16000), (22050, 16000), (8000, 16000), (16000, 22050),
              (11025, 16000), (32000, 16000), (96000, 16000), (16000, 8000), (48000, 24000)]
LENGTHS = [1, 2, 63, 64, 65, 441]                    # at 44100 -> 16000; 441 samples are exactly 160 outputs


def smooth_noise(name, n):
    """What tests/test_gpu_resample.py has always used: uniform noise through a 5-tap mean."""
    x = (synth.uniform01(name, n) * 2 - 1).astype(np.float32)
    return np.convolve(x, np.ones(5) / 5, mode="same").astype(np.float32)


def cases():
    """-> list of (label, sr_in, sr_out, float32 signal)."""
    out = [("noise %d->%d" % p, p[0], p[1], smooth_noise("rs/%d" % p[0] if p in RATE_PAIRS[:5] else "rs/%d/%d" % p, 3000))
           for p in RATE_PAIRS]
    out += [("length %d" % n, 44100, 16000, smooth_noise("rs/len%d" % n, n)) for n in LENGTHS]
    for name in ("impulse_first", "impulse_last", "square"):
        out += [("%s %d->%d" % (name, a, b), a, b, zoo.make(name, 3000, a)) for a, b in ((44100, 16000), (8000, 16000))]
    return out
