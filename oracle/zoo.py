"""A small zoo of deterministic test waveforms for the wav front end (TEST INFRASTRUCTURE, like the rest of oracle/).

The front-end tests used one kind of input: a few sines on a broadband noise floor.  On that input no mel cell is ever
clamped by ``top_db``, no filter state outlives its block and no sample is exactly zero.  The signals below are what real
files contain besides: pure tones, digital silence, decays over more than 80 dB, int16 steps, full-scale edges, single
samples, DC and rumble.  Everything random comes from ``synth.uniform01`` so that every machine builds the same bits.

``make(name, n, sr)`` -> float32 (n,).  ``NAMES`` lists all; ``WIDE_RANGE`` are the ones whose float64 log-mel spans
more than ``top_db`` (at least 30 % of the cells clamped: asserted on the reference in ``tests/test_zoo_cpu.py``).
"""
import numpy as np

from vectorquantizedcpc_amd import synth

NAMES = ("suite", "tone", "tone_silence", "tone_floor", "decay", "decay_int16", "square", "impulse_first", "impulse_last",
         "dc_rumble")
WIDE_RANGE = ("tone", "tone_silence", "tone_floor", "decay", "decay_int16")


def _noise(name, n):
    return synth.uniform01("zoo/" + name, n) - 0.5


def _voiced(t, f0=120.0):
    """A buzz with a falling harmonic spectrum: 24 harmonics of f0 with 1/h amplitudes and fixed phases."""
    h = np.arange(1, 25)
    return (np.sin(2 * np.pi * f0 * h[:, None] * t[None, :] + 0.7 * h[:, None] ** 2) / h[:, None]).sum(0) / 2.5


def make(name: str, n: int, sr: int = 16000) -> np.ndarray:
    t = np.arange(n) / float(sr)
    if name == "suite":                                   # the kind tests/test_gpu_melfront.py uses: sines on a noise floor
        x = 0.3 * np.sin(2 * np.pi * 150 * t) + 0.12 * np.sin(2 * np.pi * 1850 * t + 1.0) + 0.06 * _noise(name, n)
    elif name == "tone":
        x = 0.5 * np.sin(2 * np.pi * 440 * t)
    elif name == "tone_silence":                          # the second half is exact zeros, as after a digital fade
        x = 0.5 * np.sin(2 * np.pi * 440 * t)
        x[n // 2:] = 0.0
    elif name == "tone_floor":                            # -90 dB re full scale: under the clamp, above the amin floor
        x = 0.5 * np.sin(2 * np.pi * 440 * t) + 2.0 * 10 ** (-90 / 20) * _noise(name, n)
    elif name in ("decay", "decay_int16"):                # 60 dB per second: passes the 80 dB clamp after 1.3 s
        x = 0.8 * _voiced(t) * 10 ** (-60 * t / 20)
        if name == "decay_int16":
            x = np.round(x * 32767.0) / 32768.0
    elif name == "square":                                # full scale, edges between samples
        x = np.where(np.floor(2 * 250 * t) % 2 == 0, 1.0, -1.0)
    elif name == "impulse_first":
        x = np.zeros(n)
        x[0] = 1.0
    elif name == "impulse_last":
        x = np.zeros(n)
        x[n - 1] = 1.0
    elif name == "dc_rumble":                             # DC + 20 Hz + speech band
        x = (0.2 + 0.3 * np.sin(2 * np.pi * 20 * t) + 0.1 * np.sin(2 * np.pi * 180 * t + 0.4)
             + 0.05 * np.sin(2 * np.pi * 2310 * t) + 0.02 * _noise(name, n))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, dtype=np.float32)
