"""NumPy float32 restatement of the arithmetic of ``csrc/melfront.hip`` (TEST INFRASTRUCTURE, like the rest of oracle/).

Not a second reference: ``oracle/mel_ref.py`` (float64) stays the only one.  This module answers one question on the
CPU: how far does float32, used the way the kernel uses it, move the normalised log-mel away from float64 on a given
signal?  The GPU tests take ten times that distance as their tolerance (``tolerance``), per signal, at run time.

The kernel's steps, each rounded to float32 where the kernel rounds (it is compiled with ``-ffp-contract=off``):
peak scale ``0.999f / max|x|``; pre-emphasis ``x[i] s - a (x[i-1] s)`` on the REFLECTED index ``i`` (so the sample
before a reflected one is its left neighbour in the signal, as in ``lfilter`` followed by ``np.pad(reflect)``);
a ``win``-term windowed DFT as a float32 matrix product with the window folded into the [cos | sin] matrix;
``sqrt(re^2 + im^2)``; the float32 filterbank product; ``10 log10f(fmaxf(1e-10, a a))``; the ``top_db`` clamp against
the utterance maximum; ``/ top_db + 1``.  The order inside the two matrix products is NumPy's, not the MFMA chain's:
that difference is what the factor of ten is for.
"""
import numpy as np

from . import mel_ref

F = np.float32
CAP = 2e-4                                    # what the GPU suite allowed before this module existed: see ``tolerance``


def reflect_index(i, L):
    """The kernel's ``while (i < 0 || i >= L) { if (i < 0) i = -i; if (i >= L) i = 2 (L - 1) - i; }``, vectorised."""
    i = np.array(i, dtype=np.int64, copy=True)
    while True:
        bad = (i < 0) | (i >= L)
        if not bad.any():
            return i
        i = np.where(i < 0, -i, i)
        i = np.where(i >= L, 2 * (L - 1) - i, i)


def dft_matrix(n_fft, win):
    """(2 * nbins, win) float32: rows [w cos | -w sin] of the periodic Hann window times the DFT kernel, as the kernel builds it."""
    k = np.arange(n_fft // 2 + 1, dtype=np.int64)[:, None]
    j = np.arange(win, dtype=np.int64)[None, :]
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * j / win)
    ph = 2.0 * np.pi * ((k * j) % n_fft).astype(np.float64) / n_fft
    return np.concatenate([(w * np.cos(ph)).astype(F), (-w * np.sin(ph)).astype(F)], axis=0)


def wave_to_mel(wave, sr=16000, n_fft=2048, n_mels=80, hop=160, win=400, fmin=50.0, preemph=0.97, top_db=80.0):
    """float32 (n_mels, 1 + L // hop), computed in float32 the way the kernel does."""
    x = np.ascontiguousarray(wave, dtype=F)
    L = len(x)
    T = 1 + L // hop
    with np.errstate(divide="ignore", invalid="ignore"):
        s = F(0.999) / np.abs(x).max()
        i = reflect_index(hop * np.arange(T)[:, None] + np.arange(win)[None, :] - win // 2, L)
        xs = x * s
        prev = np.where(i > 0, F(preemph) * xs[np.maximum(i - 1, 0)], F(0.0)).astype(F)
        frames = xs[i] - prev
        spec = frames @ dft_matrix(n_fft, win).T
        nb = n_fft // 2 + 1
        re, im = spec[:, :nb], spec[:, nb:]
        mag = np.sqrt(re * re + im * im)
        a = mag @ mel_ref.mel_filterbank(sr, n_fft, n_mels, fmin).T
        l = F(10.0) * np.log10(np.fmax(F(1e-10), a * a))             # fmaxf: a NaN (silent row) takes the floor
        out = np.maximum(l, l.max() - F(top_db)) / F(top_db) + F(1.0)
    assert out.dtype == F
    return np.ascontiguousarray(out.T)


def deviation(wave, **conf):
    """max |float32 emulation - float64 reference| on the normalised log-mel of ``wave``."""
    return float(np.abs(wave_to_mel(wave, **conf).astype(np.float64) - mel_ref.wave_to_mel(wave, **conf)).max())


def tolerance(wave, **conf):
    """What a GPU result may differ from ``mel_ref`` by on ``wave``: ten times what float32 costs the emulation, and
    never more than the 2e-4 the GPU suite allowed before this module existed."""
    return min(10.0 * deviation(wave, **conf), CAP)
