"""oracle/resample_ref.py: the float64 restatement of librosa's kaiser_best resampling (convert.py:54-56 ->
librosa.load(sr=...)).  PARITY UNPINNED: resampy / librosa are absent and the reference holds no audio fixture, so the
restatement is checked through properties of the published algorithm: output length, identity at equal rates,
pass-band fidelity of tones, rejection above the new Nyquist, and agreement with scipy's polyphase resampler
(a different Kaiser-windowed sinc design) inside the common pass band."""
import numpy as np
import pytest
import scipy.signal as ss

import resample_cases
from oracle import resample_ref as R


def tone(f, sr, n):
    return np.sin(2 * np.pi * f * np.arange(n) / sr)


def test_lengths_and_identity():
    x = tone(300, 44100, 4411)
    assert R.resample(x, 44100, 16000).shape == (int(np.ceil(4411 * 16000 / 44100)),)
    assert R.resample(x, 8000, 16000).shape == (8822,)
    assert np.array_equal(R.resample(x, 16000, 16000), x)
    w, nb = R.sinc_window(**R.KAISER_BEST)
    assert nb == 512 and w.shape == (64 * 512 + 1,) and abs(w[0] - R.KAISER_BEST["rolloff"]) < 1e-15 and abs(w[-1]) < 1e-7


def test_passband_tones_and_stopband():
    for sr0, sr1, tol in ((44100, 16000, 6e-3), (48000, 16000, 6e-3), (22050, 16000, 6e-3), (8000, 16000, 1e-5)):
        n = sr0 // 8
        for f in (200.0, 1000.0, 3000.0):
            y = R.resample(tone(f, sr0, n), sr0, sr1)
            want = tone(f, sr1, len(y))
            assert np.abs(y[300:-300] - want[300:-300]).max() <= tol, (sr0, sr1, f)   # resampy's integer index step
    y = R.resample(tone(12000.0, 44100, 6000), 44100, 16000)                            # above the new Nyquist: removed
    assert np.sqrt(np.mean(y[300:-300] ** 2)) < 1e-3


def test_close_to_scipy_polyphase_in_the_passband():
    rng = np.random.default_rng(13)
    x = ss.lfilter(*ss.butter(6, 0.2), rng.standard_normal(9600))                       # band-limited noise (< 0.2 x 24 kHz)
    y = R.resample(x, 48000, 16000)
    z = ss.resample_poly(x, 1, 3, window=("kaiser", 14.769656459379492))
    m = min(len(y), len(z))
    assert np.abs(y[300:m - 300] - z[300:m - 300]).max() <= 2e-2 * np.abs(z).max()


def test_output_clock_is_the_sequential_sum():
    for sr0, sr1 in ((44100, 16000), (22050, 32000), (8000, 16000)):
        inc, acc, want = 1.0 / (float(sr1) / float(sr0)), 0.0, []
        for _ in range(70000):
            want.append(acc)
            acc += inc
        assert np.array_equal(R.output_clock(70000, sr0, sr1), np.array(want))
    assert not np.array_equal(R.output_clock(70000, 44100, 16000), np.arange(70000) * (1.0 / (16000.0 / 44100.0)))


@pytest.mark.parametrize("case", resample_cases.cases(), ids=lambda c: c[0])
def test_oracle_agrees_with_itself_under_the_float32_rule(case):
    """The GPU rule (one float32 ulp of float32(want), or 1e-12 absolute; 99.9 % bit-equal) must measure the kernel, not the
    inputs: the float64 sum taken tap by tap outwards, tap by tap inwards with the wings swapped, and by np.dot round to the
    same float32 on every case the GPU test runs."""
    label, sr0, sr1, x = case
    want = R.resample(x, sr0, sr1)
    idx = np.arange(len(want))
    for order in ("forward", "reverse"):
        ok, share, ulp, _ = R.compare_rounded(R.resample_at(x, sr0, sr1, idx, order).astype(np.float32), want)
        assert ok and share >= 0.999, (label, order, share, ulp)
    assert np.abs(R.resample_at(x, sr0, sr1, idx) - want).max() <= 1e-14 * max(1.0, np.abs(x).max())


def test_compare_rounded_rejects_what_it_should():
    want = np.linspace(-1, 1, 4001)
    w32 = want.astype(np.float32)
    assert R.compare_rounded(w32, want) == (True, 1.0, 0, 1.0)
    two = w32.copy()
    two[7] = np.nextafter(np.nextafter(two[7], np.float32(2)), np.float32(2))
    assert R.compare_rounded(two, want)[0] is False and R.compare_rounded(two, want)[2] == 2
    one = np.nextafter(w32, np.float32(2))                      # one ulp everywhere: inside the rule, but nothing bit-equal
    assert R.compare_rounded(one, want)[0] is True and R.compare_rounded(one, want)[1] < 0.001
    assert R.compare_rounded(np.array([1e-13], np.float32), np.array([-1e-13])) == (True, 1.0, 0, 0.0)
    assert R.compare_rounded(np.array([np.nan], np.float32), np.array([0.5]))[0] is False
