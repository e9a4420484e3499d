"""The signal zoo (oracle/zoo.py) and the float32 emulation of the mel kernel (oracle/mel_fp32.py) on the CPU.

This test is where the mel tolerances of tests/test_gpu_melfront_f64.py come from: per zoo signal it prints how far the
kernel's arithmetic, restated in NumPy float32, lands from the float64 reference, and the share of cells the ``top_db``
clamp and the ``amin`` floor act on in the reference.  The GPU tests allow ten times the deviation
(``mel_fp32.tolerance``, evaluated on their own inputs).  Run with ``-s`` to see the table.  Measured here (2 s at 16 kHz,
default config): deviation / clamped share / floor share

    suite          1.79e-06  0.000  0.000        decay_int16    5.41e-05  0.556  0.258
    tone           1.15e-05  0.683  0.468        square         8.94e-07  0.000  0.000
    tone_silence   1.15e-05  0.827  0.723        impulse_first  8.94e-08  0.990  0.990
    tone_floor     1.40e-05  0.681  0.000        impulse_last   5.96e-08  0.990  0.990
    decay          2.14e-06  0.579  0.497        dc_rumble      6.15e-06  0.000  0.000

Bounds asserted: every deviation stays under 2e-4, the tolerance the GPU suite used before these numbers existed
(``mel_fp32.tolerance`` caps at it, so no derived tolerance is looser than the old one); the wide-range signals have at
least 30 % clamped cells in the REFERENCE, so the GPU cases built on them cannot quietly stop testing the clamp; the suite signal has none, which is
the gap those cases close."""
import numpy as np
import pytest

from oracle import mel_fp32, mel_ref, zoo

N = 32000


@pytest.mark.parametrize("name", zoo.NAMES)
def test_emulation_against_float64_and_clamped_share(name):
    x = zoo.make(name, N)
    assert x.dtype == np.float32 and x.shape == (N,) and np.array_equal(x, zoo.make(name, N))
    dev = mel_fp32.deviation(x)
    clamped, floored = mel_ref.clamp_shares(x)
    print("\nzoo %-14s fp32 deviation %.2e  tolerance %.2e  clamped %.3f  amin floor %.3f"
          % (name, dev, mel_fp32.tolerance(x), clamped, floored))
    assert dev <= 2e-4
    if name in zoo.WIDE_RANGE:
        assert clamped >= 0.30
    if name == "suite":
        assert clamped == 0.0 and floored == 0.0


def test_zoo_properties():
    assert not zoo.make("tone_silence", N)[N // 2:].any() and zoo.make("tone_silence", N)[: N // 2].any()
    q = zoo.make("decay_int16", N).astype(np.float64) * 32768.0
    assert np.array_equal(q, np.round(q)) and len(np.unique(q[-4000:])) <= 3           # int16 steps; the tail is a few codes
    assert set(np.unique(zoo.make("square", N))) == {-1.0, 1.0}
    for name, at in (("impulse_first", 0), ("impulse_last", N - 1)):
        x = zoo.make(name, N)
        assert x[at] == 1.0 and np.count_nonzero(x) == 1
    x = zoo.make("dc_rumble", N).astype(np.float64)
    assert abs(x.mean() - 0.2) < 0.02
    floor = zoo.make("tone_floor", N).astype(np.float64) - zoo.make("tone", N)
    assert 1e-5 < np.abs(floor).max() < 1e-4                                            # about -90 dB re full scale


def test_reflection_indices_equal_numpy_reflect_padding():
    """The frame kernel's reflection loop, for every length that needs more than one reflection inside a 2048 frame."""
    for L in range(2, 451):
        want = np.pad(np.arange(L), 1024, mode="reflect")
        got = mel_fp32.reflect_index(np.arange(-1024, L + 1024), L)
        assert np.array_equal(got, want), L


@pytest.mark.parametrize("conf", [
    dict(sr=22050, n_fft=1024, win=1024, hop=256), dict(n_fft=512, win=400, hop=128, n_mels=40),
    dict(n_fft=64, win=64, hop=16), dict(n_fft=64, win=32, hop=16), dict(preemph=0.0), dict(fmin=0.0)])
def test_emulation_follows_the_reference_through_other_configs(conf):
    x = zoo.make("suite", 8000, conf.get("sr", 16000))
    dev = mel_fp32.deviation(x, **conf)
    print("\nconf %s fp32 deviation %.2e" % (conf, dev))
    assert mel_fp32.wave_to_mel(x, **conf).shape == mel_ref.wave_to_mel(x, **conf).shape
    assert dev <= 2e-4


@pytest.mark.parametrize("L", [2, 3, 159, 160, 161, 199, 200, 201, 399, 400, 401, 1023, 1024, 1025])
def test_emulation_short_lengths(L):
    x = zoo.make("suite", L)
    assert mel_fp32.wave_to_mel(x).shape == mel_ref.wave_to_mel(x).shape == (80, 1 + L // 160)
    assert mel_fp32.deviation(x) <= 2e-4
