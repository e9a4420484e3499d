"""-m gpu: csrc/loudness.hip against the float64 oracle beyond 16 kHz speech-like input.

Block energies at the existing 1e-10 relative bound (both sides float64; the kernel cuts the serial filter into 128-sample
chunks joined by a transition scan, scipy runs it serially) and LUFS at the existing 1e-9 dB: at 8, 22.05, 44.1, 48 and
96 kHz, where the high-pass poles move as close as 0.0012 to the unit circle; on DC + 20 Hz + speech band; over ten
minutes.  Next to every observed figure the test prints how far scipy's own float64 filter moves when the same signal is
filtered in two halves with carried state: that is the size of a legitimate difference between two float64 evaluations.
The block count (``np.round``: half to even) for every length from one block to 2.5 s at 16, 22.05 and 44.1 kHz; lengths
and a step at the 128-sample chunk edges; batches wider than the 64-thread scan and gate workgroups; one fully gated row
among normal ones; poison behind ``lengths``; the relative gate 0.01 LU from a block.

Observed on MI355X (max relative block error / |LUFS difference|; scipy's split-state run moved nothing: its carried
state is exact, so the fallback bound the 1e-10 cases could have taken was never needed):
    dc_rumble   8 k 1.6e-14 / 2.1e-14   16 k 4.4e-14 / 7.1e-15   22.05 k 6.6e-14 / 1.8e-14   44.1 k 1.2e-13 / 6.0e-14
                48 k 2.1e-13 / 1.6e-13   96 k 4.3e-13 / 5.3e-14
    speech      8 k 1.4e-15   22.05 k 7.8e-15   44.1 k 1.4e-14   48 k 2.0e-14   96 k 3.6e-14 (LUFS <= 1.1e-14)
    ten minutes at 16 k (5 997 blocks) 8.9e-15 / 0; chunk edges 4.6e-14; 65 rows 5.9e-15; 130 rows 7.1e-15
    relative gate: margins -0.0022 / +0.0045 LU, LUFS difference 1.8e-15 (one block the other way: 1.2 dB)

The row ``tone_silence`` found a fault, fixed in the same change.  After the tone it is digital silence, and the blocks
inside it hold only the filter's ringing: energies down to 7e-126 against 0.12 for the tone.  With the chunk scan in
plain fp64 the kernel was 1.0e-9 (8 kHz) to 4.9e-8 (96 kHz) relative from scipy there, about 70 times scipy's own distance
from a long-double run of the same recurrence (``loudness_ref.k_filter_longdouble``): P * state cancels through the
near-double pole at 1, once per 128 samples.  The scan now carries the state and P as double-double (P from a
long-double run on the host).  scipy vs long double / kernel vs long double / kernel vs scipy on that row:
    8 k 1.5e-11 / 9.7e-13 / 1.6e-11   22.05 k 2.9e-11 / 3.1e-12 / 3.2e-11   44.1 k 9.0e-11 / 1.6e-11 / 1.1e-10
    48 k 1.8e-10 / 1.7e-11 / 1.7e-10   96 k 6.5e-10 / 1.7e-11 / 6.7e-10
so the kernel is nearer the long-double run than scipy is, and what it differs from scipy by is scipy's own error.  The
same change took DC + rumble at 96 kHz from 1.0e-11 to 4.3e-13.
"""
import numpy as np
import pytest
import torch
from scipy.signal import lfilter

import vectorquantizedcpc_amd.loudness as pyloudnorm
from oracle import loudness_ref as L
from oracle import zoo
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu


def _speech(n, name, rate=16000, amp=0.3):
    u = synth.uniform01("loud64/" + name, n)
    t = np.arange(n) / float(rate)
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t + len(name))
    return (amp * env * (np.sin(2 * np.pi * 180 * t) + 0.4 * np.sin(2 * np.pi * 2310 * t + 0.3)) + 0.05 * (u - 0.5)).astype(np.float32)


def _split_move(x, rate):
    """Relative movement of the oracle's block energies when scipy filters ``x`` in two halves with carried state."""
    y = np.asarray(x, dtype=np.float64)
    h = len(y) // 2
    for b, a in L.k_weighting(rate):
        y0, zi = lfilter(b, a, y[:h], zi=np.zeros(2))
        y1, _ = lfilter(b, a, y[h:], zi=zi)
        y = np.concatenate([y0, y1])
    l, u = L.block_bounds(len(y), rate)
    z = np.array([(1.0 / (L.BLOCK_S * rate)) * np.sum(np.square(y[p:q])) for p, q in zip(l, u)])
    return float(np.abs(z / L.block_energies(x, rate) - 1).max())


def _measure(rows, rate, pad=0.0):
    lens = [len(r) for r in rows]
    x = np.full((len(rows), max(lens)), pad, np.float32)
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    lufs, z = pyloudnorm.Meter(rate).integrated_loudness(torch.from_numpy(x).cuda(), lengths=lens, return_blocks=True)
    return lufs.cpu().numpy(), [v.cpu().numpy() for v in z]


def _check(lufs, z, x, rate, label, quiet=False, ringing=False):
    """Every block at 1e-10 relative from scipy.  ``ringing=True`` (the rows that end in digital silence): scipy's own
    float64 error exceeds 1e-10 in the blocks that hold only the filter's ringing, so there every block must be within
    1e-10 of the long-double run of the same recurrence, and within max(1e-10, 10 u) of scipy, where u is scipy's largest
    distance from the long-double run on that row, measured here."""
    zw = L.block_energies(x, rate)
    assert z.shape == zw.shape, label
    bound = 1e-10
    if ringing:
        zl = L.block_energies_longdouble(x, rate)
        u = float(np.abs(zw / zl - 1).max())
        vs_ld = float(np.abs(z / zl - 1).max())
        bound = max(1e-10, 10.0 * u)
        print("\nloudness %-28s smallest block energy %.1e: scipy vs long double %.2e, kernel vs long double %.2e, kernel vs scipy %.2e (bound %.2e)"
              % (label, float(zl.min()), u, vs_ld, float(np.abs(z / zw - 1).max()), bound))
        assert vs_ld < 1e-10, (label, vs_ld)
    rel = float(np.abs(z / zw - 1).max())
    want = L.gate(zw)
    d = 0.0 if lufs == want else abs(lufs - want)
    if not quiet:
        print("\nloudness %-28s blocks %5d  max rel block error %.2e  |LUFS diff| %.2e  (scipy split-state moves %.2e)"
              % (label, len(zw), rel, d, _split_move(x, rate)))
    assert rel < bound, (label, rel, bound)
    assert d < 1e-9, (label, lufs, want)
    return rel


@pytest.mark.parametrize("rate", [8000, 22050, 44100, 48000, 96000])
def test_block_energies_at_other_rates(rate):
    n = 3 * rate + 17
    rows = [zoo.make("dc_rumble", n, rate), _speech(n - 1001, "r%d" % rate, rate), zoo.make("tone_silence", 2 * rate, rate)]
    lufs, z = _measure(rows, rate)
    for b, name in enumerate(("dc_rumble", "speech", "tone_silence")):
        _check(lufs[b], z[b], rows[b], rate, "%s @ %d" % (name, rate), ringing=name == "tone_silence")


def test_dc_and_rumble_at_16k_and_ten_minutes():
    x = zoo.make("dc_rumble", 48000)
    lufs, z = _measure([x], 16000)
    _check(lufs[0], z[0], x, 16000, "dc_rumble @ 16000")
    n = 600 * 16000
    t = np.arange(n) / 16000.0
    long_ = (_speech(n, "tenmin") * (0.6 + 0.4 * np.sin(2 * np.pi * t / 37.0)).astype(np.float32)).astype(np.float32)
    lufs, z = _measure([long_], 16000)
    assert len(z[0]) == 5997
    _check(lufs[0], z[0], long_, 16000, "ten minutes @ 16000")


@pytest.mark.parametrize("rate,lo,hi", [(16000, 6400, 40000), (22050, 8820, 55125), (44100, 17640, 110250)])
def test_block_count_for_every_length(rate, lo, hi):
    """0.4 s to 2.5 s, every sample count: (T - 0.4) / 0.1 passes x.5 (half to even) and every other rounding edge."""
    lib = pyloudnorm._lib.load()
    h = pyloudnorm._handle(rate, torch.device("cuda", 0))
    got = np.array([lib.vqcpc_loudness_blocks(h, n) for n in range(lo, hi + 1)])
    want = np.array([L.n_blocks(n, rate) for n in range(lo, hi + 1)])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (rate, [(lo + int(i), int(got[i]), int(want[i])) for i in bad[:5]])
    assert lib.vqcpc_loudness_blocks(h, lo - 1) == 0
    # the sweep does contain halves that round DOWN to even, which floor(x + 0.5) would round up (at 22 050 Hz no sample
    # count lands on a half: 8820 + 2205 k + 1102.5 is never an integer)
    x = (np.arange(lo, hi + 1) / rate - L.BLOCK_S) / (L.BLOCK_S * (1.0 - L.OVERLAP))
    assert rate == 22050 or np.any(np.round(x) != np.floor(x + 0.5))
    print("\nloudness block count @ %d: %d lengths, %d of them where half-to-even and floor(x + 0.5) differ"
          % (rate, len(got), int(np.sum(np.round(x) != np.floor(x + 0.5)))))


def test_chunk_edges_and_a_step_at_them():
    """Lengths one short of, at and one past a multiple of the 128-sample chunk (6400 = 50 chunks is one gating block; 6399 is
    shorter than one block and is refused, which tests/test_gpu_loudness.py checks), and a
    step in the signal at samples 127, 128 and 129: the last sample of chunk 0, the first of chunk 1, the one after."""
    rows, labels = [], []
    for n in (6400, 6401, 6527, 6528, 6529, 8063, 8064, 8065):
        for at in (127, 128, 129):
            x = _speech(n, "edge%d" % n, amp=0.1)
            x[at:] += np.float32(0.5)
            rows.append(x)
            labels.append("n %d step at %d" % (n, at))
    lufs, z = _measure(rows, 16000)
    worst = max(_check(lufs[b], z[b], rows[b], 16000, labels[b], quiet=True) for b in range(len(rows)))
    print("\nloudness chunk edges: %d rows, worst rel block error %.2e" % (len(rows), worst))
    one, z1 = _measure([rows[4]], 16000)
    assert one[0] == lufs[4] and np.array_equal(z1[0], z[4])


@pytest.mark.parametrize("B", [65, 130])
def test_batches_wider_than_a_workgroup(B):
    rows = [_speech(6400 + (b * 211) % 9000, "wide%d" % b, amp=0.02 + 0.004 * b) for b in range(B)]
    lufs, z = _measure(rows, 16000)
    assert lufs.shape == (B,) and len(z) == B
    worst = max(_check(lufs[b], z[b], rows[b], 16000, "row %d" % b, quiet=True) for b in range(B))
    print("\nloudness B=%d: worst rel block error %.2e" % (B, worst))
    for b in (0, 63, 64, B - 1):
        one, z1 = _measure([rows[b]], 16000)
        assert one[0] == lufs[b] and np.array_equal(z1[0], z[b]), b


def test_one_fully_gated_row_and_poison_padding():
    """A row wholly under the absolute gate reads -inf, alone in its batch; the others equal their single-row calls bit for
    bit.  NaN and 1e30 behind ``lengths`` change no bit."""
    rows = [_speech(9000 + 500 * b, "gate%d" % b, amp=0.1 + 0.05 * b) for b in range(5)]
    rows[2] = (_speech(11000, "gate-quiet") * np.float32(1e-5)).astype(np.float32)
    assert L.integrated_loudness(rows[2], 16000) == -np.inf and rows[2].any()
    lufs, z = _measure(rows, 16000)
    assert lufs[2] == -np.inf and np.isfinite(np.delete(lufs, 2)).all()
    for b in range(5):
        if b != 2:
            _check(lufs[b], z[b], rows[b], 16000, "beside a gated row: %d" % b)
        one, z1 = _measure([rows[b]], 16000)
        assert one[0] == lufs[b] and np.array_equal(z1[0], z[b]), b
    for pad in (np.nan, 1e30):
        lp, zp = _measure(rows, 16000, pad=pad)
        assert np.array_equal(lp.view(np.uint64), lufs.view(np.uint64)), pad
        assert all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(zp, z)), pad


def test_relative_gate_between_two_blocks_a_hundredth_of_a_lu_apart():
    """3 s loud, then 1 s at gain g, then 1 s at g + 0.01 dB.  g is bisected on the oracle until the relative threshold
    (mean of the absolutely gated blocks - 10 LU) falls between the loudnesses of the blocks inside the two quiet seconds; the
    conditions are asserted on the oracle, then the GPU must make the same gating decisions (1e-9 dB: one block gated
    the other way moves the result by 1e-3 dB or more)."""
    rate = 16000
    t = np.arange(5 * rate) / float(rate)
    tone = np.sin(2 * np.pi * 997 * t)

    def build(g_db):
        env = np.full(len(t), 0.5)
        env[3 * rate: 4 * rate] = 0.5 * 10 ** (g_db / 20)
        env[4 * rate:] = 0.5 * 10 ** ((g_db + 0.01) / 20)
        return (env * tone).astype(np.float32)

    def margins(x):
        z = L.block_energies(x, rate)
        l = -0.691 + 10 * np.log10(z)
        gamma = -0.691 + 10 * np.log10(np.mean(z[l >= L.GAMMA_ABS])) - 10.0
        return l - gamma, z

    lo, hi = -20.0, -5.0                                    # at lo both quiet seconds are gated, at hi neither
    for _ in range(60):
        g = 0.5 * (lo + hi)
        m, _ = margins(build(g))
        first, second = m[31:37], m[41:47]                  # blocks that lie inside seconds 4 and 5, past the edge's transient
        if second.max() < 0:
            lo = g
        elif first.min() > 0:
            hi = g
        else:
            break
    x = build(g)
    m, z = margins(x)
    assert m[31:37].max() < 0 < m[41:47].min() and m[41:47].min() - m[31:37].max() < 0.011, (g, m[31:37], m[41:47])
    got = pyloudnorm.Meter(rate).integrated_loudness(x)
    want = L.gate(z)
    dropped = L.gate(np.delete(z, 41))
    print("\nloudness relative gate: g %.4f dB, margins %.4f / +%.4f LU, |LUFS diff| %.2e (one block the other way: %.1e)"
          % (g, m[31:37].max(), m[41:47].min(), abs(got - want), abs(dropped - want)))
    assert abs(dropped - want) > 1e-4
    assert abs(got - want) < 1e-9
