"""-m gpu: csrc/resample.hip against the float64 oracle at the places the first tests did not reach.

The kernel evaluates both filter wings in float64, tap by tap in the reference's order, on the reference's own output clock
(the sequential sums ``time_register += time_increment``, made once on the host and kept in a grow-only device table),
and rounds once to float32.  So the rule is not a tolerance on amplitudes but on roundings (``resample_ref.compare_rounded``):
every output within ONE float32 ulp of ``float32(want)`` or within 1e-12 absolute where the sum cancels to nothing, and at
least 99.9 % of the outputs bit-equal.  tests/test_resample_cpu.py shows the oracle meets the same rule against itself
when its wings are summed in other orders, on every single-row case used here (tests/resample_cases.py).

Covered: ten rate pairs; lengths 1, 2, 63, 64, 65, 441 (441 samples at 44.1 kHz are exactly 160 outputs); impulses at the
first and last sample and a full-scale square wave, whose overshoot above 1 must survive; batches of 257 and 513 rows
(``RS_MAXB`` = 256 rows per launch: the second and third launches work on offset pointers); a row full to its end beside
a row of 1e30 and NaN behind ``lengths``; the clock table growing past 65 536 and 131 072 outputs on a live handle.

Observed on MI355X: in 39 of the 40 comparisons here every output is bit-equal to float32(want), the 1 537 checked outputs
of the 132 063-output signal included (max |got - want| 5.9e-8 = the float32 rounding of a value near 1.2).  The one
exception is the square wave 8000 -> 16000: plain bit equality 0.97000, the other 3 % being the edge midpoints that cancel
to 1e-17 and fall under the absolute bound; no output outside that class differs (max ulp 0).  The share the rule asserts
counts that class as equal; the plain share is printed beside it.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_cases
from oracle import resample_ref as R
from vectorquantizedcpc_amd import _lib, preprocess

pytestmark = pytest.mark.gpu


def _rule(got, want, label):
    ok, share, ulp, raw = R.compare_rounded(got, want)
    print("\nresample %-32s n %6d  max ulp %d  bit-equal %.5f (plain, cancelling outputs included: %.5f)  max |diff| %.2e"
          % (label, len(got), ulp, share, raw, float(np.abs(got - want).max()) if len(got) else 0.0))
    assert ok and share >= 0.999, (label, ulp, share)


def _batch(rows, pad=0.0, Lmax=None):
    lens = [len(r) for r in rows]
    x = np.full((len(rows), Lmax or max(lens)), pad, np.float32)
    for b, r in enumerate(rows):
        x[b, : len(r)] = r
    return x, lens


@pytest.mark.parametrize("case", resample_cases.cases(), ids=lambda c: c[0])
def test_single_rows_round_like_the_oracle(case):
    label, sr0, sr1, x = case
    got = preprocess.resample(torch.from_numpy(x).cuda(), sr0, sr1).cpu().numpy()
    want = R.resample(x, sr0, sr1)
    assert got.dtype == np.float32 and got.shape == want.shape == (int(np.ceil(len(x) * (float(sr1) / float(sr0)))),), label
    n_res = int(len(x) * (float(sr1) / float(sr0)))
    assert not got[n_res:].any() and not want[n_res:].any()          # librosa's fix_length zero tail
    _rule(got, want, label)
    if label.startswith("square"):
        assert got.max() > 1.0 and want.max() > 1.0                  # Gibbs overshoot is signal, not error: no clipping
    if label == "length 441":
        assert n_res == 160


def test_the_lengths_as_one_ragged_batch():
    rows = [c[3] for c in resample_cases.cases() if c[0].startswith("length")]
    x, lens = _batch(rows)
    got = preprocess.resample(torch.from_numpy(x).cuda(), 44100, 16000, lengths=lens).cpu().numpy()
    for b, r in enumerate(rows):
        want = R.resample(r, 44100, 16000)
        _rule(got[b, : len(want)], want, "batched length %d" % len(r))
        assert not got[b, int(len(r) * (16000.0 / 44100.0)):].any()


@pytest.mark.parametrize("B", [257, 513])
def test_more_rows_than_one_launch_holds(B):
    """Rows 0, 255, 256, 257 and the last in full against the oracle; each equals its single-row call bit for bit."""
    rows = [resample_cases.smooth_noise("rs/big/%d" % b, 600 - (b * 7) % 290) for b in range(B)]
    rows[B - 1] = resample_cases.smooth_noise("rs/big/last", 600)
    x, lens = _batch(rows)
    got = preprocess.resample(torch.from_numpy(x).cuda(), 44100, 16000, lengths=lens).cpu().numpy()
    assert got.shape == (B, int(np.ceil(600 * (16000.0 / 44100.0))))
    for b in sorted({0, 255, 256, 257, B - 1} & set(range(B))):
        want = R.resample(rows[b], 44100, 16000)
        _rule(got[b, : len(want)], want, "B=%d row %d" % (B, b))
        assert not got[b, len(want):].any()
        alone = preprocess.resample(torch.from_numpy(rows[b]).cuda(), 44100, 16000).cpu().numpy()
        assert np.array_equal(got[b, : len(alone)].view(np.uint32), alone.view(np.uint32)), b
    # every other row: the zero tail starts where its own length says (a row read at the wrong offset has another length)
    for b in range(B):
        n_res = int(lens[b] * (16000.0 / 44100.0))
        assert got[b, n_res - 1] != 0 and not got[b, n_res:].any(), b


def test_row_end_beside_a_huge_neighbour_and_poison_padding():
    full = resample_cases.smooth_noise("rs/full", 2000)
    short = resample_cases.smooth_noise("rs/short", 777)
    x, lens = _batch([full, np.full(2000, 1e30, np.float32), short])
    got = preprocess.resample(torch.from_numpy(x).cuda(), 44100, 16000, lengths=lens).cpu().numpy()
    want = R.resample(full, 44100, 16000)
    _rule(got[0], want, "full row beside 1e30")
    alone = preprocess.resample(torch.from_numpy(full).cuda(), 44100, 16000).cpu().numpy()
    assert np.array_equal(got[0].view(np.uint32), alone.view(np.uint32))
    _rule(got[2, : int(np.ceil(777 * 16000 / 44100))], R.resample(short, 44100, 16000), "short row behind 1e30")
    assert np.isfinite(got).all() and np.abs(got[1, :700]).min() > 1e29
    for pad in (np.nan, 1e30):
        xp, _ = _batch([full, np.full(2000, 1e30, np.float32), short], pad=pad)
        again = preprocess.resample(torch.from_numpy(xp).cuda(), 44100, 16000, lengths=lens).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), pad


def _call(lib, h, x):
    """One row through ``vqcpc_resampler_run`` on the handle ``h`` (not the cached one of ``preprocess.resample``)."""
    w = torch.from_numpy(x).cuda()
    n_out = lib.vqcpc_resampler_out_len(h, len(x))
    out = torch.empty(n_out, device=w.device)
    _lib.check(lib.vqcpc_resampler_run(h, w.data_ptr(), (C.c_int * 1)(len(x)), 1, len(x), out.data_ptr(), n_out, _lib.current_stream()))
    return out.cpu().numpy()


def test_clock_table_grows_on_a_live_handle():
    """A handle of its own, so the table is empty at the start whatever ran before: a short call (the table gets 65 536
    entries), a call of 132 063 outputs (it doubles twice, after a stream sync), the short call again.  The long one is
    checked at both ends and across outputs 65 536 and 131 072, where a table that was not regrown would end."""
    sr0, sr1 = 22050, 32000
    short = resample_cases.smooth_noise("rs/grow/short", 1500)
    long_ = resample_cases.smooth_noise("rs/grow/long", 91000)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.vqcpc_resampler_create(sr0, sr1, C.byref(h)))
    try:
        first = _call(lib, h, short)
        got = _call(lib, h, long_)
        again = _call(lib, h, short)
    finally:
        lib.vqcpc_resampler_destroy(h)
    _rule(first, R.resample(short, sr0, sr1), "short before growth")
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    n_res = int(91000 * (float(sr1) / float(sr0)))
    assert n_res > 131072 and got.shape == (int(np.ceil(91000 * (float(sr1) / float(sr0)))),)
    idx = np.concatenate([np.arange(0, 256), np.arange(65536 - 256, 65536 + 256), np.arange(131072 - 256, 131072 + 256),
                          np.arange(n_res - 256, len(got))])
    _rule(got[idx], R.resample_at(long_, sr0, sr1, idx), "long: ends, 65 536, 131 072")
    assert not got[n_res:].any()
    # the accumulated clock is what is being replayed: at these outputs it no longer equals t * increment
    live = idx[idx < n_res]
    assert not np.array_equal(R.output_clock(n_res, sr0, sr1)[live], live * (1.0 / (float(sr1) / float(sr0))))
