"""CPU restatement of the resampling the reference gets from ``librosa.load(path, sr=...)`` (``convert.py:54-56``) --
TEST INFRASTRUCTURE, like the rest of oracle/.

librosa ^0.8 resamples with ``res_type='kaiser_best'``, i.e. resampy's band-limited sinc interpolation (J. O. Smith,
"Digital Audio Resampling"): a half sinc window sampled at 2**precision points per zero crossing, tapered by a Kaiser
window, linearly interpolated between table entries; for down-sampling the filter is stretched and scaled by the rate
ratio.  resampy and librosa are not installed here and cannot be fetched: **parity unpinned**.  The filter
constants below (64 zero crossings, precision 9, Kaiser beta 14.769656459379492, roll-off 0.9475937167399596) are
resampy's published ``kaiser_best`` design, restated from its documentation -- they cannot be checked against the
package's stored table offline.  Everything in float64, as resampy computes on librosa's float32 input upcast.
Version assumption: the output clock follows resampy 0.2.2's interpolation loop (what librosa ^0.8 pins as >= 0.2.2), which
advances the input time by SEQUENTIAL additions `time_register += time_increment` -- not `t * time_increment` as resampy >= 0.3's
rewritten kernel does; the two differ in the last bits of the interpolation weights on long signals.
"""
import numpy as np

KAISER_BEST = {"num_zeros": 64, "precision": 9, "beta": 14.769656459379492, "rolloff": 0.9475937167399596}


def sinc_window(num_zeros, precision, beta, rolloff):
    """resampy.filters.sinc_window with a Kaiser taper: right half of the interpolation filter."""
    num_bits = 2 ** precision
    n = num_bits * num_zeros
    sinc_win = rolloff * np.sinc(rolloff * np.linspace(0, num_zeros, num=n + 1, endpoint=True))
    taper = np.kaiser(2 * n + 1, beta)[n:]
    return taper * sinc_win, num_bits


def resample(x, sr_orig, sr_new, filt=KAISER_BEST):
    """librosa.resample(x, sr_orig, sr_new, res_type='kaiser_best', fix=True, scale=False) for a mono signal."""
    x = np.asarray(x, dtype=np.float64)
    if sr_orig == sr_new:
        return x.copy()
    ratio = float(sr_new) / float(sr_orig)
    n_out = int(np.ceil(x.shape[-1] * ratio))                  # librosa's n_samples; resampy yields int(n * ratio), fix_length pads
    n_res = int(x.shape[-1] * ratio)
    win, num_table = sinc_window(**filt)
    win = win.copy()
    if ratio < 1:
        win *= ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    time_increment = 1.0 / ratio
    index_step = int(scale * num_table)
    nwin = win.shape[0]
    n_orig = x.shape[0]
    y = np.zeros(n_out)
    time_register = 0.0
    for t in range(n_res):
        n = int(time_register)
        frac = scale * (time_register - n)
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        i_max = min(n + 1, (nwin - offset) // index_step)
        if i_max > 0:
            idx = offset + index_step * np.arange(i_max)
            y[t] += np.dot(win[idx] + eta * delta[idx], x[n - np.arange(i_max)])
        frac = scale - frac
        index_frac = frac * num_table
        offset = int(index_frac)
        eta = index_frac - offset
        k_max = min(n_orig - n - 1, (nwin - offset) // index_step)
        if k_max > 0:
            idx = offset + index_step * np.arange(k_max)
            y[t] += np.dot(win[idx] + eta * delta[idx], x[n + 1 + np.arange(k_max)])
        time_register += time_increment
    return y


def output_clock(n, sr_orig, sr_new):
    """resampy 0.2.2's input time of outputs 0..n-1: the SEQUENTIAL float64 sums 0, inc, inc + inc, ... (``np.cumsum`` adds
    one term at a time, left to right)."""
    inc = 1.0 / (float(sr_new) / float(sr_orig))
    return np.concatenate([[0.0], np.cumsum(np.full(max(n - 1, 0), inc))])[:n]


def resample_at(x, sr_orig, sr_new, indices, order="forward", filt=KAISER_BEST):
    """``resample(x, sr_orig, sr_new)[indices]`` without the outputs in between (a 130 000-sample check needs a few hundred).

    Each wing is summed one tap at a time instead of by ``np.dot``: ``order='forward'`` from the centre tap outwards, left
    wing then right wing in one accumulator; ``order='reverse'`` from the far end of each wing inwards, right wing first.
    The two differ from each other and from ``resample`` by float64 rounding only, which is what the tests of the float32
    result lean on.  Indices at or past ``int(len(x) * ratio)`` give 0, as the padding of ``resample`` does."""
    x = np.asarray(x, dtype=np.float64)
    idx = np.asarray(indices, dtype=np.int64)
    ratio = float(sr_new) / float(sr_orig)
    n_orig = x.shape[0]
    n_res = int(n_orig * ratio)
    win, num_table = sinc_window(**filt)
    win = win.copy()
    if ratio < 1:
        win *= ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    index_step = int(scale * num_table)
    nwin = win.shape[0]
    live = idx < n_res
    treg = output_clock(int(idx.max()) + 1, sr_orig, sr_new)[idx]
    n = treg.astype(np.int64)
    frac = scale * (treg - n)
    wings = []
    for f, count, sign, base in ((frac, n + 1, -1, n), (scale - frac, n_orig - n - 1, 1, n + 1)):
        index_frac = f * num_table
        offset = index_frac.astype(np.int64)
        eta = index_frac - offset
        taps = np.minimum(count, (nwin - offset) // index_step)
        wings.append((offset, eta, np.where(live, taps, 0), sign, base))
    acc = np.zeros(len(idx))
    for offset, eta, taps, sign, base in (wings if order == "forward" else wings[::-1]):
        top = int(taps.max()) if len(taps) else 0
        for i in (range(top) if order == "forward" else range(top - 1, -1, -1)):
            on = i < taps
            k = np.where(on, offset + i * index_step, 0)
            src = np.where(on, base + sign * i, 0)
            acc = np.where(on, acc + (win[k] + eta * delta[k]) * x[src], acc)
    return acc


def _ordered(a32):
    """float32 -> int64 keys whose difference counts representable values between two floats."""
    u = np.ascontiguousarray(a32, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(u < 0, -(u & 0x7FFFFFFF), u)


def compare_rounded(got, want):
    """The rule for a float32 result of this float64 algorithm -> (all_within, share_bit_equal, max_ulp, raw_share).

    ``want`` is float64.  An output is within the rule if it is at most one float32 ulp from ``float32(want)`` or within
    1e-12 absolute (sums that cancel to nothing have no meaningful last bit).  ``share_bit_equal`` is the share of outputs
    whose bits equal ``float32(want)``; callers require 0.999.  Outputs inside the absolute bound count as equal there: the
    midpoint of every edge of an up-sampled square wave cancels to 1e-17, 3 % of that signal, and the float64 oracle summed
    in another order does not reproduce those bits either (``tests/test_resample_cpu.py``).  ``max_ulp`` leaves them out
    likewise.  ``raw_share`` is plain bit equality over all outputs, for the record."""
    got = np.ascontiguousarray(got, dtype=np.float32)
    w32 = np.asarray(want, dtype=np.float64).astype(np.float32)
    ulp = np.abs(_ordered(got) - _ordered(w32))
    near_zero = np.abs(got.astype(np.float64) - np.asarray(want, dtype=np.float64)) <= 1e-12
    ok = (ulp <= 1) | near_zero
    equal = (got.view(np.uint32) == w32.view(np.uint32)) | near_zero
    big = np.where(near_zero, 0, ulp)
    raw = got.view(np.uint32) == w32.view(np.uint32)
    return (bool(ok.all()), float(equal.mean()) if equal.size else 1.0, int(big.max()) if big.size else 0,
            float(raw.mean()) if raw.size else 1.0)
