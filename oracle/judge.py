"""The draw rule of the vocoder's self-oracle, stated once (tests/ and __graft_entry__.smoke() call it).

A decode is judged on ITS OWN history: the C oracle is teacher-forced on the samples the decode drew, and wherever the oracle's
Gumbel-max draw differs, the drawn class must score within TIE of the oracle's best -- a rounding-level tie between two
summation orders.  How many draws must be exact is the caller's criterion, from the (n, exact) pairs this returns.
(The float64 judges, f64_ref.check_draws and tests/vocoder_size_cases.judge_draws, are another rule.)
"""
import numpy as np

from .ref import mulaw_decode, sample_from_logits, vocoder_generate

TIE = 2e-5        # on the Gumbel-max score, fp32


def judge_draws(sd, z, spk, mu, *, seed, utt_ids, rows, steps, n_codes=None, wav=None, bits=8):
    """``mu`` (B, T): the classes a decode drew for code rows ``z`` (B, Tc) and speakers ``spk`` (B,) -- numpy or CPU tensors;
    ``utt_ids[b]``: row b's sampling-stream id.  For every b in ``rows``, over the first n = min(steps, 320 * n_codes[b]) draws:
    every draw that differs from the oracle's is within TIE of its best score and, if ``wav`` (B, T) is given, wav[b, :n] is the
    mu-law table of the draws and wav[b, n:] is zero.  Returns [(n, exact draws)] in the order of ``rows``."""
    z, spk, mu = np.asarray(z), np.asarray(spk), np.asarray(mu)
    table = None if wav is None else np.array([mulaw_decode(c, bits) for c in range(1 << bits)], np.float32)
    stats = []
    for b in rows:
        nc = z.shape[1] if n_codes is None else n_codes[b]
        n = min(steps, 320 * nc)
        drawn = mu[b, :n]
        history = np.concatenate([[1 << (bits - 1)], drawn[:-1]])
        r = vocoder_generate(sd, z[b, :nc], int(spk[b]), seed=seed, utterance=utt_ids[b], n_steps=n, inputs=history,
                             want_logits=True, bits=bits)
        differ = np.nonzero(r["samples"] != drawn)[0]
        for t in differ:
            pick, sc = sample_from_logits(r["logits"][t], seed, utt_ids[b], int(t))
            gap = sc[pick] - sc[int(drawn[t])]              # fp32, like the scores
            assert gap <= TIE, f"row {b}, step {int(t)}: the sample is not the oracle's Gumbel-max choice (class {int(drawn[t])} " \
                               f"scores {float(gap):.3g} below the oracle's {pick})"
        if wav is not None:
            w = np.asarray(wav)[b]
            assert np.array_equal(w[:n], table[drawn]), f"row {b}: the waveform is not the mu-law table of its draws"
            assert not w[n:].any(), f"row {b}: samples behind the end ({n})"
        stats.append((n, n - len(differ)))
    return stats
