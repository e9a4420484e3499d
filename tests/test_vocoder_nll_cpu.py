"""Vocoder scoring without a GPU (the ABI of vqcpc_vocoder_nll: tests/test_abi_cpu.py): the `score-vocoder` command line, the driver's cut rule and
bucket bookkeeping (stub models), the float64 helper against torch's cross_entropy, the mu-law path, and the conditions on the
inputs of the GPU cases (tests/nll_ref.py): at most 1 % ambiguous samples, some surely correct ones.

The tests of the command line, the driver and the mu-law path need the feature and fail without it.  The float64 helper
test, the ambiguity-cap cases and the wave determinism test check the TEST inputs and helpers themselves (tests/nll_ref.py and
oracle/f64_ref.py only): they hold with or without the feature, and are here so that a bad input is caught without a GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nll_ref
from vectorquantizedcpc_amd import cli, driver, preprocess, synth


def test_cli_score_vocoder_parses_and_rejects_a_missing_checkpoint(capsys):
    assert "score-vocoder" in cli.__doc__
    for argv in (["score-vocoder", "--dataset", "d", "--in-dir", "w"],
                 ["score-vocoder", "--dataset", "d", "--in-dir", "w", "--cpc-checkpoint", "c.pt"],
                 ["score-vocoder", "--dataset", "d", "--random-init"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
    capsys.readouterr()
    seen = {}
    orig = cli.score_vocoder_dataset
    cli.score_vocoder_dataset = lambda args: seen.update(vars(args)) or 0
    try:
        assert cli.main(["score-vocoder", "--dataset", "d", "--in-dir", "w", "--random-init", "--per-utterance"]) == 0
    finally:
        cli.score_vocoder_dataset = orig
    assert seen["in_dir"] == "w" and seen["per_utterance"] and seen["random_init"] and seen["max_batch"] == 64


class _Conf:
    class rnnms:
        upsampling_t = 160
        bits_mu_law = 8


class _StubVocoder:
    """Records every nll() call; an utterance's 'nll' is the sum of its scored targets, so the bookkeeping is checkable."""
    conf = _Conf

    def __init__(self):
        self.calls = []

    def nll(self, audio, z, speaker, *, lengths=None, n_codes=None, per_sample=False):
        self.calls.append((tuple(audio.shape), tuple(z.shape), list(lengths), list(n_codes), speaker.tolist()))
        B = audio.shape[0]
        s = torch.zeros(B, dtype=torch.float64)
        n = torch.zeros(B, dtype=torch.int64)
        for b in range(B):
            assert lengths[b] - 1 <= 320 * n_codes[b] and lengths[b] <= audio.shape[1] and n_codes[b] <= z.shape[1]
            n[b] = max(lengths[b] - 1, 0)
            s[b] = float(audio[b, 1:lengths[b]].sum())
            assert (z[b, :n_codes[b]] == 1000 * int(speaker[b]) + torch.arange(n_codes[b])).all()     # its own codes, in its row
        from vectorquantizedcpc_amd.network_vocoder import VocoderNLL
        return VocoderNLL(s, n, n // 2, None)


def test_driver_cut_rule_and_bucket_bookkeeping(monkeypatch):
    assert driver.scored_samples(1000, 3) == 961 and driver.scored_samples(900, 3) == 900 and driver.scored_samples(5, 0) == 1
    frames = [21, 40, 22, 101, 39, 64, 23]
    mels = [torch.zeros(80, t) for t in frames]
    speakers = [3, 1, 4, 1, 5, 9, 2]
    lens = [160 * (t - 1) + 37 * i for i, t in enumerate(frames)]                  # samples: some past what the codes cover
    lens[5] = 5000                                                                  # shorter than its 32 codes cover
    audio = [np.arange(n) % 256 for n in lens]

    def fake_encode(encoder, ms, **kw):
        return [{"indices": 1000 * speakers[i] + torch.arange(driver.out_frames(m.shape[-1]))} for i, m in enumerate(ms)]

    monkeypatch.setattr(driver, "encode_utterances", fake_encode)
    enc = torch.nn.Linear(1, 1)
    want_total = None
    for max_batch in (2, 64):
        voc = _StubVocoder()
        rec, tot = driver.score_vocoder(enc, voc, mels, audio, speakers, max_batch=max_batch, max_pad_frac=0.25)
        assert all(len(c[2]) <= max_batch for c in voc.calls)
        assert sorted(s for c in voc.calls for s in c[4]) == sorted(speakers)
        for i, r in enumerate(rec):
            nc = driver.out_frames(frames[i])
            keep = min(lens[i], 320 * nc + 1)
            assert r["n_codes"] == nc and r["n_scored"] == keep - 1 and r["n_cut"] == lens[i] - keep
            assert r["nll_sum"] == float(audio[i][1:keep].sum())
        assert rec[5]["n_cut"] == 0 and rec[3]["n_cut"] > 0
        assert tot["n_scored"] == sum(r["n_scored"] for r in rec) and tot["nll_sum"] == sum(r["nll_sum"] for r in rec)
        assert tot["n_cut"] == sum(r["n_cut"] for r in rec) and tot["n_utterances"] == 7
        assert tot["loss"] == tot["nll_sum"] / tot["n_scored"] and tot["accuracy"] == tot["n_correct"] / tot["n_scored"]
        assert abs(tot["bits_per_sample"] * np.log(2.0) - tot["loss"]) < 1e-9
        want_total = want_total or tot
        assert tot == want_total
    with pytest.raises(ValueError):
        driver.score_vocoder(enc, _StubVocoder(), mels, None, speakers)


def test_float64_helper_against_torch_cross_entropy():
    g = torch.Generator().manual_seed(5)
    e = torch.randn(3, 50, 256, generator=g, dtype=torch.float64) * 3.0
    t = torch.randint(0, 256, (3, 50), generator=g)
    t[0, 0] = int(e[0, 0].argmax())
    nll, lse, et, gap_t, gap_2 = nll_ref.nll_from_energies(e, t)
    want = F.cross_entropy(e.transpose(1, 2), t, reduction="none").numpy()
    assert np.abs(nll - want).max() <= 1e-12
    assert abs(nll.mean() - float(F.cross_entropy(e.transpose(1, 2), t))) <= 1e-12
    assert np.abs(lse - et - nll).max() <= 1e-12
    assert gap_t[0, 0] == 0.0 and (gap_t >= 0).all() and (gap_2 >= 0).all()
    srt = np.sort(e.numpy(), axis=-1)
    assert np.array_equal(gap_2, srt[..., -1] - srt[..., -2])


def test_mulaw_path_is_the_host_formula():
    w = nll_ref.waves(3)[1]
    want = preprocess.mulaw_encode(w / np.abs(w).max() * 0.999, 256)
    got = driver.mulaw_classes(w)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(driver.mulaw_classes(torch.from_numpy(w)), want)
    assert got.min() >= 0 and got.max() <= 255


def test_synthetic_waves_are_deterministic_and_mixed_length():
    a, b = nll_ref.waves(12), nll_ref.waves(12)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert len({len(x) for x in a}) >= 6 and all(np.abs(x).max() < 1.0 for x in a)


@pytest.mark.parametrize("name", ["default", "stressed"])
@pytest.mark.parametrize("case", ["equal", "ragged", "big"])
def test_gpu_case_inputs_respect_the_ambiguity_cap(name, case):
    """From the float64 reference alone: at most 1 % of the scored samples of every GPU case are ambiguous (target within
    2 LOGIT_TOL of the best energy without surely being it)."""
    ref = nll_ref.reference(name, case)
    frac = ref.ambiguous_fraction()
    print("%s %s: %d scored, %d surely correct, %d ambiguous (%.4f %%), loss %.6f" % (
        name, case, int(ref.n_scored.sum()), int(ref.sure_correct.sum()), int(ref.ambiguous.sum()), 100 * frac, ref.loss))
    assert frac <= nll_ref.AMBIGUOUS_CAP
    assert np.isfinite(ref.nll).all() and (ref.bound[ref.mask] > 0).all()
    if case == "equal":
        assert int(ref.sure_correct.sum()) > 0
