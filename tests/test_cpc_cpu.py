"""CPU-side checks of CPC scoring: the ``CPCLoss`` surface against what the reference recorded in ``tests/golden/cpc_*.npz``
(``tools/gen_cpc_golden.py``), the negative-sampling protocol, the meaning of the fixtures' index arrays (a float64 numpy
restatement of ``model.py:191-316`` reproduces the reference's float64 results from them), the ABI additions and the
grouping logic of ``driver.score_batches``."""
import os
import re

import numpy as np
import pytest
import torch

import oracle
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, driver, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FULL_CASES = ["train_shape", "ties", "small_odd", "one_utt"]          # checked score by score, position by position
NEAR_TIE_CAP = 0.005


def load_case(name):
    """Fixture of one case with its index arrays as int64: ``utt`` (K, Utt, Neg), ``seq`` (K, Spk, Utt, Neg, L)."""
    g = dict(np.load(os.path.join(GOLD, f"cpc_{name}.npz")))
    n_pred, Spk, Utt, Neg, z_dim, c_dim, T = (int(v) for v in g["case"])
    K = n_pred // 2
    g.update(n_pred=n_pred, Spk=Spk, Utt=Utt, Neg=Neg, c_dim=c_dim, T=T, K=K, N=Spk * Utt, L=T - K)
    if str(g["draws"]) == "inline":
        utt, seq = g["utt_index"], g["seq_index"]
    else:                                                             # the train shape's draws: one file per step
        steps = [np.load(os.path.join(GOLD, f"cpc_{g['draws']}_draws_k{k}.npz")) for k in range(1, K + 1)]
        utt, seq = np.stack([s["utt_index"] for s in steps]), np.stack([s["seq_index"] for s in steps])
    g["utt"], g["seq"] = utt.astype(np.int64), seq.astype(np.int64)
    assert g["utt"].shape == (K, Utt, Neg) and g["seq"].shape == (K, Spk, Utt, Neg, T - K)
    if "margin" in g:
        g["correct"] = np.unpackbits(g["correct"])[: K * Spk * Utt * (T - K)].reshape(K, Spk * Utt, T - K).astype(bool)
    return g


def case_inputs(g, name):
    sd = synth.cpc_state_dict(n_prediction_steps=g["n_pred"], c_dim=g["c_dim"])
    z, c = synth.cpc_inputs(name, g["N"], g["T"], c_dim=g["c_dim"], n_codes=int(g["n_codes"]), runs=bool(g["runs"]))
    return sd, z, c


def f64_cpc(z, c, sd, utt, seq, dtype=np.float64):
    """Steps 1-5 of ``CPCLoss.forward`` in float64 numpy.  -> dict: ``f`` scores (K, N, 1 + Neg, L); ``mag`` = the magnitude
    sum of the score tolerance, (sum_d |z_d| (|W_k| |c| + |b_k|)_d + sum_d |z_d Wc_d|) / 8; ``step_loss`` (K), ``loss``;
    ``pos_loss`` = lse - f[:, :, 0] per position (K, N, L).  ``dtype=np.float32``: the same statements with every array and
    every operation in fp32 -- the plain fp32 restatement whose distance from float64 tests/cpc_cases.py calls ``err32``."""
    K, Spk, Utt, Neg, L = seq.shape
    z, c = np.asarray(z, dtype), np.asarray(c, dtype)
    zs = z.reshape(Spk, Utt, -1, z.shape[-1])
    f, mag = np.empty((K, Spk * Utt, 1 + Neg, L), dtype), np.empty((K, Spk * Utt, 1 + Neg, L), dtype)
    spk = np.arange(Spk).reshape(-1, 1, 1, 1)
    for k in range(1, K + 1):
        W = sd[f"predictors.{k - 1}.weight"].numpy().astype(dtype)
        b = sd[f"predictors.{k - 1}.bias"].numpy().astype(dtype)
        wc = c[:, :L] @ W.T + b                                                       # 1.
        wc_abs = np.abs(c[:, :L]) @ np.abs(W).T + np.abs(b)
        shift = zs[:, :, k:L + k]                                                     # 2. positives z[n, t + k]
        neg = shift[spk, utt[k - 1][None, :, :, None], seq[k - 1]]                    # 3. within speaker
        rows = np.concatenate([shift[:, :, None], neg], axis=2).reshape(Spk * Utt, 1 + Neg, L, -1)
        f[k - 1] = (rows * wc[:, None]).sum(-1) / dtype(8.0)                          # 4.
        mag[k - 1] = ((np.abs(rows) * wc_abs[:, None]).sum(-1) + np.abs(rows * wc[:, None]).sum(-1)) / dtype(8.0)
    m = f.max(axis=2, keepdims=True)                                                  # 5.
    lse = m[:, :, 0] + np.log(np.exp(f - m).sum(axis=2))
    pos_loss = lse - f[:, :, 0]
    step_loss = pos_loss.reshape(K, -1).mean(axis=1)
    return {"f": f, "mag": mag, "step_loss": step_loss, "loss": step_loss.mean(), "pos_loss": pos_loss}


# ------------------------------------------------------------------ module surface
def test_state_dict_surface_matches_reference():
    g = load_case("train_shape")
    cpc = V.CPCLoss(V.ConfCPC(12, 8, 8, 17, 64, 256))
    sd = cpc.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]] and len(sd) == 24
    assert [list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()] == g["shapes"].tolist()
    want = synth.cpc_state_dict()
    cpc.load_state_dict(want)
    assert all(torch.equal(cpc.state_dict()[k], want[k]) for k in want)
    assert cpc.n_prediction_steps == 6                                  # model.py:181


def test_no_cpu_fallback_and_shape_errors():
    cpc = V.CPCLoss(V.ConfCPC(12, 8, 8, 17, 64, 256)).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpc(torch.zeros(64, 70, 64), torch.zeros(64, 70, 256))


def test_cpc_checkpoint_entry(tmp_path):
    from vectorquantizedcpc_amd import io
    path = tmp_path / "ck.pt"
    torch.save({"encoder": {"w": torch.zeros(1)}, "cpc": synth.cpc_state_dict(), "epoch": 3}, path)
    sd = io.load_cpc_checkpoint(path)
    V.CPCLoss(V.ConfCPC(12, 8, 8, 17, 64, 256)).load_state_dict(sd)


# ------------------------------------------------------------------ protocol
def test_negatives_protocol_ranges_and_determinism():
    K, Spk, Utt, Neg, L = 3, 2, 5, 7, 13
    utt, seq = synth.cpc_negatives(13, 0, K, Spk, Utt, Neg, L)
    assert utt.dtype == torch.int64 and tuple(utt.shape) == (K, Utt, Neg) and tuple(seq.shape) == (K, Spk, Utt, Neg, L)
    assert int(utt.min()) >= 0 and int(utt.max()) < Utt and int(seq.min()) >= 0 and int(seq.max()) < L
    assert not bool((seq == torch.arange(L)).any())                     # never the anchor's own time step
    assert len(torch.unique(utt)) == Utt and len(torch.unique(seq)) == L
    again = synth.cpc_negatives(13, 0, K, Spk, Utt, Neg, L)
    assert torch.equal(utt, again[0]) and torch.equal(seq, again[1])
    other = synth.cpc_negatives(13, 1, K, Spk, Utt, Neg, L)
    assert not torch.equal(utt, other[0]) and not torch.equal(seq, other[1])
    seeded = synth.cpc_negatives(14, 0, K, Spk, Utt, Neg, L)
    assert not torch.equal(seq, seeded[1])
    assert not torch.equal(seq[0], seq[1])                              # the step is part of the counter
    utt2, seq2 = synth.cpc_negatives(13, 0, 1, 1, 1, 1, 2)              # L = 2: the only other position
    assert torch.equal(seq2.reshape(-1), torch.tensor([1, 0])) and int(utt2.max()) == 0


def test_negatives_protocol_known_answers():
    """Three draws recomputed word by word with the oracle's Philox (import only)."""
    seed, stream, K, Spk, Utt, Neg, L = (5 << 32) | 13, 9, 6, 8, 8, 17, 64
    utt, seq = synth.cpc_negatives(seed, stream, K, Spk, Utt, Neg, L)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    for k, u, j in ((1, 0, 0), (4, 7, 16), (6, 3, 5)):
        i = u * Neg + j
        w = oracle.philox4x32_10((i >> 2, (0 << 16) | k, stream, 0), key)[i & 3]
        assert int(utt[k - 1, u, j]) == w % Utt
    for k, s, u, j, t in ((1, 0, 0, 0, 0), (3, 7, 7, 16, 63), (6, 2, 5, 9, 31)):
        i = ((s * Utt + u) * Neg + j) * L + t
        w = oracle.philox4x32_10((i >> 2, (1 << 16) | k, stream, 0), key)[i & 3]
        assert int(seq[k - 1, s, u, j, t]) == (1 + w % (L - 1) + t) % L


# ------------------------------------------------------------------ fixtures mean what the ABI comment says
@pytest.mark.parametrize("name", FULL_CASES)
def test_f64_restatement_reproduces_reference(name):
    g = load_case(name)
    sd, z, c = case_inputs(g, name)
    r = f64_cpc(z.numpy(), c.numpy(), sd, g["utt"], g["seq"])
    assert np.abs(r["step_loss"] - g["step_loss64"]).max() <= 1e-12 * np.abs(g["step_loss64"]).max()
    assert abs(r["loss"] - float(g["loss64"])) <= 1e-12 * abs(float(g["loss64"]))
    ref_err, tol_max = float(g["ref_err"]), float(g["tol_max"])
    assert abs((ref_err + 1.5e-7 * r["mag"]).max() - tol_max) <= 1e-12 * tol_max
    margin64 = r["f"][:, :, 0] - r["f"][:, :, 1:].max(axis=2)
    sure = (g["margin"] == 0) | (np.abs(g["margin"]) > 2 * tol_max)
    assert np.array_equal((margin64 >= 0)[sure], g["correct"][sure])
    assert np.array_equal(g["correct"], g["margin"] >= 0)
    assert np.allclose(g["correct"].reshape(g["K"], -1).mean(1), g["accuracies"], atol=1e-7)
    # the conditions the GPU accuracy check rests on hold for the reference alone
    near = (g["margin"] != 0) & (np.abs(g["margin"]) <= 2 * tol_max)
    assert all(near[k].mean() <= NEAR_TIE_CAP for k in range(g["K"]))
    assert not bool((g["seq"] == np.arange(g["L"])).any()) and g["utt"].max() < g["Utt"] and g["seq"].max() < g["L"]
    print(f"{name}: share of negatives bit-equal to their positive {float(g['share_equal_negatives']):.4f}, exact-tie positions "
          f"{float(g['share_ties']):.4f}, near-tie positions {int(near.sum())}, ref_err {ref_err:.3g}, tol_max {tol_max:.3g}")


def test_ties_case_holds_exact_ties():
    g = load_case("ties")
    assert (g["margin"] == 0).mean() >= 0.10                            # the tie rule cannot pass by luck
    assert g["correct"][g["margin"] == 0].all()                        # first maximum: a tie is correct (model.py:307)


def test_e2e_fixture_shares_the_train_draws():
    g, t = load_case("train_e2e"), load_case("train_shape")
    assert np.array_equal(g["utt"], t["utt"]) and np.array_equal(g["seq"], t["seq"])
    assert g["step_loss"].shape == (6,) and g["accuracies"].shape == (6,) and g["n_near_1e5"].shape == (6,)


def test_fixture_sizes():
    biggest_before = os.path.getsize(os.path.join(GOLD, "encoder_c2_init.npz"))
    for f in os.listdir(GOLD):
        if f.startswith("cpc_"):
            assert os.path.getsize(os.path.join(GOLD, f)) < biggest_before, f


# ------------------------------------------------------------------ ABI
def test_abi_additions():
    for name in ("vqcpc_cpc_create", "vqcpc_cpc_destroy", "vqcpc_cpc_score"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)


def test_kernel_source_has_no_float_atomics_or_spin_waits():
    text = open(os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", "cpc.hip")).read()
    code = re.sub(r"//.*", "", text)
    assert not re.search(r"atomic|while\s*\((?!0\))|s_sleep|memrealtime", code)


# ------------------------------------------------------------------ driver
class _Scorer:
    """Stand-in for Encoder / CPCLoss: records what it is called with."""

    def __init__(self, S, U, n_pred):
        self.n_speakers_per_batch, self.n_utterances_per_speaker = S, U
        self.conf = V.ConfCPC(n_pred, S, U, 3, 64, 256)
        self.calls = []

    def encode(self, mels):
        self.calls.append(("enc", tuple(mels.shape), mels[:, 0, 0].clone()))
        return mels[:, :1, ::2], mels[:, :2, ::2], torch.tensor(0.5), torch.tensor(10.0 * len(self.calls))

    def __call__(self, z, c, seed, stream_id):
        self.calls.append(("cpc", tuple(z.shape), seed, stream_id))
        return torch.tensor(float(stream_id + 1)), [0.25 * (stream_id + 1), 0.5]


def test_score_batches_grouping_and_skipping():
    S, U, n_pred, frames = 2, 2, 4, 8
    need = frames + n_pred
    mk = lambda tag, T: torch.full((80, T), float(tag)) + torch.arange(T) * 1e-3
    data = {
        "a": [mk(1, 40), mk(2, need - 1), mk(3, need)],          # the short one is passed over, two remain
        "b": [mk(4, 11), mk(5, 30)],                              # one long-enough utterance: skipped, and named
        "c": [mk(6, 20), mk(7, 21), mk(8, 22)],                   # three: the first two are used
        "d": [mk(9, 25), mk(10, 26)],
        "e": [mk(11, 30), mk(12, 31)],                            # left over: no whole batch
        "f": [],
    }
    groups, skipped, left = driver.score_groups({k: [m.shape[1] for m in v] for k, v in data.items()}, S, U, need)
    assert groups == [[("a", [0, 2]), ("c", [0, 1])], [("d", [0, 1]), ("e", [0, 1])]]
    assert skipped == ["b", "f"] and left == []
    del data["e"]
    sc = _Scorer(S, U, n_pred)
    r = driver.score_batches(sc.encode, sc, data, sample_frames=frames, seed=13, device="cpu")
    assert r["batches"] == 1 and r["utterances"] == 4 and r["speakers_skipped"] == ["b", "f"] and r["speakers_left_over"] == ["d"]
    assert [c[0] for c in sc.calls] == ["enc", "cpc"] and sc.calls[0][1] == (4, 80, need) and sc.calls[1][2:] == (13, 0)
    starts = driver.cut_positions(13, 0, [40, need, 20, 21], need)
    assert starts[1] == 0 and all(0 <= s <= T - need for s, T in zip(starts, [40, need, 20, 21]))
    assert starts == driver.cut_positions(13, 0, [40, need, 20, 21], need) != driver.cut_positions(13, 1, [40, need, 20, 21], need)
    want = torch.tensor([1.0, 3.0, 6.0, 7.0]) + torch.tensor(starts) * 1e-3
    assert torch.allclose(sc.calls[0][2], want, atol=1e-6)         # speaker-major order, cut where the protocol says
    assert r["cpc_loss"] == 1.0 and r["vq_loss"] == 0.5 and r["accuracies"] == [0.25, 0.5]
    data["e"] = [mk(11, 30), mk(12, 31)]
    sc = _Scorer(S, U, n_pred)
    r = driver.score_batches(sc.encode, sc, data, sample_frames=frames, seed=13, device="cpu")
    assert r["batches"] == 2 and r["cpc_loss"] == 1.5 and r["accuracies"] == [0.375, 0.5] and r["speakers_left_over"] == []
    assert [c[3] for c in sc.calls if c[0] == "cpc"] == [0, 1]     # stream id = batch number
