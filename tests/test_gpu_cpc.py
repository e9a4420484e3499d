"""-m gpu: CPC scoring (``CPCLoss`` through ``vqcpc_cpc_score``) against the reference's recorded results
(``tests/golden/cpc_*.npz``, ``tools/gen_cpc_golden.py``) and a float64 restatement with the reference's own draws.

Yardsticks (none of them measured on the code under test):
* scores: ``|f_gpu - f64| <= ref_err + 1.5e-7 (sum_d |z_d| (|W_k| |c| + |b_k|)_d + sum_d |z_d Wc_d|) / 8`` -- the error of an
  fp32 fma chain against float64 for the 256-term predictor product carried through the dot with ``z``, the 64-term dot's
  own, plus the reference's own fp32 distance from float64 on the same case;
* losses: ``ref_loss_err + tol_max + 1e-6 |loss64|``;
* per-position ``correct``: equal to the reference's wherever its margin is exactly 0 (a tie is correct) or larger than
  ``2 tol_max``; the positions in between are listed and may number at most 0.5 % of a case's positions.
"""
import numpy as np
import pytest
import torch

import vectorquantizedcpc_amd as V
from test_cpc_cpu import FULL_CASES, NEAR_TIE_CAP, case_inputs, f64_cpc, load_case
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu


def module_for(g, device="cuda"):
    cpc = V.CPCLoss(V.ConfCPC(g["n_pred"], g["Spk"], g["Utt"], g["Neg"], 64, g["c_dim"]))
    cpc.load_state_dict(synth.cpc_state_dict(n_prediction_steps=g["n_pred"], c_dim=g["c_dim"]))
    return cpc.to(device).eval()


def bits(t):
    return t.reshape(-1).view(torch.uint8)


def set_at(t, index, value):
    t = t.clone()
    t[index] = value
    return t


def negatives_of(g):
    return torch.from_numpy(g["utt"]), torch.from_numpy(g["seq"])


@pytest.mark.parametrize("name", FULL_CASES)
def test_scores_loss_and_accuracy_against_reference(name):
    g = load_case(name)
    sd, z, c = case_inputs(g, name)
    want = f64_cpc(z.numpy(), c.numpy(), sd, g["utt"], g["seq"])
    cpc = module_for(g)
    r = cpc.forward_detailed(z.cuda(), c.cuda(), negatives=negatives_of(g), want_correct=True, want_scores=True)
    ref_err, tol_max = float(g["ref_err"]), float(g["tol_max"])

    # scores
    f = r["scores"].cpu().numpy().astype(np.float64)
    err = np.abs(f - want["f"])
    tol = ref_err + 1.5e-7 * want["mag"]
    print(f"\n{name}: max(|f_gpu - f64| / tol) = {(err / tol).max():.4f}   max|f_gpu - f64| / ref_err = {err.max() / ref_err:.4f}   "
          f"(max|f_gpu - f64| = {err.max():.3g}, ref_err = {ref_err:.3g}, tol_max = {tol_max:.3g})")
    assert (err <= tol).all()
    rows = r["scores"].cpu().numpy()[:, :: max(1, g["N"] // 2)][:, :2][..., [0, g["L"] - 1]]
    assert np.abs(rows - g["rows_scores"]).max() <= 2 * tol_max                  # the reference's fp32 rows themselves

    # losses
    loss, step = float(r["loss"]), r["step_loss"].cpu().numpy().astype(np.float64)
    bound = float(g["ref_loss_err"]) + tol_max + 1e-6 * abs(float(g["loss64"]))
    print(f"{name}: |loss_gpu - loss64| = {abs(loss - float(g['loss64'])):.3g}  max|step_loss_gpu - step_loss64| = "
          f"{np.abs(step - g['step_loss64']).max():.3g}  (bound {bound:.3g}; the reference's own |loss32 - loss64| = {float(g['ref_loss_err']):.3g})")
    assert abs(loss - float(g["loss64"])) <= bound
    assert (np.abs(step - g["step_loss64"]) <= float(g["ref_loss_err"]) + tol_max + 1e-6 * np.abs(g["step_loss64"])).all()

    # accuracy, position by position
    correct = r["correct"].cpu().numpy().astype(bool)
    sure = (g["margin"] == 0) | (np.abs(g["margin"]) > 2 * tol_max)
    differ = np.argwhere(correct != g["correct"])
    print(f"{name}: exact-tie positions {int((g['margin'] == 0).sum())}, near-tie positions (0 < |margin| <= 2 tol_max) "
          f"{int((~sure).sum())} of {sure.size}: {np.argwhere(~sure).tolist()}; positions where correct differs: {differ.tolist()}")
    assert np.array_equal(correct[sure], g["correct"][sure])
    assert correct[g["margin"] == 0].all()
    assert (~sure).sum() <= NEAR_TIE_CAP * sure.size
    acc = r["accuracy"].cpu().numpy()
    assert np.array_equal(acc, correct.reshape(g["K"], -1).sum(1).astype(np.float32) / np.float32(g["N"] * g["L"]))
    assert (np.abs(acc - g["accuracies"]) <= ((~sure).reshape(g["K"], -1).sum(1) + 1e-3) / (g["N"] * g["L"])).all()

    # the public call returns the reference's types
    out_loss, accs = cpc(z.cuda(), c.cuda(), negatives=negatives_of(g))
    assert out_loss.dim() == 0 and out_loss.is_cuda and not out_loss.requires_grad and isinstance(accs, list)
    assert float(out_loss) == loss and accs == [float(a) for a in acc]


@pytest.mark.parametrize("name,seed,stream", [("train_shape", 13, 0), ("small_odd", (7 << 32) | 5, 3), ("ties", 1, 1), ("one_utt", 13, 2)])
def test_protocol_mode_equals_explicit_indices_bit_for_bit(name, seed, stream):
    g = load_case(name)
    _, z, c = case_inputs(g, name)
    cpc = module_for(g)
    a = cpc.forward_detailed(z.cuda(), c.cuda(), seed=seed, stream_id=stream, want_correct=True, want_scores=True)
    neg = synth.cpc_negatives(seed, stream, g["K"], g["Spk"], g["Utt"], g["Neg"], g["L"])
    b = cpc.forward_detailed(z.cuda(), c.cuda(), negatives=neg, want_correct=True, want_scores=True)
    for key in ("loss", "step_loss", "accuracy", "correct", "scores"):
        assert torch.equal(bits(a[key]), bits(b[key])), key
    other = cpc.forward_detailed(z.cuda(), c.cuda(), seed=seed, stream_id=stream + 1)
    assert not torch.equal(other["step_loss"], a["step_loss"])


def test_repeatable_streams_and_devices():
    g = load_case("train_shape")
    _, z, c = case_inputs(g, "train_shape")
    cpc = module_for(g, "cuda:0")
    z, c = z.to("cuda:0"), c.to("cuda:0")
    a = cpc.forward_detailed(z, c, want_correct=True, want_scores=True)
    b = cpc.forward_detailed(z, c, want_correct=True, want_scores=True)
    for key in a:
        assert torch.equal(bits(a[key]), bits(b[key])), key
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        d = cpc.forward_detailed(z, c, want_correct=True)
    s.synchronize()
    assert torch.equal(d["step_loss"], a["step_loss"]) and torch.equal(d["correct"], a["correct"])
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            e = cpc.forward_detailed(z, c, want_correct=True)
        assert torch.equal(e["step_loss"], a["step_loss"]) and torch.equal(e["correct"], a["correct"])
    # the handle follows the parameters
    cpc.load_state_dict(synth.cpc_state_dict(seed=14))
    assert not torch.equal(cpc.forward_detailed(z, c)["step_loss"], a["step_loss"])
    cpc.load_state_dict(synth.cpc_state_dict())
    assert torch.equal(cpc.forward_detailed(z, c)["step_loss"], a["step_loss"])


def test_end_to_end_against_reference_encoder_and_cpc():
    """``train_e2e``: this project's ``Encoder.forward`` -> ``CPCLoss`` with the reference's draws, against the reference's
    ``Encoder.forward`` -> ``CPCLoss.forward``.  1e-5 is the project's teacher-forced tolerance, not a value measured here."""
    g = load_case("train_e2e")
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict(ln_affine="random", codebook="data"))
    enc = enc.cuda().eval()
    z, c, _, _ = enc(synth.mel(str(g["mel"]), 64, 140).cuda())
    cpc = module_for(g)
    r = cpc.forward_detailed(z, c, negatives=negatives_of(g))
    step, acc = r["step_loss"].cpu().numpy().astype(np.float64), r["accuracy"].cpu().numpy().astype(np.float64)
    ref_step, ref_acc = g["step_loss"].astype(np.float64), g["accuracies"].astype(np.float64)
    positions = g["N"] * g["L"]
    print(f"\ntrain_e2e: |step_loss - ref| = {np.abs(step - ref_step).tolist()}  |loss - ref| = {abs(float(r['loss']) - float(g['loss'])):.3g}  "
          f"|accuracy - ref| * positions = {(np.abs(acc - ref_acc) * positions).round(2).tolist()} "
          f"(allowed {(g['n_near_1e5'] + 1).tolist()} of {positions})")
    assert (np.abs(step - ref_step) <= 1e-5 * np.maximum(1.0, np.abs(ref_step))).all()
    assert (np.abs(acc - ref_acc) <= (g["n_near_1e5"] + 1) / positions + 1e-7).all()


def test_error_surface():
    g = load_case("small_odd")
    _, z, c = case_inputs(g, "small_odd")
    z, c = z.cuda(), c.cuda()
    cpc = module_for(g)
    good = cpc.forward_detailed(z, c, negatives=negatives_of(g))["step_loss"].clone()
    with pytest.raises(RuntimeError, match=r"expected z of shape \(6, T, 64\)"):
        cpc(z[:5], c[:5])
    with pytest.raises(RuntimeError, match=r"expected z of shape"):
        cpc(z, c[:, :, :64])
    with pytest.raises(RuntimeError, match=r"expected T >= 4"):
        cpc(z[:, :3], c[:, :3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpc(z.cpu(), c.cpu())
    utt, seq = negatives_of(g)
    for bad_utt, bad_seq in ((utt, set_at(seq, (0, 0, 0, 0, 0), g["L"])), (utt, set_at(seq, (1, 2, 1, 6, 16), -1)),
                             (set_at(utt, (0, 0, 0), g["Utt"]), seq)):
        with pytest.raises(IndexError, match="outside"):
            cpc(z, c, negatives=(bad_utt, bad_seq))
    with pytest.raises(RuntimeError, match="int64 tensor of shape"):
        cpc(z, c, negatives=(utt, seq[:, :, :, :, :-1]))
    assert torch.equal(cpc.forward_detailed(z, c, negatives=negatives_of(g))["step_loss"], good)     # the next call is fine
    for conf in ((12, 8, 8, 65, 64, 256), (12, 8, 8, 17, 32, 256), (12, 8, 8, 17, 64, 96), (34, 8, 8, 17, 64, 256)):
        bad = V.CPCLoss(V.ConfCPC(*conf)).cuda()
        with pytest.raises(RuntimeError):
            bad(torch.zeros(64, 70, conf[4], device="cuda"), torch.zeros(64, 70, conf[5], device="cuda"))
