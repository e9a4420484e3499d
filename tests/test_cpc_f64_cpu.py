"""CPU-side conditions of the CPC float64 cases (tests/cpc_cases.py, run on the GPU by tests/test_gpu_cpc_f64.py): the reference
alone -- float64 ``f64_cpc`` and the same statements in fp32 numpy -- meets every bound the GPU is held to, the cases reach what
they are there to reach, and ``f64_cpc`` reproduces the reference project's ``CPCLoss(...).double()`` at the new shapes
(``tests/golden/cpc_f64_pins.npz``, written by ``tools/gen_cpc_golden.py --pins``)."""
import os

import numpy as np
import pytest

import cpc_cases
from test_cpc_cpu import GOLD, NEAR_TIE_CAP

ALL = [(n, None) for n in cpc_cases.CASES] + [("partials", cpc_cases.SHRINK_T)]      # the short call of the workspace test too


@pytest.mark.parametrize("name,T", ALL)
def test_reference_alone_meets_the_bounds(name, T):
    ref = cpc_cases.reference(name, T)
    r64, r32, K = ref["r64"], ref["r32"], ref["K"]
    assert r64["f"].shape == (K, ref["N"], ref["J"], ref["L"]) and r64["pos_loss"].shape == (K, ref["N"], ref["L"])
    assert np.array_equal(r64["pos_loss"].reshape(K, -1).mean(axis=1), r64["step_loss"])

    # the fp32 restatement uses at most half of the score bound's 1.5e-7 mag part, everywhere
    ratio = (np.abs(r32["f"].astype(np.float64) - r64["f"]) / (1.5e-7 * r64["mag"])).max()
    # its step losses are inside the end-to-end loss bound
    s3 = cpc_cases.stage3(r32["f"])
    step32 = r32["step_loss"].astype(np.float64)
    bound = cpc_cases.loss_bound(ref, s3, step32)
    e2e = np.abs(step32 - r64["step_loss"])
    near, ties = ref["near"], ref["margin64"] == 0
    print(f"\n{name}{'' if T is None else f' at T = {T}'}: max(|f32 - f64| / (1.5e-7 mag)) = {ratio:.4f}, err32 = {ref['err32']:.3g}, "
          f"tol_max = {ref['tol_max']:.3g}, max|f64| = {np.abs(r64['f']).max():.4g}; max(|step_loss32 - step_loss64| / bound) = "
          f"{(e2e / bound).max():.4f} (max error {e2e.max():.3g}); exact-tie positions {int(ties.sum())}, near-tie positions "
          f"{int(near.sum())} of {near.size}; step_loss64 {r64['step_loss'].min():.4f} .. {r64['step_loss'].max():.4f}, "
          f"log(1 + Neg) = {np.log(ref['J']):.4f}")
    assert ratio <= 0.5
    assert (e2e <= bound).all()
    assert all(near[k].mean() <= NEAR_TIE_CAP for k in range(K))
    # a float64 tie is a tie of bit-equal rows, and is correct on the fp32 side too
    assert s3["ok"][ties].all()
    assert np.array_equal(s3["ok"][~near], (ref["margin64"] >= 0)[~near])


def test_peaked_stresses_the_softmax():
    ref = cpc_cases.reference("peaked")
    f = ref["r64"]["f"]
    share = (f.max(axis=2) > 88.8).mean()                  # expf(f) overflows in fp32 above 88.72
    print(f"\npeaked: share of positions whose row maximum exceeds 88.8 = {share:.4f}, max|f64| = {np.abs(f).max():.4g}, "
          f"step_loss64 = {np.round(ref['r64']['step_loss'], 3).tolist()}")
    assert share >= 0.01
    assert np.abs(f).max() > 100
    assert (ref["r64"]["step_loss"] > 10 * np.log(1 + ref["Neg"])).all()


def test_cases_reach_what_they_are_for():
    g = cpc_cases.case("partials")
    P = g["N"] * -(-g["L"] // 16)
    assert P == 595 and P > 512 and P % 256 != 0           # two or three partials per thread of the finish kernel
    g = cpc_cases.case("c64_min")
    assert g["L"] == 2 and g["Neg"] == 1 and g["c_dim"] == 64 and g["T"] == g["K"] + 2
    g = cpc_cases.case("c512_neg64")
    assert g["c_dim"] == 512 and g["J"] * 16 == 4 * 256 + 16 and g["L"] % 16 == 1      # five pair passes, the last with 16 live pairs
    g = cpc_cases.case("steps16")
    assert g["K"] == 16 and g["L"] == 15
    g = cpc_cases.case("partials", cpc_cases.SHRINK_T)
    assert g["L"] == 2 and g["T"] == g["K"] + 2


def test_edges_index_arrays():
    g = cpc_cases.case("edges")
    utt, seq = (a.numpy() for a in cpc_cases.edges_negatives(g))
    K, Spk, Utt, Neg, L = g["K"], g["Spk"], g["Utt"], g["Neg"], g["L"]
    assert utt.shape == (K, Utt, Neg) and seq.shape == (K, Spk, Utt, Neg, L) and utt.dtype == seq.dtype == np.int64
    assert utt.min() == 0 and utt.max() == Utt - 1 and seq.min() == 0 and seq.max() == L - 1
    t = np.arange(L)
    assert (seq[:, :, :, 0::2] == L - 1 - t).all()
    assert (seq[:, :, :, 1::2, 0::2] == 0).all() and (seq[:, :, :, 1::2, 1::2] == L - 1).all()
    assert (utt[:, :, 0] == Utt - 1).all() and (utt[:, :, 1] == 0).all() and (utt[:, :, 2:] == (Utt - 1 - np.arange(Utt))[None, :, None]).all()
    # negative 0 of anchor 0 at the last step reads the very last row of z: ((Spk - 1) Utt + Utt - 1) T + (L - 1) + K = N T - 1
    assert (seq[K - 1, Spk - 1, :, 0, 0] == L - 1).all() and (utt[K - 1, :, 0] == Utt - 1).all() and L - 1 + K == g["T"] - 1
    assert (seq[:, :, :, :, L - 1] == 0).all()             # and the last anchor reads the first frame a step may use


@pytest.mark.parametrize("name", cpc_cases.PROTOCOL_CASES)
def test_f64_restatement_reproduces_reference_at_the_new_shapes(name):
    pins = np.load(os.path.join(GOLD, "cpc_f64_pins.npz"))
    ref = cpc_cases.reference(name)
    want, acc = pins[f"{name}_step_loss64"], pins[f"{name}_accuracy"]
    assert want.shape == acc.shape == (ref["K"],) and want.dtype == np.float64
    got = ref["r64"]["step_loss"]
    print(f"\n{name}: max relative |step_loss64 - reference's| = {(np.abs(got - want) / np.abs(want)).max():.3g}")
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()
    assert np.allclose((ref["margin64"] >= 0).reshape(ref["K"], -1).mean(axis=1), acc, atol=1e-7)
