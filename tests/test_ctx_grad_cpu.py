"""CPU-side checks of the context-LSTM gradients: the float64 reference of tests/ctx_grad_ref.py against its pins
(tests/golden/ctx_grad_pins.npz), the judge held by an fp32 numpy restatement in the kernels' documented order and by a differently
ordered one (so the bound is shown passable before a GPU is involved, and rests on nothing the GPU does), the ABI addition and the
command line.

The wide cases (tests/golden/ctx_grad_wide_pins.npz): their pins, the condition that the fp32 reference has kept its digits, both
restatements under the whole-tensor and the per-step judge, and four faults seeded into the restatement that the judges must
notice -- among them a scan that stops propagating 30 steps from the end, which the whole-tensor judge alone lets pass."""
import os
import re

import numpy as np
import pytest
import torch

import cpc_grad_ref
import ctx_grad_ref as R
import grad_judge
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, cli, driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("vqcpc_encoder_context_saved_bytes", "vqcpc_encoder_context_fwd", "vqcpc_encoder_context_bwd")


# ------------------------------------------------------------------ reference
@pytest.mark.parametrize("name", R.ALL_CASES + [R.CHAIN])
def test_pins_reproduce_from_the_float64_reference(name):
    ref = R.grads64(name)
    grad_judge.check_pins(ref, R.pins(), name, list(ref), R.POSITIONS)


@pytest.mark.parametrize("name", R.ALL_CASES)
def test_kernel_order_fp32_restatement_stays_within_the_judge(name):
    R.judge(name, R.kernel_order32(name), "kernel-order fp32 numpy")


@pytest.mark.parametrize("name", R.ALL_CASES)
def test_reordered_fp32_restatement_stays_within_the_judge(name):
    R.judge(name, R.reordered32(name), "reordered fp32 numpy")


def test_kernel_order_restatement_of_the_chain_stays_within_the_judge():
    """The composition with the CPC loss: dc from float64 autograd of the loss at the restatement's own fp32 c."""
    g = R.chain_case()
    c32 = R.kernel_order32(R.CHAIN, grad_c=np.zeros(g["c"].shape, np.float32))["c"]
    c = torch.from_numpy(c32).double().requires_grad_(True)
    cpc_grad_ref.loss_torch(g["z"].double(), c, g["W"].double(), g["b"].double(), g["rows"])[0].backward()
    got = R.kernel_order32(R.CHAIN, grad_c=c.grad.numpy().astype(np.float32))
    R.judge(R.CHAIN, {k: got[k] for k in ("c", "W_ih", "W_hh", "b")}, "kernel-order fp32 numpy")


def test_structure_of_the_reference():
    assert not R.grads64("t1")["W_hh"].any()                         # no previous step: h_prev is zero
    assert all(R.grads64("t1")[k].any() for k in ("z", "W_ih", "b"))


# ------------------------------------------------------------------ the wide cases (tests/golden/ctx_grad_wide_pins.npz)
@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_pins_reproduce_from_the_float64_reference(name):
    ref, p = R.grads64(name), R.pins()
    T = R.load(name)["T"]
    grad_judge.check_pins(ref, p, name, list(ref), R.POSITIONS)
    for k in R.STEP_TENSORS:
        steps, e_ref = p[f"{name}_{k}_step_max"], p[f"{name}_{k}_step_e_ref"]
        assert steps.shape == e_ref.shape == (T,)
        assert (np.abs(R.step_max(ref[k]) - steps) <= 1e-12 * steps).all(), k      # step by step: a zero step is pinned as zero
        assert steps.max() == float(p[f"{name}_{k}_max"]) and e_ref.max() == float(p[f"{name}_{k}_e_ref"]), k


def test_structure_of_the_wide_cases():
    """The table of the cases holds what it says: tiles, slabs, and the shape of the upstream gradient and of dz."""
    rows = {n: R.load(n)["B"] * R.load(n)["T"] for n in R.ALL_WIDE}
    assert rows["slab_exact"] == 1024 and rows["slab_plus_one"] == 1025 and rows["b130"] == 5 * 1024 + 80 and rows["h64_slabs"] > 12 * 1024
    assert all(R.load(n)["D"] == 64 for n in R.ALL_WIDE)
    p = R.pins()
    for n in ("tail", "tail_stressed", "tail_h64"):
        G, dz = R.load(n)["G"], p[f"{n}_z_step_max"]
        assert not G[:, :-1].any() and G[:, -1].all()
        assert dz.argmax() == len(dz) - 1 and dz.argmin() == 0 and dz.min() > 0.0
    assert p["tail_z_step_max"][0] < 1e-11 * p["tail_z_step_max"][-1] and p["tail_z_step_max"][0] > 1e-20     # far above fp32's subnormals
    assert p["tail_stressed_z_step_max"][0] < 1e-3 * p["tail_stressed_z_step_max"][-1]
    G, dz = R.load("cpc_shaped")["G"], p["cpc_shaped_z_step_max"]
    assert G[:, :64].all() and not G[:, 64:].any() and dz[:64].all() and not dz[64:].any()
    g = R.load("long_stressed")
    plain = R.lstm_weights("long_stressed", 64, 256)
    H = g["H"]
    lift = torch.zeros(4 * H)
    lift[H:2 * H] = 3.0
    assert torch.equal(g["w_ih"], plain["w_ih"] * 8) and torch.equal(g["w_hh"], plain["w_hh"]) and torch.equal(g["b_hh"], plain["b_hh"] * 8)
    assert torch.equal(g["b_ih"], plain["b_ih"] * 8 + lift)


@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_fp32_reference_of_the_wide_cases_has_not_drifted(name):
    """The condition on the inputs: e_ref <= 1e-5 max |G64| for every tensor, so the judge's bound is a statement about fp32 and not
    about a reference that lost its digits."""
    p = R.pins()
    for k in R.TENSORS:
        e_ref, top = float(p[f"{name}_{k}_e_ref"]), float(p[f"{name}_{k}_max"])
        print(f"{name} {k}: e_ref / max|G64| = {e_ref / top:.3g}")
        assert 0.0 < e_ref <= 1e-5 * top, (k, e_ref, top)


def both_judges(name, got, what):
    R.judge(name, got, what)
    R.judge_steps(name, got, what)


@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_reordered_fp32_restatement_stays_within_both_judges(name):
    both_judges(name, R.reordered32(name), "reordered fp32 numpy")


@pytest.mark.parametrize("name", [n for n in R.ALL_WIDE if R.WIDE_CASES[n][1] <= 500])      # at T = 3000 its loops take most of a minute
def test_kernel_order_fp32_restatement_stays_within_both_judges(name):
    both_judges(name, R.kernel_order32(name), "kernel-order fp32 numpy")


# ------------------------------------------------------------------ would the judges notice?  Faults seeded into the restatement
def fails(judge, name, got, what):
    try:
        judge(name, got, what)
    except AssertionError as e:
        print(f"{what} {name}: {judge.__name__} fails: {e}")
        return True
    return False


def test_a_scan_that_stops_propagating_passes_the_whole_tensor_judge_and_fails_the_per_step_one():
    """The gap the per-step judge closes, in one assertion: the recurrent term dropped for t < T - 30 on ``tail``."""
    got = R.reordered32("tail", fault="drop_rec")
    R.judge("tail", got, "dh_rec dropped for t < T - 30:")                           # the largest elements are all at late steps
    assert fails(R.judge_steps, "tail", got, "dh_rec dropped for t < T - 30:")


def test_flushed_small_dA_values_are_noticed():
    got = R.reordered32("tail_stressed", fault="flush_small")
    fails(R.judge, "tail_stressed", got, "dA below 1e-6 of its maximum flushed:")    # printed, not required: the values are small
    assert fails(R.judge_steps, "tail_stressed", got, "dA below 1e-6 of its maximum flushed:")


def test_masked_columns_that_carry_column_0_are_noticed():
    got = R.reordered32("b130", fault="masked_reads_col0")
    R.judge_steps("b130", got, "masked columns carry utterance 0:")                  # c and dz of a live column do not see them
    assert fails(R.judge, "b130", got, "masked columns carry utterance 0:")          # the sums over rows do


def test_a_skipped_short_last_slab_is_noticed():
    got = R.reordered32("slab_plus_one", fault="skip_short_slab")
    assert fails(R.judge, "slab_plus_one", got, "last slab of one row skipped:")


# ------------------------------------------------------------------ ABI
def test_abi_addition():
    text = open(os.path.join(ROOT, "include", "vqcpc.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    for cite in ("model.py:57", ":69", ":85", "train_cpc.py:116-124"):
        assert cite in text, cite


def test_kernel_source_has_no_atomics_or_spin_waits():
    for name in ("context_grad.hip", "seq_step.h", "grad_slab.h"):
        text = open(os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", name)).read()
        code = re.sub(r"//.*", "", text)
        assert not re.search(r"atomic|while\s*\((?!0\))|s_sleep|memrealtime|asm", code), name


# ------------------------------------------------------------------ module surface and command line
def test_context_has_no_cpu_fallback():
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.context(torch.zeros(2, 5, 64), differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.context(torch.zeros(2, 5, 64))
    assert "context LSTM have no backward" not in " ".join(V.CPCLoss.__doc__.split())


def test_cli_fit_context_help_parses(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["fit-context", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert "--out-checkpoint" in text and "--steps" in text and "--freeze-predictors" in text


class _Enc(torch.nn.Module):
    """Stand-in for Encoder in ``fit_context``: ``rnn`` is one weight, ``context`` a plain function of it."""

    def __init__(self):
        super().__init__()
        self.rnn = torch.nn.Linear(1, 1, bias=False)
        self.calls = []

    def forward(self, mels):
        self.calls.append(("enc", torch.is_grad_enabled()))
        return mels[:, :1, ::2], mels[:, :2, ::2], torch.tensor(0.5), torch.tensor(10.0)

    def context(self, z, *, differentiable=False):
        self.calls.append(("ctx", differentiable, torch.is_grad_enabled()))
        return z * self.rnn.weight[0, 0]


class _Cpc(torch.nn.Module):
    def __init__(self, S, U, n_pred):
        super().__init__()
        self.n_speakers_per_batch, self.n_utterances_per_speaker, self.n_prediction_steps = S, U, n_pred // 2
        self.conf = V.ConfCPC(n_pred, S, U, 3, 64, 256)
        self.predictors = torch.nn.ModuleList([torch.nn.Linear(2, 1) for _ in range(n_pred)])

    def forward(self, z, c, seed, stream_id, differentiable=False):
        assert differentiable and c.requires_grad
        return (c ** 2).mean() + sum((p.weight ** 2).sum() for p in self.predictors[:self.n_prediction_steps]), [0.5]


def test_fit_context_wiring():
    S, U, n_pred, frames = 2, 2, 4, 8
    mk = lambda tag, T: torch.full((80, T), 0.05 * tag) + torch.arange(T) * 1e-3
    data = {"a": [mk(1, 40), mk(2, 30)], "b": [mk(4, 21), mk(5, 30)], "c": [mk(6, 20), mk(7, 21)], "d": [mk(9, 25), mk(10, 26)]}
    for train_predictors in (True, False):
        enc, cpc = _Enc(), _Cpc(S, U, n_pred)
        made = []
        before = [p.weight.detach().clone() for p in cpc.predictors]
        r = driver.fit_context(enc, cpc, data, steps=5, lr=0.1, optimizer=lambda ps, lr: (made.append([id(p) for p in ps]),
                               torch.optim.SGD(ps, lr=lr))[1], sample_frames=frames, seed=13, device="cpu", train_predictors=train_predictors)
        K = n_pred // 2
        want = [id(p) for p in enc.rnn.parameters()] + ([id(p) for m in cpc.predictors[:K] for p in m.parameters()] if train_predictors else [])
        assert made == [want]
        assert set(r) == {"losses", "accuracies", "steps", "batches", "utterances", "speakers_skipped", "speakers_left_over"}
        assert r["steps"] == 5 and r["batches"] == 2 and all(a > b for a, b in zip(r["losses"], r["losses"][2:]))
        assert [c for c in enc.calls if c[0] == "enc"] == [("enc", False)] * 2             # front end once per batch, no_grad
        assert [c for c in enc.calls if c[0] == "ctx"] == [("ctx", True, True)] * 5        # the context every step, differentiable
        for k, p in enumerate(cpc.predictors):
            assert torch.equal(p.weight, before[k]) != (train_predictors and k < K)


def test_fitted_checkpoint_with_an_encoder_update(tmp_path):
    from vectorquantizedcpc_amd import io, synth
    src, out = tmp_path / "in.pt", tmp_path / "out.pt"
    cpc_sd = synth.cpc_state_dict()
    torch.save({"encoder": {"w": torch.arange(3.0), "rnn.weight_ih_l0": torch.zeros(2)}, "cpc": cpc_sd, "epoch": 3}, src)
    io.save_fitted_checkpoint(out, cpc_sd, src, encoder_update={"rnn.weight_ih_l0": torch.ones(2)})
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["epoch"] == 3 and torch.equal(ck["encoder"]["w"], torch.arange(3.0)) and torch.equal(ck["encoder"]["rnn.weight_ih_l0"], torch.ones(2))
    with pytest.raises(KeyError):
        io.save_fitted_checkpoint(out, cpc_sd, src, encoder_update={"rnn.nope": torch.ones(2)})
