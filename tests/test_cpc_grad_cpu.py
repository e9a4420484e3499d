"""CPU-side checks of the CPC gradients: the float64 reference of tests/cpc_grad_ref.py against what the reference project's
autograd recorded (tests/golden/cpc_grad_pins.npz), the judge held by a differently ordered fp32 backward (so the bound rests on
nothing the GPU does), structural facts of the gradients, the ABI addition, the CPU-tensor error and the wiring of
``driver.fit_predictors``."""
import os
import re

import pytest
import torch

import cpc_grad_ref as R
import grad_judge
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ reference
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_pins_reproduce_from_the_float64_restatement(name):
    ref, p = R.grads64(name), R.pins()
    grad_judge.check_pins(ref, p, name, R.TENSORS, R.POSITIONS)
    assert abs(ref["loss"] - float(p[f"{name}_loss64"])) <= 1e-12 * abs(float(p[f"{name}_loss64"]))


@pytest.mark.parametrize("name", R.ALL_CASES)
def test_reordered_fp32_backward_stays_within_the_judge(name):
    R.judge(name, R.reordered32(name), "reordered fp32 numpy")


@pytest.mark.parametrize("name", ["small_odd", "edges", "long"])
def test_structure_of_the_float64_gradients(name):
    g, ref = R.load(name), R.grads64(name)
    assert not ref["z"][:, 0].any()                                  # frame 0 is neither a positive nor a negative of any step
    assert not ref["c"][:, g["L"]:].any()                            # contexts past L predict nothing
    assert ref["c"][:, :g["L"]].any() and ref["z"][:, 1:].any()
    # sum_j g_j = 0 at every position: dloss/df summed over an anchor's 1 + Neg scores
    z, c, W, b = (g[k].double() for k in R.TENSORS)
    rows = R.row_index(g)
    L = g["L"]
    for k in range(g["K"]):
        wc = torch.nn.functional.linear(c[:, :L], W[k], b[k])
        f = ((z.reshape(-1, 64)[torch.from_numpy(rows[k])] * wc[:, None]).sum(-1) / 8.0).requires_grad_(True)
        (torch.logsumexp(f, dim=1) - f[:, 0]).mean().backward()
        assert float(f.grad.sum(dim=1).abs().max()) <= 1e-15


# ------------------------------------------------------------------ ABI
def test_abi_addition():
    assert "vqcpc_cpc_grad" in _lib.SYMBOLS and hasattr(_lib.load(), "vqcpc_cpc_grad")


def test_kernel_source_has_no_atomics_or_spin_waits():
    for name in ("cpc_grad.hip", "cpc_tile.h"):
        text = open(os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", name)).read()
        code = re.sub(r"//.*", "", text)
        assert not re.search(r"atomic|while\s*\((?!0\))|s_sleep|memrealtime", code), name


# ------------------------------------------------------------------ module surface
def test_differentiable_has_no_cpu_fallback():
    cpc = V.CPCLoss(V.ConfCPC(12, 8, 8, 17, 64, 256))
    z, c = torch.zeros(64, 70, 64, requires_grad=True), torch.zeros(64, 70, 256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpc(z, c, differentiable=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cpc(z.detach(), c, differentiable=True)                      # the predictors require grad
    assert "nothing here trains" not in V.CPCLoss.__doc__


# ------------------------------------------------------------------ driver
class _Fit(torch.nn.Module):
    """Stand-in for Encoder / CPCLoss in ``fit_predictors``: records its calls; its loss is a plain function of the first K
    predictors, so the optimizer wiring shows in the numbers."""

    def __init__(self, S, U, n_pred):
        super().__init__()
        self.n_speakers_per_batch, self.n_utterances_per_speaker, self.n_prediction_steps = S, U, n_pred // 2
        self.conf = V.ConfCPC(n_pred, S, U, 3, 64, 256)
        self.predictors = torch.nn.ModuleList([torch.nn.Linear(2, 1) for _ in range(n_pred)])
        self.calls = []

    def encode(self, mels):
        self.calls.append(("enc", tuple(mels.shape), torch.is_grad_enabled()))
        return mels[:, :1, ::2], mels[:, :2, ::2], torch.tensor(0.5), torch.tensor(10.0)

    def forward(self, z, c, seed, stream_id, differentiable=False):
        self.calls.append(("cpc", tuple(z.shape), seed, stream_id, differentiable, torch.is_grad_enabled()))
        loss = sum((p.weight ** 2).sum() + (p.bias ** 2).sum() for p in self.predictors[:self.n_prediction_steps])
        return loss, [0.25 * (stream_id + 1), 0.5]


def test_fit_predictors_grouping_streams_and_optimizer_wiring():
    S, U, n_pred, frames = 2, 2, 4, 8
    need = frames + n_pred
    mk = lambda tag, T: torch.full((80, T), float(tag)) + torch.arange(T) * 1e-3
    data = {"a": [mk(1, 40), mk(2, need - 1), mk(3, need)], "b": [mk(4, 11), mk(5, 30)], "c": [mk(6, 20), mk(7, 21), mk(8, 22)],
            "d": [mk(9, 25), mk(10, 26)], "e": [mk(11, 30), mk(12, 31)], "f": [mk(13, 40), mk(14, 41)]}
    fit = _Fit(S, U, n_pred)
    before = [p.weight.detach().clone() for p in fit.predictors]
    made = []

    def optimizer(params, lr):
        made.append([id(p) for p in params])
        return torch.optim.SGD([p for p in fit.parameters() if id(p) in made[-1]], lr=lr)

    r = driver.fit_predictors(fit.encode, fit, data, steps=5, lr=0.25, optimizer=optimizer, sample_frames=frames, seed=13, device="cpu")
    K = n_pred // 2
    assert made == [[id(p) for m in fit.predictors[:K] for p in m.parameters()]]          # only the first K predictors
    assert r["speakers_skipped"] == ["b"] and r["speakers_left_over"] == ["f"] and r["batches"] == 2 and r["steps"] == 5
    cpc_calls = [c for c in fit.calls if c[0] == "cpc"]
    enc_calls = [c for c in fit.calls if c[0] == "enc"]
    assert len(cpc_calls) == 5 and len(enc_calls) == 2                  # a frozen encoder: every batch is encoded once
    assert [c[3] for c in cpc_calls] == [0, 1, 0, 1, 0]                  # stream id = batch number, the batches cycled
    assert all(c[2] == 13 and c[4] is True and c[5] is True for c in cpc_calls)           # differentiable, grad mode on
    assert all(c[1] == (S * U, 80, need) and c[2] is False for c in enc_calls)          # the encoder under no_grad
    assert len(r["losses"]) == 5 and len(r["accuracies"]) == 5 and r["accuracies"][1] == [0.5, 0.5]
    assert all(a > b for a, b in zip(r["losses"], r["losses"][1:]))      # SGD at lr 0.25 halves every parameter per step
    for k, p in enumerate(fit.predictors):
        if k < K:
            assert torch.allclose(p.weight, before[k] * 0.5 ** 5)
        else:
            assert torch.equal(p.weight, before[k]) and p.weight.grad is None
    # the same cuts as score_batches: one shared batching
    sc_calls = []
    fit3 = _Fit(S, U, n_pred)
    driver.score_batches(lambda m: (sc_calls.append(m[:, 0, 0].clone()), fit3.encode(m))[1], fit3, data, sample_frames=frames, seed=13,
                         device="cpu")
    seen = []
    fit2 = _Fit(S, U, n_pred)
    driver.fit_predictors(lambda m: (seen.append(m[:, 0, 0].clone()), fit2.encode(m))[1], fit2, data, steps=2, lr=0.1,
                          optimizer=torch.optim.SGD, sample_frames=frames, seed=13, device="cpu")
    assert len(sc_calls) == 2 and all(torch.equal(a, b) for a, b in zip(sc_calls, seen))


# ------------------------------------------------------------------ io
def test_fitted_checkpoint_replaces_cpc_and_keeps_the_rest(tmp_path):
    from vectorquantizedcpc_amd import io, synth
    src, out = tmp_path / "in.pt", tmp_path / "out.pt"
    old, new = synth.cpc_state_dict(), synth.cpc_state_dict(seed=14)
    torch.save({"encoder": {"w": torch.arange(3.0)}, "cpc": old, "epoch": 3}, src)
    io.save_fitted_checkpoint(out, new, src)
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert set(ck) == {"encoder", "cpc", "epoch"} and ck["epoch"] == 3 and torch.equal(ck["encoder"]["w"], torch.arange(3.0))
    assert list(ck["cpc"]) == list(old) and len(ck["cpc"]) == 24 and all(torch.equal(ck["cpc"][k], new[k]) for k in new)
    io.save_fitted_checkpoint(out, new, None, encoder_state={"w": torch.ones(2)})
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert set(ck) == {"encoder", "cpc"} and torch.equal(ck["encoder"]["w"], torch.ones(2))
    V.CPCLoss(V.ConfCPC(12, 8, 8, 17, 64, 256)).load_state_dict(io.load_cpc_checkpoint(out))
