"""-m gpu: the CPC gradients (``csrc/cpc_grad.hip``, ``vqcpc_cpc_grad``) -- the forward's bits against ``vqcpc_cpc_score``, the four
gradients against float64 on the four recorded fixtures, the six cases of tests/cpc_cases.py and ``long`` (L = 1099), their
repeatability on a dirty work space, exact zeros, partial requests, the autograd surface of ``CPCLoss`` and a 20-step fit.

Cases, reference and judge: tests/cpc_grad_ref.py (``judge`` prints every figure, then asserts); tests/test_cpc_grad_cpu.py holds
a differently ordered fp32 backward to the same judge on the CPU.  Nothing here is measured on the code under test.
"""
import ctypes

import numpy as np
import pytest
import torch

import cpc_cases
import cpc_grad_ref as R
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

GRADS = ("z", "c", "W", "b")


def module_for(g):
    cpc = V.CPCLoss(V.ConfCPC(g["n_pred"], g["Spk"], g["Utt"], g["Neg"], 64, g["c_dim"]))
    cpc.load_state_dict(g["sd"])
    return cpc.cuda()


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def same_bits(a, b, keys):
    for key in keys:
        assert torch.equal(bits(a[key]), bits(b[key])), key


def indices(g):
    return g["utt"], g["seq"]


# ------------------------------------------------------------------ 1. the forward is vqcpc_cpc_score's
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_loss_bits_equal_the_score_entry(name):
    g = R.load(name)
    cpc = module_for(g)
    z, c = g["z"].cuda(), g["c"].cuda()
    for kw in ({"negatives": indices(g)}, {"seed": (3 << 32) | 7, "stream_id": 2}):
        same_bits(cpc.gradients(z, c, **kw), cpc.forward_detailed(z, c, **kw), ("loss", "step_loss", "accuracy"))
        same_bits(cpc.gradients(z, c, wrt=("W",), **kw), cpc.forward_detailed(z, c, **kw), ("loss", "step_loss", "accuracy"))


# ------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_gradients_against_float64(name):
    g = R.load(name)
    cpc = module_for(g)
    r = cpc.gradients(g["z"].cuda(), g["c"].cuda(), negatives=indices(g))
    R.judge(name, {k: r[k].cpu().numpy() for k in GRADS}, "GPU")
    assert abs(float(r["loss"]) - R.grads64(name)["loss"]) <= 1e-5 * max(1.0, abs(R.grads64(name)["loss"]))
    if name in cpc_cases.PROTOCOL_CASES or name in R.LONG:       # these cases' index arrays ARE the protocol's at (13, 0)
        same_bits(cpc.gradients(g["z"].cuda(), g["c"].cuda(), seed=13, stream_id=0), r, GRADS + ("loss", "step_loss", "accuracy"))


# ------------------------------------------------------------------ 3. equal inputs, equal bits, on a work space that is dirty
def test_repeatable_on_a_dirty_work_space():
    g, small, short = R.load("partials"), R.load("c64_min"), cpc_cases.reference("partials", cpc_cases.SHRINK_T)
    cpc, other = module_for(g), module_for(small)
    z, c = g["z"].cuda(), g["c"].cuda()
    first = cpc.gradients(z, c, negatives=indices(g))
    other.gradients(small["z"].cuda(), small["c"].cuda(), negatives=indices(small))
    second = cpc.gradients(z, c, negatives=indices(g))
    cpc.gradients(short["z"].cuda(), short["c"].cuda(), negatives=(short["utt"], short["seq"]))       # T = 3 on the grown work space
    other.gradients(small["z"].cuda(), small["c"].cuda(), negatives=indices(small))
    third = cpc.gradients(z, c, negatives=indices(g))
    same_bits(first, second, GRADS + ("loss", "step_loss", "accuracy"))
    same_bits(first, third, GRADS + ("loss", "step_loss", "accuracy"))


# ------------------------------------------------------------------ 4. zeros and partial requests
@pytest.mark.parametrize("name", ["small_odd", "long"])
def test_exact_zeros_and_partial_requests(name):
    g = R.load(name)
    cpc = module_for(g)
    z, c = g["z"].cuda().requires_grad_(True), g["c"].cuda().requires_grad_(True)
    loss, _ = cpc(z, c, negatives=indices(g), differentiable=True)
    loss.backward()
    assert not z.grad[:, 0].any() and not c.grad[:, g["L"]:].any()
    assert bits(z.grad[:, 0]).eq(0).all() and bits(c.grad[:, g["L"]:]).eq(0).all()                     # +0, not -0
    assert z.grad[:, 1:].any() and c.grad[:, :g["L"]].any()
    full = {"W": torch.stack([p.weight.grad for p in cpc.predictors[:g["K"]]]), "b": torch.stack([p.bias.grad for p in cpc.predictors[:g["K"]]])}
    cpc.zero_grad(set_to_none=True)
    z2, c2 = g["z"].cuda(), g["c"].cuda()
    loss2, _ = cpc(z2, c2, negatives=indices(g), differentiable=True)
    loss2.backward()
    assert z2.grad is None and c2.grad is None
    only = {"W": torch.stack([p.weight.grad for p in cpc.predictors[:g["K"]]]), "b": torch.stack([p.bias.grad for p in cpc.predictors[:g["K"]]])}
    same_bits(full, only, ("W", "b"))
    assert torch.equal(bits(loss.detach()), bits(loss2.detach()))
    # one gradient alone: the other launches are skipped, the bits stay
    r = cpc.gradients(z2, c2, negatives=indices(g))
    for k in GRADS:
        alone = cpc.gradients(z2, c2, negatives=indices(g), wrt=(k,))
        assert all(alone[o] is None for o in GRADS if o != k)
        same_bits(alone, r, (k,))


# ------------------------------------------------------------------ 5. upstream gradient
def test_upstream_gradient_scales_and_unused_predictors_get_none():
    g = R.load("small_odd")
    K = g["K"]
    got = []
    for scale in (1.0, 2.0):
        cpc = module_for(g)
        z, c = g["z"].cuda().requires_grad_(True), g["c"].cuda().requires_grad_(True)
        loss, acc = cpc(z, c, negatives=indices(g), differentiable=True)
        assert loss.requires_grad and len(acc) == K
        (scale * loss).backward()
        assert all(p.weight.grad is not None and p.bias.grad is not None for p in cpc.predictors[:K])
        assert all(p.weight.grad is None and p.bias.grad is None for p in cpc.predictors[K:])
        got.append({"z": z.grad, "c": c.grad, "W": torch.stack([p.weight.grad for p in cpc.predictors[:K]]),
                    "b": torch.stack([p.bias.grad for p in cpc.predictors[:K]])})
    for k in GRADS:
        assert torch.equal(bits(got[1][k]), bits(got[0][k] * 2.0)), k
    same_bits(got[0], module_for(g).gradients(g["z"].cuda(), g["c"].cuda(), negatives=indices(g)), GRADS)


# ------------------------------------------------------------------ 6. the flag
def test_default_and_no_grad_stay_detached():
    g = R.load("small_odd")
    cpc = module_for(g)
    z, c = g["z"].cuda().requires_grad_(True), g["c"].cuda().requires_grad_(True)
    loss, _ = cpc(z, c, negatives=indices(g))
    assert not loss.requires_grad and loss.grad_fn is None
    with torch.no_grad():
        quiet, _ = cpc(z, c, negatives=indices(g), differentiable=True)
    assert not quiet.requires_grad and quiet.grad_fn is None
    hot, _ = cpc(z, c, negatives=indices(g), differentiable=True)
    assert hot.requires_grad
    assert torch.equal(bits(loss), bits(quiet)) and torch.equal(bits(loss), bits(hot.detach()))
    for p in cpc.parameters():
        p.requires_grad_(False)
    cold, _ = cpc(z.detach(), c.detach(), negatives=indices(g), differentiable=True)       # nothing to differentiate
    assert not cold.requires_grad


# ------------------------------------------------------------------ 7. a fit
FIT_STEPS, FIT_LR = 20, 16.0      # at lr 16 the float64 restatement's own loss falls at every one of the 20 steps (2.0927 -> 0.1577);
                                  # found on the CPU with that restatement alone, and asserted below


def test_fit_on_one_fixed_batch_follows_float64():
    g = R.load("small_odd")
    rows, K = R.row_index(g), g["K"]
    z64, c64 = g["z"].double(), g["c"].double()
    W64, b64 = g["W"].double().clone().requires_grad_(True), g["b"].double().clone().requires_grad_(True)
    ref_losses = []
    for _ in range(FIT_STEPS):
        loss, _ = R.loss_torch(z64, c64, W64, b64, rows)
        gW, gb = torch.autograd.grad(loss, (W64, b64))
        ref_losses.append(float(loss.detach()))
        with torch.no_grad():
            W64 -= FIT_LR * gW
            b64 -= FIT_LR * gb
    assert all(a > b for a, b in zip(ref_losses, ref_losses[1:])), ref_losses

    cpc = module_for(g)
    opt = torch.optim.SGD([p for m in cpc.predictors[:K] for p in m.parameters()], lr=FIT_LR)
    z, c = g["z"].cuda(), g["c"].cuda()
    losses, handles = [], set()
    for _ in range(FIT_STEPS):
        opt.zero_grad(set_to_none=True)
        loss, _ = cpc(z, c, negatives=indices(g), differentiable=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
        handles.add(cpc._handle.value)
    losses = [float(l) for l in losses]
    assert len(handles) == 1                                                 # an optimizer step does not rebuild the native handle
    print(f"\nfit: GPU loss {losses[0]:.6f} -> {losses[-1]:.6f}, float64 {ref_losses[0]:.6f} -> {ref_losses[-1]:.6f}")
    assert losses[-1] < losses[0]
    W = torch.stack([p.weight.detach() for p in cpc.predictors[:K]]).cpu().double().numpy()
    b = torch.stack([p.bias.detach() for p in cpc.predictors[:K]]).cpu().double().numpy()
    for k, got, ref in (("W", W, W64.detach().numpy()), ("b", b, b64.detach().numpy())):
        drift, allowed = float(np.abs(got - ref).max()), FIT_STEPS * FIT_LR * R.bound("small_odd", k)
        print(f"fit: max|{k}_gpu - {k}_64| = {drift:.3g}, steps * lr * judge = {allowed:.3g} (ratio {drift / allowed:.3f})")
        assert drift <= allowed
    # scoring afterwards reads the fitted predictors, not the copies the handle was built with
    after = cpc.forward_detailed(z, c, negatives=indices(g))["loss"]
    assert float(after) < losses[-1] + 1e-6 and float(after) < losses[0]


# ------------------------------------------------------------------ 8. ABI errors
def test_abi_errors_enqueue_nothing():
    g = R.load("small_odd")
    cpc = module_for(g)
    K, T = g["K"], g["T"]
    z, c = g["z"].cuda(), g["c"].cuda()
    W, b = g["W"].cuda(), g["b"].cuda()
    utt, seq = g["utt"].cuda(), g["seq"].cuda()
    lib, h, s = _lib.load(), cpc._native(), _lib.current_stream()
    out = torch.full((1 + 2 * K,), -7.0, device="cuda")
    gW, gb = torch.full_like(W, -7.0), torch.full_like(b, -7.0)

    def call(T=T, W=W.data_ptr(), b=b.data_ptr(), utt=utt.data_ptr(), seq=seq.data_ptr()):
        return lib.vqcpc_cpc_grad(h, z.data_ptr(), c.data_ptr(), T, W, b, utt, seq, 13, 0, out[0:].data_ptr(), out[1:].data_ptr(),
                                  out[1 + K:].data_ptr(), None, None, gW.data_ptr(), gb.data_ptr(), s)

    INVALID = -1
    assert call(T=K + 1) == INVALID and b"n_steps + 2" in lib.vqcpc_last_error()
    assert call(W=None) == INVALID and call(b=None) == INVALID and b"W and bias" in lib.vqcpc_last_error()
    assert call(utt=None) == INVALID and call(seq=None) == INVALID and b"utt_index and seq_index" in lib.vqcpc_last_error()
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert call() == INVALID and b"belongs to device" in lib.vqcpc_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((gW == -7.0).all()) and bool((gb == -7.0).all())
    assert call() == 0 and call(W=None, b=None) == 0 and call(utt=None, seq=None) == 0
    torch.cuda.synchronize()
    assert bool((out != -7.0).all()) and bool((gW != -7.0).all())
    assert isinstance(h, ctypes.c_void_p)


# ------------------------------------------------------------------ 9. the command line: score, fit, score, checkpoint
def test_cli_fit_predictors_end_to_end(tmp_path, capsys):
    import json
    from vectorquantizedcpc_amd import cli, io, synth
    ds = tmp_path / "datasets" / "eng"
    (ds / "test").mkdir(parents=True)
    names = [f"S{s}_{u}" for s in (1, 2) for u in "ab"]
    for n in names:
        np.save(ds / "test" / f"{n}.mel.npy", synth.mel("fit/" + n, 1, 44)[0].numpy())
    (ds / "test.json").write_text(json.dumps([["x", 0, 1, f"eng/test/{n}"] for n in names]))
    common = ["--dataset", str(ds), "--prediction-steps", "4", "--speakers", "2", "--utterances", "2", "--negatives", "3",
              "--sample-frames", "16"]
    src, first, second = tmp_path / "in.pt", tmp_path / "fit1.pt", tmp_path / "fit2.pt"
    # from a checkpoint (a data-scale codebook, so the scores are not all alike): everything but "cpc" is carried over
    init = synth.cpc_state_dict(n_prediction_steps=4)
    torch.save({"encoder": synth.encoder_state_dict(ln_affine="random", codebook="data"), "cpc": init, "epoch": 7}, src)
    assert cli.main(["fit-predictors", *common, "--cpc-checkpoint", str(src), "--out-checkpoint", str(first), "--steps", "10", "--lr", "1e-3"]) == 0
    text = capsys.readouterr().out
    assert text.count("cpc loss:") == 2 and "before the fit" in text and "after the fit" in text
    old, ck = (torch.load(f, map_location="cpu", weights_only=True) for f in (src, first))
    assert set(ck) == {"encoder", "cpc", "epoch"} and ck["epoch"] == 7 and list(ck["cpc"]) == list(init) and len(ck["cpc"]) == 8
    assert all(torch.equal(ck["encoder"][k], v) for k, v in old["encoder"].items())
    for k in range(4):
        moved = not torch.equal(ck["cpc"][f"predictors.{k}.weight"], init[f"predictors.{k}.weight"])
        assert moved == (k < 2), k                                           # the K predictors in use, and only those
    line = [l for l in text.splitlines() if l.startswith("fitted")][0]
    lo, hi = (float(v) for v in line.split("cpc loss ")[1].split(" -> "))
    assert hi < lo, line
    assert io.load_cpc_checkpoint(first).keys() == init.keys()
    # seeded weights: the encoder they name is written next to the fitted predictors
    assert cli.main(["fit-predictors", *common, "--random-init", "--out-checkpoint", str(second), "--steps", "2"]) == 0
    ck2 = torch.load(second, map_location="cpu", weights_only=True)
    assert set(ck2) == {"encoder", "cpc"} and list(ck2["cpc"]) == list(init)
    assert all(torch.equal(ck2["encoder"][k], v) for k, v in synth.encoder_state_dict().items())
    assert torch.equal(ck2["cpc"]["predictors.3.weight"], init["predictors.3.weight"])
