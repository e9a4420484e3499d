"""-m gpu: the context LSTM's gradients (``csrc/context_grad.hip``, ``vqcpc_encoder_context_fwd`` / ``_bwd``) -- the forward's bits
against ``vqcpc_encoder_context``, the four gradients and ``c`` against float64 on the nine cases of tests/ctx_grad_ref.py, their
repeatability on a dirty work space, partial requests, the autograd surface of ``Encoder.context``, the chain with ``CPCLoss``, a
20-step fit, the ABI's errors and ``cli fit-context``.

Cases, reference and judge: tests/ctx_grad_ref.py (``judge`` prints every figure, then asserts); tests/test_ctx_grad_cpu.py holds two
fp32 restatements to the same judge on the CPU.  Nothing here is measured on the code under test.

The encoder handle has z_dim = 64.  The one case with D = 32 (``h64``) runs with ``z`` and ``W_ih`` zero-padded to 64 columns: the
added terms are exact zeros in every sum, the first 32 columns are judged as they stand and the padding must come back as zeros.
"""
import ctypes

import numpy as np
import pytest
import torch

import ctx_grad_ref as R
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, synth

pytestmark = pytest.mark.gpu

NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
_state = {}


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def encoder(H):
    """A fresh Encoder with c_dim = H on the GPU (seeded weights; the tests give ``rnn`` its own)."""
    if H not in _state:
        _state[H] = synth.encoder_state_dict(c_dim=H)
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, H))
    enc.load_state_dict(_state[H])
    return enc.cuda().eval()


def on_gpu(g):
    """z (B, T, 64) and the four LSTM tensors of a case on the GPU, D padded to 64 with zeros."""
    pad = 64 - g["D"]
    z = torch.nn.functional.pad(g["z"], (0, pad)).cuda().contiguous()
    w_ih = torch.nn.functional.pad(g["w_ih"], (0, pad)).cuda().contiguous()
    return z, [w_ih, g["w_hh"].cuda(), g["b_ih"].cuda(), g["b_hh"].cuda()]


def set_rnn(enc, ws):
    with torch.no_grad():
        for n, w in zip(NAMES, ws):
            getattr(enc.rnn, n).copy_(w)


def run(enc, z, ws, G, want=(True, True, True, True)):
    """fwd + bwd with the caller's weights -> dict c, z, W_ih, W_hh, b (device tensors or None)."""
    c, saved = enc._context_fwd(z, ws)
    gz, gi, gh, gb = enc._context_bwd(z, c, saved, G, ws[:2], want)
    return {"c": c, "z": gz, "W_ih": gi, "W_hh": gh, "b": gb}


def unpadded(g, r):
    """numpy results cut back to the case's D; the padding must be zero."""
    D = g["D"]
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}
    for k in ("z", "W_ih"):
        if out[k] is not None:
            assert not out[k][..., D:].any(), k
            out[k] = np.ascontiguousarray(out[k][..., :D])
    return out


# ------------------------------------------------------------------ 1. the forward is vqcpc_encoder_context's
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_forward_bits_equal_the_context_entry(name):
    g = R.load(name)
    enc = encoder(g["H"])
    z, ws = on_gpu(g)
    set_rnn(enc, ws)
    want = enc.context(z)                                            # vqcpc_encoder_context: at B = 1, H = 256 the resident scan
    assert not want.requires_grad
    mine, _ = enc._context_fwd(z, ws)                                # the caller's pointers
    own, _ = enc._context_fwd(z, None)                               # NULL: the handle's copies
    assert torch.equal(bits(mine), bits(want)) and torch.equal(bits(own), bits(want))
    one, _ = enc._context_fwd(z[:1].contiguous(), ws)                # B = 1 of the same case
    assert torch.equal(bits(one), bits(enc.context(z[:1].contiguous())))
    assert torch.equal(bits(one), bits(want[:1]))                    # an utterance does not depend on its batch


# ------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_gradients_against_float64(name):
    g = R.load(name)
    enc = encoder(g["H"])
    z, ws = on_gpu(g)
    R.judge(name, unpadded(g, run(enc, z, ws, g["G"].cuda())), "GPU")


# ------------------------------------------------------------------ 3. equal inputs, equal bits, on a work space that is dirty
def test_repeatable_on_a_dirty_work_space():
    small, large = R.load("partial_tile"), R.load("two_tiles")
    enc = encoder(256)
    z, ws = on_gpu(small)
    zl, wl = on_gpu(large)
    G, Gl = small["G"].cuda(), large["G"].cuda()
    first = run(enc, z, ws, G)
    before = enc.workspace_bytes()
    run(enc, zl, wl, Gl)                                             # a larger call: the work space grows and is left full of it
    assert enc.workspace_bytes() > before
    c, saved = enc._context_fwd(z, ws)
    keep = saved.clone()
    saved.fill_(float("nan"))                                        # the buffer the test owns, dirtied before it is filled again
    c2, saved2 = enc._context_fwd(z, ws)
    saved.copy_(keep)
    gz, gi, gh, gb = enc._context_bwd(z, c, saved, G, ws[:2])
    second = {"c": c, "z": gz, "W_ih": gi, "W_hh": gh, "b": gb}
    run(enc, zl, wl, Gl * float("nan"))                              # NaN through the scan's work space: dA, the carry, the partials
    third = run(enc, z, ws, G)
    for k in R.TENSORS:
        assert torch.equal(bits(first[k]), bits(second[k])) and torch.equal(bits(first[k]), bits(third[k])), k
        assert torch.isfinite(third[k]).all(), k
    assert torch.equal(bits(c2), bits(c)) and torch.equal(bits(saved2), bits(keep))
    assert enc.workspace_bytes() >= before


# ------------------------------------------------------------------ 4. partial requests
@pytest.mark.parametrize("name", ["two_tiles", "t1", "h64"])
def test_partial_requests_and_exact_zeros(name):
    g = R.load(name)
    enc = encoder(g["H"])
    z, ws = on_gpu(g)
    G = g["G"].cuda()
    full = run(enc, z, ws, G)
    for i, k in enumerate(R.GRADS):
        alone = run(enc, z, ws, G, tuple(j == i for j in range(4)))
        assert all(alone[o] is None for o in R.GRADS if o != k)
        assert torch.equal(bits(alone[k]), bits(full[k])), k
    pair = run(enc, z, ws, G, (False, True, False, True))
    assert pair["z"] is None and pair["W_hh"] is None
    assert torch.equal(bits(pair["W_ih"]), bits(full["W_ih"])) and torch.equal(bits(pair["b"]), bits(full["b"]))
    if g["T"] == 1:
        assert bits(full["W_hh"]).eq(0).all()                        # +0, not -0


# ------------------------------------------------------------------ 5. the autograd surface
def test_autograd_surface():
    g = R.load("partial_tile")
    z, ws = on_gpu(g)
    G = g["G"].cuda()
    got = []
    for scale in (1.0, 2.0):
        enc = encoder(256)
        set_rnn(enc, ws)
        zz = z.clone().requires_grad_(True)
        plain = enc.context(zz)
        with torch.no_grad():
            quiet = enc.context(zz, differentiable=True)
        assert not plain.requires_grad and plain.grad_fn is None and not quiet.requires_grad and quiet.grad_fn is None
        c = enc.context(zz, differentiable=True)
        assert c.requires_grad
        assert torch.equal(bits(plain), bits(c.detach())) and torch.equal(bits(quiet), bits(c.detach()))
        (scale * (c * G).sum()).backward()
        assert torch.equal(bits(enc.rnn.bias_ih_l0.grad), bits(enc.rnn.bias_hh_l0.grad))
        got.append({"z": zz.grad, "W_ih": enc.rnn.weight_ih_l0.grad, "W_hh": enc.rnn.weight_hh_l0.grad, "b": enc.rnn.bias_ih_l0.grad})
    direct = run(encoder(256), z, ws, G)
    for k in R.GRADS:
        assert torch.equal(bits(got[0][k]), bits(direct[k])), k
        assert torch.equal(bits(got[1][k]), bits(got[0][k] * 2.0)), k

    # a frozen rnn with z.requires_grad yields only dz; nothing to differentiate: detached
    enc = encoder(256)
    set_rnn(enc, ws)
    for p in enc.rnn.parameters():
        p.requires_grad_(False)
    zz = z.clone().requires_grad_(True)
    (enc.context(zz, differentiable=True) * G).sum().backward()
    assert torch.equal(bits(zz.grad), bits(direct["z"])) and all(p.grad is None for p in enc.rnn.parameters())
    assert not enc.context(z, differentiable=True).requires_grad

    # five optimizer steps: the handle is not rebuilt, and every step reads the moved weights
    enc = encoder(256)
    set_rnn(enc, ws)
    enc.context(z)
    opt = torch.optim.SGD(enc.rnn.parameters(), lr=1e-3)
    handles, values = set(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        c = enc.context(z, differentiable=True)
        loss = (c * G).sum()
        loss.backward()
        opt.step()
        handles.add(enc._handle.value)
        values.append(loss.detach())
    values = [float(v) for v in values]
    assert len(handles) == 1 and all(a > b for a, b in zip(values, values[1:])), values
    fresh = enc.context(z)                                           # through _native(): rebuilt once, reads the stepped weights
    again, _ = enc._context_fwd(z, [getattr(enc.rnn, n).detach() for n in NAMES])
    assert torch.equal(bits(fresh), bits(again)) and enc._handle.value is not None


# ------------------------------------------------------------------ 6. the chain with CPCLoss
def chain_modules():
    g = R.chain_case()
    enc = encoder(g["H"])
    set_rnn(enc, [g[k].cuda() for k in ("w_ih", "w_hh", "b_ih", "b_hh")])
    cpc = V.CPCLoss(V.ConfCPC(g["n_pred"], g["Spk"], g["Utt"], g["Neg"], 64, g["c_dim"]))
    cpc.load_state_dict(g["sd"])
    return g, enc, cpc.cuda()


def test_chain_with_the_cpc_loss():
    g, enc, cpc = chain_modules()
    z, neg = g["z"].cuda(), (g["utt"], g["seq"])
    loss, _ = cpc(z, enc.context(z, differentiable=True), negatives=neg, differentiable=True)
    loss.backward()
    assert z.grad is None
    ws = [getattr(enc.rnn, n).detach() for n in NAMES]
    c, saved = enc._context_fwd(z, ws)
    dc = cpc.gradients(z, c, negatives=neg, wrt=("c",))["c"]
    _, gi, gh, gb = enc._context_bwd(z, c, saved, dc, ws[:2], (False, True, True, True))
    rnn = enc.rnn
    assert torch.equal(bits(rnn.weight_ih_l0.grad), bits(gi)) and torch.equal(bits(rnn.weight_hh_l0.grad), bits(gh))
    assert torch.equal(bits(rnn.bias_ih_l0.grad), bits(gb)) and torch.equal(bits(rnn.bias_hh_l0.grad), bits(gb))
    R.judge(R.CHAIN, {"c": c.cpu().numpy(), "W_ih": gi.cpu().numpy(), "W_hh": gh.cpu().numpy(), "b": gb.cpu().numpy()}, "GPU")
    K = g["K"]
    assert all(p.weight.grad is not None for p in cpc.predictors[:K]) and all(p.weight.grad is None for p in cpc.predictors[K:])


# ------------------------------------------------------------------ 7. a fit
FIT_STEPS, FIT_LR = 20, 4.0       # at lr 4 the float64 composition's own loss falls at every one of the 20 steps (2.0762 -> 1.0280);
                                  # found on the CPU with that composition alone, and asserted below


def test_fit_on_one_fixed_batch_follows_float64():
    ref_losses, p64 = R.chain_sgd(torch.float64, FIT_STEPS, FIT_LR)
    assert all(a > b for a, b in zip(ref_losses, ref_losses[1:])), ref_losses
    _, p32 = R.chain_sgd(torch.float32, FIT_STEPS, FIT_LR)           # the reference's own fp32, on the CPU

    g, enc, cpc = chain_modules()
    K = g["K"]
    z, neg = g["z"].cuda(), (g["utt"], g["seq"])
    opt = torch.optim.SGD(list(enc.rnn.parameters()) + [p for m in cpc.predictors[:K] for p in m.parameters()], lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad(set_to_none=True)
        loss, _ = cpc(z, enc.context(z, differentiable=True), negatives=neg, differentiable=True)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(l) for l in losses]
    print(f"\nfit: GPU loss {losses[0]:.6f} -> {losses[-1]:.6f}, float64 {ref_losses[0]:.6f} -> {ref_losses[-1]:.6f}")
    assert losses[-1] < losses[0]
    got = {k: getattr(enc.rnn, n).detach().cpu().double().numpy() for k, n in zip(R.CHAIN_PARAMS[:4], NAMES)}
    got["W"] = torch.stack([p.weight.detach() for p in cpc.predictors[:K]]).cpu().double().numpy()
    got["b"] = torch.stack([p.bias.detach() for p in cpc.predictors[:K]]).cpu().double().numpy()
    bad = []
    for k in R.CHAIN_PARAMS:
        drift, own = float(np.abs(got[k] - p64[k]).max()), float(np.abs(p32[k] - p64[k]).max())
        allowed = 4.0 * max(own, R.U32 * float(np.abs(p64[k]).max()))
        print(f"fit: max|{k}_gpu - {k}_64| = {drift:.3g}, torch fp32 on the CPU drifts {own:.3g}, allowed {allowed:.3g} (ratio {drift / allowed:.3f})")
        if not drift <= allowed:
            bad.append((k, drift, allowed))
    assert not bad, bad


# ------------------------------------------------------------------ 8. ABI errors
def test_abi_errors_enqueue_nothing():
    g = R.load("partial_tile")
    enc = encoder(256)
    z, ws = on_gpu(g)
    G = g["G"].cuda()
    B, T, H = g["B"], g["T"], g["H"]
    lib, h, s = _lib.load(), enc._native(), _lib.current_stream()
    n = ctypes.c_uint64()
    assert lib.vqcpc_encoder_context_saved_bytes(h, B, T, ctypes.byref(n)) == 0 and n.value % 16 == 0 and n.value > 0
    c = torch.full((B, T, H), -7.0, device="cuda")
    saved = torch.full((n.value // 4,), -7.0, device="cuda")
    outs = [torch.full(sh, -7.0, device="cuda") for sh in ((B, T, 64), (4 * H, 64), (4 * H, H), (4 * H,))]
    wp = [w.data_ptr() for w in ws]

    def fwd(z=z.data_ptr(), B=B, T=T, w=wp, c=c.data_ptr(), saved=saved.data_ptr()):
        return lib.vqcpc_encoder_context_fwd(h, z, B, T, *w, c, saved, s)

    def bwd(z=z.data_ptr(), B=B, T=T, w=wp[:2], c=c.data_ptr(), saved=saved.data_ptr(), G=G.data_ptr(), outs=[o.data_ptr() for o in outs]):
        return lib.vqcpc_encoder_context_bwd(h, z, B, T, *w, c, saved, G, *outs, s)

    INVALID = -1
    assert lib.vqcpc_encoder_context_saved_bytes(h, 0, T, ctypes.byref(n)) == INVALID
    for call in (fwd, bwd):
        assert call(z=None) == INVALID and call(c=None) == INVALID and call(saved=None) == INVALID
        assert b"null argument" in lib.vqcpc_last_error()
        assert call(B=0) == INVALID and call(T=0) == INVALID and b"B >= 1" in lib.vqcpc_last_error()
        assert call(z=z.data_ptr() + 4) == INVALID and b"16-byte aligned" in lib.vqcpc_last_error()
    assert bwd(G=None) == INVALID
    assert fwd(w=[wp[0], None, None, None]) == INVALID and fwd(w=[wp[0], wp[1], wp[2], None]) == INVALID
    assert b"all of the LSTM's weight tensors" in lib.vqcpc_last_error()
    assert bwd(w=[wp[0], None]) == INVALID and bwd(w=[None, wp[1]]) == INVALID
    assert bwd(outs=[outs[0].data_ptr() + 4, None, None, None]) == INVALID
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            assert fwd() == INVALID and b"belongs to device" in lib.vqcpc_last_error()
            assert bwd() == INVALID and b"belongs to device" in lib.vqcpc_last_error()
    torch.cuda.synchronize()
    assert bool((c == -7.0).all()) and bool((saved == -7.0).all()) and all(bool((o == -7.0).all()) for o in outs)
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool((c != -7.0).all()) and all(bool((o != -7.0).all()) for o in outs)
    set_rnn(enc, ws)
    h = enc._native()
    assert fwd(w=[None] * 4) == 0 and bwd(w=[None, None]) == 0 and bwd(outs=[None] * 4) == 0
    torch.cuda.synchronize()
    assert isinstance(h, ctypes.c_void_p)


# ------------------------------------------------------------------ 9. the command line: score, fit, score, checkpoint
def test_cli_fit_context_end_to_end(tmp_path, capsys):
    import json
    from vectorquantizedcpc_amd import cli, io
    ds = tmp_path / "datasets" / "eng"
    (ds / "test").mkdir(parents=True)
    names = [f"S{s}_{u}" for s in (1, 2) for u in "ab"]
    for n in names:
        np.save(ds / "test" / f"{n}.mel.npy", synth.mel("fit/" + n, 1, 44)[0].numpy())
    (ds / "test.json").write_text(json.dumps([["x", 0, 1, f"eng/test/{n}"] for n in names]))
    common = ["--dataset", str(ds), "--prediction-steps", "4", "--speakers", "2", "--utterances", "2", "--negatives", "3",
              "--sample-frames", "16"]
    src, out = tmp_path / "in.pt", tmp_path / "fit.pt"
    init = synth.cpc_state_dict(n_prediction_steps=4)
    torch.save({"encoder": synth.encoder_state_dict(ln_affine="random", codebook="data"), "cpc": init, "epoch": 7}, src)
    assert cli.main(["fit-context", *common, "--cpc-checkpoint", str(src), "--out-checkpoint", str(out), "--steps", "10", "--lr", "1e-3"]) == 0
    text = capsys.readouterr().out
    assert text.count("cpc loss:") == 2 and "before the fit" in text and "after the fit" in text
    line = [l for l in text.splitlines() if l.startswith("fitted")][0]
    lo, hi = (float(v) for v in line.split("cpc loss ")[1].split(" -> "))
    assert hi < lo, line
    old, ck = (torch.load(f, map_location="cpu", weights_only=True) for f in (src, out))
    assert set(ck) == {"encoder", "cpc", "epoch"} and ck["epoch"] == 7 and list(ck["cpc"]) == list(init)
    assert list(ck["encoder"]) == list(old["encoder"])
    for k, v in old["encoder"].items():
        assert torch.equal(ck["encoder"][k], v) != k.startswith("rnn."), k                # only encoder.rnn.* moved
    for k in range(4):
        for p in ("weight", "bias"):
            assert torch.equal(ck["cpc"][f"predictors.{k}.{p}"], init[f"predictors.{k}.{p}"]) != (k < 2), (k, p)
    assert io.load_cpc_checkpoint(out).keys() == init.keys()
    assert cli.main(["score", *common, "--cpc-checkpoint", str(out)]) == 0                 # score reads the fitted checkpoint
    assert "cpc loss:" in capsys.readouterr().out
