"""-m gpu: the front end's gradients (``csrc/front_grad.hip``, ``vqcpc_encoder_front_fwd`` / ``_bwd``) past the fifteen cases of
tests/test_gpu_front_grad.py -- the fourteen ``WIDE_CASES`` of tests/front_grad_ref.py: three slabs with a ragged last one (two whole
tiles and one of 5 rows), one utterance of 2050 rows on the direct conv order, utterances of ONE output frame (T = 2, 3: every row is
an utterance's first and last, taps read only padding), calls of 1 and 17 rows, ``in_channels`` 16 / 128 / 144 / 256 with two slabs
and both conv orders by name, a silent utterance (zero-variance rows), mel at 50 x the synthetic scale, and an upstream gradient that
is zero but for six rows.

Per case: the five ReLU masks against the CPU oracle's, the bits of ``z_pre`` and ``saved`` against ``vqcpc_encoder_stage``, then the
17 gradients against float64 under the family's one rule, ``max |G - G64| <= 4 max(e_ref, 2^-24 max |G64|)`` (tests/grad_judge.py;
``judge`` prints every figure, then asserts).  tests/test_front_grad_cpu.py holds two fp32 numpy restatements to the same judge on the
CPU and shows that eight seeded faults fail it.  Nothing here is measured on the code under test.

Then what no figure shows: the conv taps that read only padding come back +0 bit for bit; an utterance run alone has the bits of its
rows in the batch; guard words in front of and behind ``z_pre``, ``saved`` and all 17 gradients stay and every word between them is
written; NaN behind the valid data of ``mel``, ``G`` and ``saved`` changes no bit; partial requests at two and three slabs have the
bits of the full call; a work space that a larger call drove NaN through gives the same bits again; two autograd graphs of different
shapes alive over one handle accumulate the fp32 sum of the two direct calls.

Measured on an MI355X over the fourteen cases (the file runs in 11 s, no test above 2.3 s).  Largest ``max |G_gpu - G64| / e_ref`` per
tensor (the bound is 4): conv 0.71 (``c128_m1``); dgamma of LN 0 .. 4: 1.05 (``r17``), 0.78 (``silent``), 1.19 (``sparse_G``), 1.48, 1.36
(``r1``); dbeta: 0.73 (``T2``), 0.97 (``silent``), 0.71 (``r1``), 0.93 (``sparse_G``), 1.96 (``r1``); fc 0 .. 3: 1.01 (``c128_m1``), 1.57
(``r1``), 1.36 (``c16_slabs``), 2.28 (``r1``); out_w 2.95 (``r1``: a product of one row, one rounding per element, the figure of both CPU
restatements too); out_b 2.74 (``one_long``; on ``r1`` it is exact, as is its ``e_ref``).  ``tail37``: 0.14 .. 1.54 (out_b).  Largest
``err / bound`` (the bound is 1): 0.74 (out_w, ``r1``), then 0.69 (out_b, ``one_long``).  No test found a fault: the kernels are unchanged.
"""
import ctypes

import numpy as np
import pytest
import torch

import front_grad_ref as R
import test_gpu_front_grad as base
from test_gpu_front_grad import TOP_TWO, bits, encoder, front_params, on_gpu
from vectorquantizedcpc_amd import _lib, synth

pytestmark = pytest.mark.gpu

_full = {}
OUT = R.KEYS + ["z_pre", "saved"]


@pytest.fixture(scope="module", autouse=True)
def release_what_this_file_holds():
    """The cases, the float64 references and the device buffers of this file are released when it is done, so that the files that
    run after it find the process -- its heap and torch's caching allocator -- as they would without it."""
    yield
    import gc
    R._cases.clear()
    R._fwd.clear()
    R._refs.clear()
    _full.clear()
    base._state.clear()
    gc.collect()
    torch.cuda.empty_cache()


def run(enc, g, mel, ws, G, want=None, mode=None):
    """fwd + bwd with the caller's weights -> dict by ``R.KEYS`` (device tensors or None), ``z_pre`` and ``saved``."""
    mode = g["mode"] if mode is None else mode
    asked = tuple(want is None or k in want for k in R.KEYS)
    z_pre, saved = enc._front_fwd(mel, ws, mode)
    grads = enc._front_bwd(mel, saved, G, ws, asked, mode)
    return dict(zip(R.KEYS, grads), z_pre=z_pre, saved=saved)


def inputs(name):
    g = R.load(name)
    mel, ws = on_gpu(g)
    return g, mel, ws, g["G"].cuda()


def full(name):
    """fwd + bwd of a wide case on a fresh handle, all 17 gradients: computed once and shared (read-only)."""
    if name not in _full:
        g, mel, ws, G = inputs(name)
        _full[name] = run(encoder(g["C"]), g, mel, ws, G)
    return _full[name]


def same_bits(a, b, what, keys=OUT):
    for k in keys:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


# ------------------------------------------------------------------ 1. the forward is vqcpc_encoder_stage's, then the judge
@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_forward_bits_equal_the_stage_entry(name):
    g, mel, ws, _ = inputs(name)
    enc = encoder(g["C"], g["w"])
    forced = R.masks(name)
    for l, s in enumerate((1, 3, 5, 7, 9)):                          # first: a mask mismatch is reported as what it is
        got = (enc.stage(mel, s, g["mode"]) > 0).cpu().numpy().reshape(g["R"], 512)
        assert np.array_equal(got, forced[l]), f"{name}: ReLU mask {l} differs from the oracle's in {(got != forced[l]).sum()} elements"
    mine = full(name)                                                # the caller's pointers
    own, saved_own = enc._front_fwd(mel, None, g["mode"])            # NULL: the handle's copies
    want = enc.stage(mel, 10, g["mode"])
    assert torch.equal(bits(mine["z_pre"]), bits(want)) and torch.equal(bits(own), bits(want))
    saved = mine["saved"]
    assert torch.equal(bits(saved), bits(saved_own))
    n = g["R"] * 512
    assert saved.numel() == g["R"] * (10 * 512 + 10)
    for l, s in enumerate((0, 2, 4, 6, 8)):                          # saved: the rows entering each LayerNorm and leaving each ReLU
        assert torch.equal(bits(saved[l * n:(l + 1) * n]), bits(enc.stage(mel, s, g["mode"]))), l
        assert torch.equal(bits(saved[(5 + l) * n:(6 + l) * n]), bits(enc.stage(mel, s + 1, g["mode"]))), l
    assert bool(torch.isfinite(saved).all())                         # the (mean, rstd) pairs behind them


@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_gradients_against_float64(name):
    got = full(name)
    R.judge(name, {k: got[k].cpu().numpy() for k in R.KEYS}, "GPU")


# ------------------------------------------------------------------ 2. taps that read only padding
@pytest.mark.parametrize("name,taps", [("T2", (0, 3)), ("T2_m1", (0, 3)), ("T3_m2", (0,))])
def test_taps_that_read_only_padding_are_plus_zero(name, taps):
    conv = full(name)["conv"]
    ref = R.grads64(name)["conv"]
    for tap in range(4):
        assert bool(ref[:, :, tap].any()) == (tap not in taps), tap
        if tap in taps:
            assert bool(bits(conv[:, :, tap]).eq(0).all()), (name, tap)      # +0, not -0
        else:
            assert bool(conv[:, :, tap].ne(0).any()), (name, tap)


# ------------------------------------------------------------------ 3. an utterance does not depend on its batch
@pytest.mark.parametrize("name", ["tail37", "T2"])
def test_an_utterance_alone_has_the_bits_of_its_rows_in_the_batch(name):
    g, mel, ws, _ = inputs(name)
    B, To, n = g["B"], g["To"], g["R"]
    enc = encoder(g["C"])
    zb, sb = enc._front_fwd(mel, ws, 2)                              # the direct order by name: B = 1 would resolve AUTO otherwise
    rows, stats = sb[:10 * n * 512].view(10, n, 512), sb[10 * n * 512:].view(5, n, 2)
    for u in (0, B // 2, B - 1):
        za, sa = enc._front_fwd(mel[u:u + 1].contiguous(), ws, 2)
        at = slice(u * To, (u + 1) * To)
        assert torch.equal(bits(za), bits(zb[u:u + 1])), (u, "z_pre")
        assert torch.equal(bits(sa[:10 * To * 512].view(10, To, 512)), bits(rows[:, at])), (u, "saved rows")
        assert torch.equal(bits(sa[10 * To * 512:].view(5, To, 2)), bits(stats[:, at])), (u, "saved statistics")


# ------------------------------------------------------------------ 4. guard words
FRONT, BACK = 4096 + 48, 4096          # bytes of sentinel around every output; 48: the output is 16-byte aligned and no more


class Guarded:
    """``nbytes`` of output inside a larger buffer of 0xFF bytes, the output's own bytes included: every fp32 word a NaN."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = torch.full((FRONT + nbytes + BACK,), 0xFF, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0

    def data_ptr(self):
        return self.buf.data_ptr() + FRONT

    def guards_intact(self):
        return bool((self.buf[:FRONT] == 0xFF).all()) and bool((self.buf[FRONT + self.n:] == 0xFF).all())

    def values(self):
        return self.buf[FRONT:FRONT + self.n].view(torch.float32)


@pytest.mark.parametrize("name", ["tail37", "c256_slabs_m2"])
def test_guard_words_around_every_output(name):
    g, mel, ws, G = inputs(name)
    B, T = g["B"], g["T"]
    enc = encoder(g["C"])
    lib, h, s = _lib.load(), enc._native(), _lib.current_stream()
    n = ctypes.c_uint64()
    assert lib.vqcpc_encoder_front_saved_bytes(h, B, T, ctypes.byref(n)) == 0 and n.value == g["R"] * (10 * 512 + 10) * 4
    out = {k: Guarded(w.numel() * 4) for k, w in zip(R.KEYS, ws)}
    out.update(z_pre=Guarded(g["R"] * 64 * 4), saved=Guarded(n.value))
    W = enc._front_struct(ws)
    _lib.check(lib.vqcpc_encoder_front_fwd(h, mel.data_ptr(), B, T, g["mode"], ctypes.byref(W), out["z_pre"].data_ptr(),
                                           out["saved"].data_ptr(), s))
    _lib.check(lib.vqcpc_encoder_front_bwd(h, mel.data_ptr(), B, T, g["mode"], ctypes.byref(W), out["saved"].data_ptr(), G.data_ptr(),
                                           ctypes.byref(enc._front_struct([out[k] for k in R.KEYS])), s))
    torch.cuda.synchronize()
    ref = full(name)
    for k in OUT:
        assert out[k].guards_intact(), k
        assert bool(torch.isfinite(out[k].values()).all()), k        # every word between the guards was written
        assert torch.equal(bits(out[k].values()), bits(ref[k])), k


# ------------------------------------------------------------------ 5. NaN behind the valid data
def nan_behind(t):
    """A contiguous copy of ``t`` at the front of a larger buffer whose remainder is NaN."""
    big = torch.full((t.numel() + 4096,), float("nan"), device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape)


@pytest.mark.parametrize("name", ["tail37", "r17", "T2"])
def test_nan_behind_the_valid_data_changes_no_bit(name):
    g, mel, ws, G = inputs(name)
    enc = encoder(g["C"])
    mel_n, G_n = nan_behind(mel), nan_behind(G)
    z_pre, saved = enc._front_fwd(mel_n, ws, g["mode"])
    saved_n = nan_behind(saved)
    grads = enc._front_bwd(mel_n, saved_n, G_n, ws, (True,) * 17, g["mode"])
    same_bits(dict(zip(R.KEYS, grads), z_pre=z_pre, saved=saved), full(name), "NaN behind mel, G and saved")


# ------------------------------------------------------------------ 6. partial requests at two and three slabs
@pytest.mark.parametrize("name", ["tail37", "c144_slabs"])
def test_partial_requests_have_the_bits_of_the_full_call(name):
    g, mel, ws, G = inputs(name)
    ref = full(name)
    for want in (("conv",), ("ln_g0",), ("fc1",), ("out_b",), TOP_TWO):
        got = run(encoder(g["C"]), g, mel, ws, G, want)              # a fresh handle: its work space is this request's alone
        assert all(got[k] is None for k in R.KEYS if k not in want), want
        same_bits(got, ref, want, want)


# ------------------------------------------------------------------ 7. a dirty work space
def rows63_c256():
    """A 63-row call at in_channels = 256 with the weights of ``c256_slabs_m2`` (no reference: compared with itself)."""
    w = R.load("c256_slabs_m2")["w"]
    return dict(B=3, T=42, C=256, To=21, R=63, mode=0, mel=synth.mel("front_grad/c256_rows63", 3, 42, n_mels=256),
                G=R._u("c256_rows63/G", (3, 21, 64), 1.0), w=w)


@pytest.mark.parametrize("large,small", [("tail37", "r17"), ("c256_slabs_m2", None)])
def test_repeatable_after_nan_went_through_a_larger_work_space(large, small):
    gl, mel_l, ws_l, G_l = inputs(large)
    gs = R.load(small) if small else rows63_c256()
    (mel_s, ws_s), G_s = on_gpu(gs), gs["G"].cuda()
    enc = encoder(gl["C"])
    run(enc, gl, mel_l, ws_l, G_l)
    before = enc.workspace_bytes()
    first = run(enc, gs, mel_s, ws_s, G_s)
    assert enc.workspace_bytes() == before                           # grow-only: the small call runs in the large call's dirt
    poisoned = run(enc, gl, mel_l, ws_l, G_l * float("nan"))         # NaN through every gradient buffer and partial
    assert all(bool(torch.isnan(poisoned[k]).any()) for k in R.KEYS)
    again = run(enc, gs, mel_s, ws_s, G_s)
    same_bits(first, again, "after NaN")
    same_bits(first, full(small) if small else run(encoder(gs["C"]), gs, mel_s, ws_s, G_s), "a fresh handle")
    assert all(bool(torch.isfinite(again[k]).all()) for k in OUT)


# ------------------------------------------------------------------ 8. two graphs of different shapes alive over one handle
def test_two_graphs_alive_over_one_work_space():
    (ga, mel_a, ws_a, G_a), (gb, mel_b, ws_b, G_b) = inputs("partial_tile"), inputs("tail37")
    assert all(torch.equal(x, y) for x, y in zip(ws_a, ws_b))        # one set of weights
    direct_a = run(encoder(), ga, mel_a, ws_a, G_a)
    direct_b = full("tail37")
    enc = encoder(80, ga["w"])
    za = enc.front_end(mel_a, differentiable=True)
    zb = enc.front_end(mel_b, differentiable=True)                   # the larger call dirties the work space under the first graph
    assert torch.equal(bits(za.detach()), bits(direct_a["z_pre"])) and torch.equal(bits(zb.detach()), bits(direct_b["z_pre"]))
    handle = enc._handle.value
    (zb * G_b).sum().backward()                                      # in reverse order
    (za * G_a).sum().backward()
    for k, p in zip(R.KEYS, front_params(enc)):
        assert torch.equal(bits(p.grad), bits(direct_b[k] + direct_a[k])), k
    assert enc._handle.value == handle

    enc = encoder(80, ga["w"])
    z = enc.front_end(mel_b, differentiable=True)
    loss = (z * G_b).sum()
    loss.backward(retain_graph=True)
    for k, p in zip(R.KEYS, front_params(enc)):
        assert torch.equal(bits(p.grad), bits(direct_b[k])), k
    loss.backward(retain_graph=True)
    for k, p in zip(R.KEYS, front_params(enc)):
        assert torch.equal(bits(p.grad), bits(direct_b[k] * 2.0)), k
