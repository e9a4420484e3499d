"""-m gpu: the context LSTM's gradients (``csrc/context_grad.hip``, ``vqcpc_encoder_context_fwd`` / ``_bwd``) past the nine cases of
tests/test_gpu_ctx_grad.py -- the twelve ``WIDE_CASES`` of tests/ctx_grad_ref.py: nine utterance tiles with two live columns in the
last, row counts on and one past a slab edge, three tiles at H = 512, thirteen slabs at H = 64, 3 000 steps of BPTT, the forward
suite's ``stressed`` weights, and upstream gradients that are zero but for late steps, as ``CPCLoss`` hands them over.

Per case: the forward's bits against ``vqcpc_encoder_context``, then ``c`` and the four gradients against float64 under two judges
(tests/ctx_grad_ref.py; both print every figure, then assert): per tensor ``max |G - G64| <= 4 max(e_ref, 2^-24 max |G64|)``, and for
``c`` and ``dz`` the same rule per time step, which holds a step ten orders of magnitude below the tensor's largest to its own
size.  tests/test_ctx_grad_cpu.py holds two fp32 numpy restatements to both judges on the CPU and shows that four seeded faults fail
them.  Nothing here is measured on the code under test.

Then what no figure shows: an utterance run alone has the bits of its rows in the batch; guard words in front of and behind ``c``,
``saved`` and the four gradients stay as they were and every word between them is written; NaN behind the valid rows of ``z``,
``grad_c`` and ``c`` changes no bit; each gradient asked for alone has the bits of the full call; a work space that a larger call
drove NaN through gives the same bits again.

Measured on an MI355X over the twelve cases (bound: 4 in the first line, 1 in the second).  Largest ``max |G_gpu - G64| / e_ref``
per tensor: c 1.30 (``long_stressed``), dz 1.04 (``h512_tiles``), dW_ih 1.97 (``tail_h64``), dW_hh 1.59 (``tail_h64``), db 0.66
(``tail_stressed``).  Largest per-step ``err / bound``: c 0.92 (``long_stressed``, t = 1604), dz 0.54 (``tail_stressed``, t = 12,
where ``max |dz[:, t]|`` is 2.9e-4 of 1.76 at t = 199); on ``tail`` 0.36 at t = 11, where ``max |dz[:, t]|`` is 3.1e-11 of 0.24; the
six steps t >= 64 of ``cpc_shaped`` come back zero.  The CPU restatements reach 0.71 (c) and 0.63 (dz) per step.
"""
import ctypes

import numpy as np
import pytest
import torch

import ctx_grad_ref as R
from test_gpu_ctx_grad import bits, encoder, on_gpu, run, set_rnn
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

_full = {}


def inputs(name):
    g = R.load(name)
    z, ws = on_gpu(g)
    return g, z, ws, g["G"].cuda()


def full(name):
    """fwd + bwd of a wide case, all four gradients: computed once and shared (read-only)."""
    if name not in _full:
        g, z, ws, G = inputs(name)
        _full[name] = run(encoder(g["H"]), z, ws, G)
    return _full[name]


def same_bits(a, b, what):
    for k in R.TENSORS:
        assert torch.equal(bits(a[k]), bits(b[k])), (what, k)


# ------------------------------------------------------------------ 1. the forward's bits, then both judges
@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_case_against_float64(name):
    g, z, ws, G = inputs(name)
    enc = encoder(g["H"])
    set_rnn(enc, ws)
    want = enc.context(z)                                            # vqcpc_encoder_context
    own, _ = enc._context_fwd(z, None)                               # NULL: the handle's copies
    got = full(name)                                                 # the caller's pointers
    assert torch.equal(bits(got["c"]), bits(want)) and torch.equal(bits(own), bits(want))
    host = {k: v.cpu().numpy() for k, v in got.items()}
    R.judge(name, host, "GPU")
    R.judge_steps(name, host, "GPU")


# ------------------------------------------------------------------ 2. an utterance does not depend on its batch
@pytest.mark.parametrize("name,utterances", [("b130", (0, 15, 16, 127, 128, 129)), ("slab_plus_one", (0, 15, 16, 24))])
def test_an_utterance_alone_has_the_bits_of_its_rows_in_the_batch(name, utterances):
    g, z, ws, G = inputs(name)
    enc = encoder(g["H"])
    batch = full(name)
    for u in utterances:
        alone = run(enc, z[u:u + 1].contiguous(), ws, G[u:u + 1].contiguous(), (True, False, False, False))
        assert torch.equal(bits(alone["c"]), bits(batch["c"][u:u + 1])), (u, "c")
        assert torch.equal(bits(alone["z"]), bits(batch["z"][u:u + 1])), (u, "dz")


# ------------------------------------------------------------------ 3. guard words
FRONT, BACK = 4096 + 48, 4096          # bytes of sentinel around every output; 48: the output is 16-byte aligned and no more


class Guarded:
    """``nbytes`` of output inside a larger buffer filled with the byte ``fill``, the output's own bytes included."""

    def __init__(self, nbytes, fill):
        self.n, self.fill = nbytes, fill
        self.buf = torch.full((FRONT + nbytes + BACK,), fill, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        self.ptr = self.buf.data_ptr() + FRONT

    def guards_intact(self):
        return bool((self.buf[:FRONT] == self.fill).all()) and bool((self.buf[FRONT + self.n:] == self.fill).all())

    def words(self):
        return self.buf[FRONT:FRONT + self.n].view(torch.int32)


@pytest.mark.parametrize("name", ["slab_plus_one", "b130"])
def test_guard_words_around_every_output(name):
    g, z, ws, G = inputs(name)
    B, T, H = g["B"], g["T"], g["H"]
    enc = encoder(H)
    lib, h, s = _lib.load(), enc._native(), _lib.current_stream()
    n = ctypes.c_uint64()
    assert lib.vqcpc_encoder_context_saved_bytes(h, B, T, ctypes.byref(n)) == 0
    assert n.value == B * T * 6 * H * 4                              # gates (R, 4H), cell (R, H), tanh(cell) (R, H) in fp32
    sizes = {"c": B * T * H * 4, "saved": n.value, "z": B * T * 64 * 4, "W_ih": 4 * H * 64 * 4, "W_hh": 4 * H * H * 4, "b": 4 * H * 4}
    wp = [w.data_ptr() for w in ws]
    runs = []
    for fill in (0xA5, 0x5A):          # a word that holds the sentinel after both runs was not written (equal inputs give equal bits)
        out = {k: Guarded(v, fill) for k, v in sizes.items()}
        _lib.check(lib.vqcpc_encoder_context_fwd(h, z.data_ptr(), B, T, *wp, out["c"].ptr, out["saved"].ptr, s))
        _lib.check(lib.vqcpc_encoder_context_bwd(h, z.data_ptr(), B, T, *wp[:2], out["c"].ptr, out["saved"].ptr, G.data_ptr(),
                                                 *[out[k].ptr for k in R.GRADS], s))
        torch.cuda.synchronize()
        for k, o in out.items():
            assert o.guards_intact(), (k, hex(fill))
        runs.append(out)
    first, second = runs
    word = lambda fill: int.from_bytes(bytes([fill] * 4), "little", signed=True)
    for k in sizes:
        a, b = first[k].words(), second[k].words()
        unwritten = (a == word(0xA5)) & (b == word(0x5A))
        assert not bool(unwritten.any()), (k, int(unwritten.sum()))
        assert torch.equal(a, b), k
    ref = full(name)
    for k in R.TENSORS:
        assert torch.equal(first[k].words(), bits(ref[k]).view(torch.int32)), k


# ------------------------------------------------------------------ 4. NaN behind the valid rows
def nan_behind(t):
    """A contiguous copy of ``t`` at the front of a larger buffer whose remainder is NaN."""
    big = torch.full((t.numel() + 4096,), float("nan"), device=t.device)
    big[:t.numel()] = t.reshape(-1)
    return big[:t.numel()].view(t.shape)


def test_nan_behind_the_valid_rows_changes_no_bit():
    name = "slab_plus_one"
    g, z, ws, G = inputs(name)
    enc = encoder(g["H"])
    ref = full(name)
    zn, Gn = nan_behind(z), nan_behind(G)
    c, saved = enc._context_fwd(zn, ws)
    cn = nan_behind(c)
    gz, gi, gh, gb = enc._context_bwd(zn, cn, saved, Gn, ws[:2])
    same_bits({"c": c, "z": gz, "W_ih": gi, "W_hh": gh, "b": gb}, ref, "NaN behind z, grad_c and c")


# ------------------------------------------------------------------ 5. partial requests
@pytest.mark.parametrize("name", ["slab_plus_one", "h64_slabs"])
def test_each_gradient_alone_has_the_bits_of_the_full_call(name):
    g, z, ws, G = inputs(name)
    enc = encoder(g["H"])
    ref = full(name)
    for i, k in enumerate(R.GRADS):
        alone = run(enc, z, ws, G, tuple(j == i for j in range(4)))
        assert all(alone[o] is None for o in R.GRADS if o != k)
        assert torch.equal(bits(alone[k]), bits(ref[k])), k


# ------------------------------------------------------------------ 6. a dirty work space
def test_repeatable_after_nan_went_through_a_larger_work_space():
    small, large = inputs("slab_plus_one"), inputs("b130")
    enc = encoder(256)
    first = run(enc, *small[1:])
    poisoned = run(enc, large[1], large[2], large[3] * float("nan"))  # NaN through dA, the carry and the partials of six slabs
    assert all(torch.isnan(poisoned[k]).any() for k in R.GRADS)
    again = run(enc, *small[1:])
    same_bits(first, again, "after NaN")
    same_bits(first, full("slab_plus_one"), "another handle")
    assert all(torch.isfinite(again[k]).all() for k in R.TENSORS)
