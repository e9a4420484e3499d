"""-m gpu: the vocoder's gradients (``csrc/vocoder_grad.hip``, ``vqcpc_vocoder_ar_fwd`` / ``_bwd``) -- the nine gradients of
``rnnms.ar`` and ``grad_cond`` against float64 on the twelve cases of tests/voc_grad_ref.py, the forward's bits against
``Vocoder.nll``, partial requests, repeatability on a dirty work space and the autograd surface of ``Vocoder.nll``.

Cases, reference and judge: tests/voc_grad_ref.py and tests/grad_judge.py (``judge`` prints every figure, then asserts): per tensor
``max |G - G64| <= 4 max(e_ref, 2^-24 max |G64|)``.  Nothing here is measured on the code under test.

Observed on an MI355X, largest err / bound per tensor over the twelve cases: embedding 0.256, w_ih 0.272, w_hh 0.230, b_ih 0.240, b_hh
0.225, fc1_weight 0.345, fc1_bias 0.219, fc2_weight 0.505, fc2_bias 0.610, grad_cond 0.279.
"""
import numpy as np
import pytest
import torch

import voc_grad_ref as R
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu

_voc = {}


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def conf(c):
    return V.ConfVocoder(rnnms=V.ConfRNNMSVocoder(dim_voc_latent=c["C"], upsampling_t=c["up"],
                                                  wave_ar=V.ConfWaveAR(size_i_embed_ar=c["de"], size_h_rnn=c["Hr"])))


def vocoder(c, fresh=False):
    """The Vocoder of a case's sizes and weight set on the GPU, with the case's options set.  Cases without options share one per
    size and weight set, which therefore keeps the library's defaults; a case that carries options gets a module of its own, so
    no option is ever set back."""
    key = (c["Hr"], c["de"], c["C"], c["up"], c["weights"])
    if fresh or c["options"] or key not in _voc:
        v = V.Vocoder(conf(c))
        v.load_state_dict(c["sd"])
        v = v.to("cuda").eval()
        for k, o in c["options"].items():
            v.set_option(k, o)
        if fresh or c["options"]:
            return v
        _voc[key] = v
    return _voc[key]


def inputs(c):
    return (c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda()), dict(lengths=c["lengths"], n_codes=c["n_codes"])


def run(voc, c, **kw):
    args, lens = inputs(c)
    return voc.ar_gradients(*args, **lens, grad_loss=c["grad_loss"], **kw)


# ------------------------------------------------------------------ 1. against float64
@pytest.mark.parametrize("name", R.ALL_CASES)
def test_gradients_against_float64(name):
    c = R.load(name)
    voc = vocoder(c)
    got = run(voc, c, cond_grad=True)
    if name == "b32_big":                                            # ar_gru_big_kernel ran the forward
        assert voc.kernel_times(1)[4] == 2.0
    ref = R.grads64(name)
    loss = float(got["loss"])
    print(f"GPU {name}: loss {loss:.9f}, float64 {float(ref['loss']):.9f}")      # the forward's own bound: tests/test_gpu_vocoder_nll.py
    host = {k: got[k].cpu().numpy() for k in R.TENSORS}
    if name == "const_audio":                                        # rows of classes never fed: +0, bit for bit
        rows = np.arange(256) != 77
        assert not host["embedding"][rows].view(np.uint32).any() and host["embedding"][77].any()
    if name == "ragged":                                             # frames no scored step reads: +0
        for b, (n, nc) in enumerate(zip(c["slen"], c["n_codes"])):
            used = (n + c["up"] - 1) // c["up"]
            assert not host["grad_cond"][b, used:].view(np.uint32).any(), b
            assert used == 0 or host["grad_cond"][b, :used].any(), b
    R.judge(name, host, "GPU")


# ------------------------------------------------------------------ 2. the forward is Vocoder.nll's
@pytest.mark.parametrize("name", ["ragged", "chunks", "b32_big", "h1024"])
def test_forward_bits_equal_the_scoring_entry(name):
    c = R.load(name)
    voc = vocoder(c)
    args, lens = inputs(c)
    want = voc.nll(*args, **lens)
    call = voc._nll_call(*args, lens["lengths"], lens["n_codes"])
    own = voc._ar_fwd(call, None, want_cond=True)                                           # NULL: the handle's copies
    mine = voc._ar_fwd(call, voc._ar_weights(voc._ar_params(), args[0].device))             # the caller's pointers
    cond = voc.condition(args[1], args[2]) if c["n_codes"] == [c["Tc"]] * c["B"] else None
    for got in (own, mine):
        assert torch.equal(bits(got[0]), bits(want.nll_sum)) and torch.equal(got[1], want.n_scored) and torch.equal(got[2], want.n_correct)
    assert int(want.n_scored.sum()) == sum(c["slen"])
    if cond is not None:
        assert torch.equal(bits(own[3]), bits(cond))
    for b, nc in enumerate(c["n_codes"]):
        assert not bits(own[3][b, 2 * nc:]).any()                    # +0 past an utterance's frames


def test_forward_with_moved_weights_has_the_bits_of_a_handle_made_from_them():
    c = R.load("h512")
    voc = vocoder(c, fresh=True)
    args, lens = inputs(c)
    voc.nll(*args, **lens)                                           # a live handle with the old weights
    handle = voc._handle.value
    moved = [p.detach() * 1.25 for p in voc._ar_params()]
    call = voc._nll_call(*args, lens["lengths"], lens["n_codes"])
    got = voc._ar_fwd(call, voc._ar_weights(moved, args[0].device))
    assert voc._handle.value == handle
    other = vocoder(c, fresh=True)
    with torch.no_grad():
        for p, w in zip(other._ar_params(), moved):
            p.copy_(w)
    want = other.nll(*args, **lens)
    assert torch.equal(bits(got[0]), bits(want.nll_sum)) and torch.equal(got[2], want.n_correct)
    g1 = voc.ar_gradients(*args, **lens, weights=moved, cond_grad=True)
    g2 = other.ar_gradients(*args, **lens, cond_grad=True)
    saved = other._ar_fwd(call, None)[4]                             # NULL: the copies in the handle `other.nll` made
    grads, gc = other._ar_bwd(call, saved, None, cond_grad=True)
    g3 = dict(zip(R.KEYS, grads), grad_cond=gc)
    for k in R.TENSORS:
        assert torch.equal(bits(g1[k]), bits(g2[k])) and torch.equal(bits(g2[k]), bits(g3[k])), k


def test_a_new_state_dict_behind_a_live_handle_is_not_missed():
    """The gradient entries read the nine tensors of rnnms.ar from the caller but the two embedding tables and the prenet from the
    handle's copies: after ``load_state_dict`` (or an in-place write to a frozen tensor) behind a live handle they must give the
    bits of a fresh module built from the new state dict -- while a step on rnnms.ar alone keeps the handle."""
    c = R.load("h512")
    args, lens = inputs(c)
    other_sd = synth.vocoder_state_dict(seed=99, dim_voc_latent=c["C"], size_i_embed_ar=c["de"], size_h_rnn=c["Hr"])
    fresh = V.Vocoder(conf(c))
    fresh.load_state_dict(other_sd)
    fresh = fresh.cuda().eval()
    want = fresh.ar_gradients(*args, **lens, cond_grad=True)
    want_nll = fresh.nll(*args, **lens)
    spk_table = fresh.speaker_embedding.weight.detach().clone()

    for use in ("ar_gradients", "nll"):
        voc = vocoder(c, fresh=True)
        voc.nll(*args, **lens)                                       # a live handle with the first state dict's copies
        voc.load_state_dict(other_sd)
        if use == "ar_gradients":
            got = voc.ar_gradients(*args, **lens, cond_grad=True)
            for k in R.TENSORS + ("cond", "nll_sum"):
                assert torch.equal(bits(got[k]), bits(want[k])), k
        else:
            res = voc.nll(*args, **lens, differentiable=True)
            assert torch.equal(bits(res.nll_sum), bits(want_nll.nll_sum)) and torch.equal(res.n_correct, want_nll.n_correct)
            res.loss.backward()
            for k, p in zip(voc.AR_KEYS, voc._ar_params()):
                assert torch.equal(bits(p.grad), bits(want[k])), k
        # an in-place write to one frozen tensor alone, then to one of rnnms.ar alone
        with torch.no_grad():
            voc.speaker_embedding.weight.mul_(1.5)
            fresh.speaker_embedding.weight.copy_(spk_table * 1.5)
        moved = fresh.ar_gradients(*args, **lens, cond_grad=True)
        got = voc.ar_gradients(*args, **lens, cond_grad=True)
        assert not torch.equal(bits(moved["cond"]), bits(want["cond"]))
        for k in R.TENSORS + ("cond",):
            assert torch.equal(bits(got[k]), bits(moved[k])), k
        handle = voc._handle.value
        with torch.no_grad():
            voc.rnnms.ar.fc2.bias.add_(0.25)
        voc.ar_gradients(*args, **lens)
        assert voc._handle.value == handle                           # a step on rnnms.ar costs no new handle
        with torch.no_grad():                                        # `fresh` as it was, for the second round
            fresh.speaker_embedding.weight.copy_(spk_table)


# ------------------------------------------------------------------ 3. partial requests
@pytest.mark.parametrize("name", ["ragged", "chunks"])
def test_partial_requests_give_the_bits_of_the_full_call(name):
    c = R.load(name)
    voc = vocoder(c)
    full = run(voc, c, cond_grad=True)
    for want, cg in ((("fc2_weight", "fc2_bias"), False), ((), True), (("w_hh",), False), (("fc1_bias",), False), (("embedding", "b_ih"), False)):
        part = run(voc, c, want=want, cond_grad=cg)
        assert {k for k in R.TENSORS if k in part} == set(want) | ({"grad_cond"} if cg else set())
        for k in want + (("grad_cond",) if cg else ()):
            assert torch.equal(bits(part[k]), bits(full[k])), (want, k)
    with pytest.raises(RuntimeError, match="no wanted output"):
        run(voc, c, want=())


# ------------------------------------------------------------------ 4. equal inputs, equal bits, on a work space that is dirty
def test_repeatable_on_a_dirty_work_space():
    small, large = R.load("ragged"), R.load("b17")
    voc = vocoder(small, fresh=True)
    first = run(voc, small, cond_grad=True)
    before = voc.workspace_bytes()
    run(voc, large, cond_grad=True)                                  # another shape: the work space is left full of it
    second = run(voc, small, cond_grad=True)
    args, lens = inputs(large)
    voc.ar_gradients(*args, **lens, grad_loss=float("nan"), cond_grad=True)      # NaN through the backward's buffers: dlogit, da, dh, dgi, the carry, the tables
    third = run(voc, small, cond_grad=True)
    for k in R.TENSORS + ("nll_sum",):
        assert torch.equal(bits(first[k]), bits(second[k])) and torch.equal(bits(first[k]), bits(third[k])), k
        assert torch.isfinite(third[k]).all(), k
    assert voc.workspace_bytes() >= before


# ------------------------------------------------------------------ 5. the autograd surface
def test_autograd_surface():
    c = R.load("ragged")
    args, lens = inputs(c)
    direct = vocoder(c).ar_gradients(*args, **lens)
    voc = vocoder(c, fresh=True)
    plain = voc.nll(*args, **lens)
    with torch.no_grad():
        quiet = voc.nll(*args, **lens, differentiable=True)
    assert plain.loss.grad_fn is None and quiet.loss.grad_fn is None
    res = voc.nll(*args, **lens, differentiable=True)
    assert res.loss.requires_grad and res.loss.dtype == torch.float64
    assert torch.equal(bits(res.nll_sum), bits(plain.nll_sum)) and torch.equal(res.n_correct, plain.n_correct)
    assert torch.equal(bits(res.loss.detach()), bits(plain.loss))
    res.loss.backward()
    for k, p in zip(voc.AR_KEYS, voc._ar_params()):
        assert torch.equal(bits(p.grad), bits(direct[k])), k
    frozen = [voc.code_embedding.weight, voc.speaker_embedding.weight] + list(voc.rnnms.prenet.parameters())
    assert all(p.grad is None for p in frozen)

    # only the parameters that require a gradient are asked for; an upstream factor scales them
    voc = vocoder(c, fresh=True)
    for p in voc._ar_params()[:5]:
        p.requires_grad_(False)
    (voc.nll(*args, **lens, differentiable=True).loss * 2.0).backward()
    assert all(p.grad is None for p in voc._ar_params()[:5])
    scaled = vocoder(c).ar_gradients(*args, **lens, grad_loss=2.0)
    for k, p in list(zip(voc.AR_KEYS, voc._ar_params()))[5:]:
        assert torch.equal(bits(p.grad), bits(scaled[k])), k
    for p in voc._ar_params():
        p.requires_grad_(False)
    assert voc.nll(*args, **lens, differentiable=True).loss.grad_fn is None

    # five optimizer steps: the handle is not rebuilt, every step reads the moved weights, and the loss falls
    voc = vocoder(c, fresh=True)
    voc.nll(*args, **lens)
    opt = torch.optim.SGD(voc.rnnms.ar.parameters(), lr=0.5)
    handles, values = set(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = voc.nll(*args, **lens, differentiable=True).loss
        loss.backward()
        opt.step()
        handles.add(voc._handle.value)
        values.append(float(loss.detach()))
    assert len(handles) == 1 and all(a > b for a, b in zip(values, values[1:])), values
    fresh = voc.nll(*args, **lens)                                   # through _native(): rebuilt once, reads the stepped weights
    again = voc._ar_fwd(voc._nll_call(*args, lens["lengths"], lens["n_codes"]), voc._ar_weights(voc._ar_params(), args[0].device))
    assert torch.equal(bits(fresh.nll_sum), bits(again[0])) and float(fresh.loss) < values[-1]
