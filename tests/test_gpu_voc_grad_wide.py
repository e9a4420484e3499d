"""-m gpu: the vocoder's gradients (``csrc/vocoder_grad.hip``, ``vqcpc_vocoder_ar_fwd`` / ``_bwd``) past the twelve cases of
tests/test_gpu_voc_grad.py -- the eight ``WIDE_CASES`` of tests/voc_grad_ref.py: frames cut by a chunk edge and a frame longer than
two chunks (``voc_frame_sum_kernel``'s clamps), row counts of one chunk on and two past a slab edge, utterances that end on, one
past and one short of each chunk edge, size_h_rnn 1024 over three batch tiles of which the middle one scores nothing, a call of one
step (the step kernel without its product), saturated gates across seven chunk edges; dim_voc_latent 128 to 1024, size_i_embed_ar
96.

Per case: the forward's bits against ``Vocoder.nll`` and ``Vocoder.condition``, then the nine gradients and ``grad_cond`` against
float64 under two judges (tests/grad_judge.py; both print every figure, then assert): per tensor ``max |G - G64| <= 4 max(e_ref,
2^-24 max |G64|)``, and for ``embedding`` per class and ``grad_cond`` per utterance and frame the same rule over one row, with rows
that are zero in float64 exact ``+0``.  tests/test_voc_grad_cpu.py holds the fp32 CPU run to both judges and shows that two seeded
faults -- no carry across a chunk edge, a cut frame that keeps its first chunk's share only -- fail them.  Nothing here is measured
on the code under test.

Then what no figure shows: guard words in front of and behind every output of the C entry points stay as they were and every word
between them is written; class values outside the table behind ``n_audio[b]``, code indices outside the table behind ``n_codes[b]``
and NaN behind an utterance's frames in ``cond_in`` and ``grad_cond`` change no bit and raise nothing; each gradient asked for alone
has the bits of the full call; a work space that a larger call drove NaN through gives the same bits again.

Observed on an MI355X over the eight cases, largest err / bound per tensor: embedding 0.310, w_ih 0.235, b_ih 0.266, b_hh 0.206,
fc1_bias 0.258, grad_cond 0.250 (all ``stressed_edges``), w_hh 0.266 and fc2_bias 0.381 (``h1024_tiles``), fc1_weight 0.318
(``slab_plus_two``), fc2_weight 0.432 (``one_step``).  Worst per-row ratio: ``embedding`` 0.520 (``h1024_tiles``, class 176), ``grad_cond``
0.441 (``stressed_edges``, utterance 1, frame 13).  Chain on ``straddle`` and ``slab_plus_two``: 0.241 among the eighteen conditioning
tensors, 0.403 among the nine of rnnms.ar ("past the cases").
"""
import ctypes

import numpy as np
import pytest
import torch

import cond_grad_ref as CR
import voc_grad_ref as R
from test_gpu_cond_grad import chain_inputs, chain_vocoder
from test_gpu_ctx_grad_wide import Guarded
from test_gpu_voc_grad import bits, inputs, run, vocoder
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

_full = {}
OUTPUTS = R.TENSORS + ("cond", "nll_sum", "n_scored", "n_correct")


def full(name):
    """(module, forward + backward of a wide case with every output): computed once and shared (read-only).  Every case with a
    chunk of its own has a module of its own."""
    if name not in _full:
        c = R.load(name)
        voc = vocoder(c)
        _full[name] = (voc, run(voc, c, cond_grad=True))
    return _full[name]


# ------------------------------------------------------------------ 1. the forward's bits, then both judges
@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_case_against_float64(name):
    c = R.load(name)
    voc, got = full(name)
    args, lens = inputs(c)
    want = voc.nll(*args, **lens)                                    # vqcpc_vocoder_nll
    assert torch.equal(bits(got["nll_sum"]), bits(want.nll_sum)) and torch.equal(got["n_scored"], want.n_scored)
    assert torch.equal(got["n_correct"], want.n_correct) and int(want.n_scored.sum()) == sum(c["slen"])
    if c["n_codes"] == [c["Tc"]] * c["B"]:
        assert torch.equal(bits(got["cond"]), bits(voc.condition(args[1], args[2])))
    for b, nc in enumerate(c["n_codes"]):
        assert not bits(got["cond"][b, 2 * nc:]).any()               # +0 past an utterance's frames
    ref = R.grads64(name)
    print(f"GPU {name}: loss {float(got['loss']):.9f}, float64 {float(ref['loss']):.9f}")
    host = {k: got[k].cpu().numpy() for k in R.TENSORS}
    R.judge(name, host, "GPU")
    R.judge_rows(name, host, "GPU")
    fed = sorted({int(x) for b, n in enumerate(c["slen"]) for x in c["audio"][b, :n]})
    emb = host["embedding"]
    assert not emb[[k for k in range(256) if k not in fed]].view(np.uint32).any() and all(emb[k].any() for k in fed)
    for b, n in enumerate(c["slen"]):                                # frames no scored step reads: +0
        used = -(-n // c["up"])
        assert not host["grad_cond"][b, used:].view(np.uint32).any(), b
        assert all(host["grad_cond"][b, f].any() for f in range(used)), b
    if name == "one_step":
        assert c["slen"] == [1, 0, 0, 1] and not host["grad_cond"][1:3].view(np.uint32).any()


@pytest.mark.parametrize("name", CR.CHAIN_WIDE)
def test_wide_chain_against_float64(name):
    c = R.load(name)
    voc = chain_vocoder(c)
    args, lens = chain_inputs(c)
    got = voc.vocoder_gradients(*args, **lens, grad_loss=c["grad_loss"])
    ref = CR.chain64(name)
    print(f"GPU chain {name}: loss {float(got['loss']):.9f}, float64 {float(ref['loss']):.9f}")
    CR.judge_chain(name, {k: got[k].cpu().numpy() for k in CR.ALL27}, "GPU")
    ar = full(name)[1]                                               # the scoring half is vqcpc_vocoder_ar_fwd / _bwd's
    assert torch.equal(bits(got["nll_sum"]), bits(ar["nll_sum"]))
    for k, n in zip(R.KEYS, CR.AR_NAMES):
        assert torch.equal(bits(got[n]), bits(ar[k])), k


# ------------------------------------------------------------------ 2. guard words, through the C entry points
@pytest.mark.parametrize("name", ["slab_plus_two", "h1024_tiles"])
def test_guard_words_around_every_output(name):
    c = R.load(name)
    voc, ref = full(name)
    args, lens = inputs(c)
    audio, z, spk, B, Tc, L, na, nc = voc._nll_call(*args, lens["lengths"], lens["n_codes"])
    ws = voc._ar_weights(voc._ar_params(), z.device)
    h, lib, s = voc._ar_handle(z.device, ws, None), _lib.load(), _lib.current_stream()
    n = ctypes.c_uint64()
    assert lib.vqcpc_vocoder_ar_saved_bytes(h, B, L, ctypes.byref(n)) == 0
    assert n.value == -(-B * (L - 1) * c["Hr"] * 4 // 256) * 256     # h_t (B, L - 1, Hr) in fp32
    sizes = {k: p.numel() * 4 for k, p in zip(R.KEYS, voc._ar_params())}
    sizes.update(grad_cond=B * 2 * Tc * c["C"] * 4, cond=B * 2 * Tc * c["C"] * 4, nll_sum=B * 8, n_scored=B * 8, n_correct=B * 8, saved=n.value)
    head = (h, audio.data_ptr(), z.data_ptr(), spk.data_ptr(), B, Tc, L, nc, na, voc._ar_struct(ws))
    runs = []
    for fill in (0xA5, 0x5A):          # a word that holds the sentinel after both runs was not written (equal inputs give equal bits)
        out = {k: Guarded(v, fill) for k, v in sizes.items()}
        grads = _lib.VocoderArTensors()
        for k in R.KEYS:
            setattr(grads, k, out[k].ptr)
        _lib.check(lib.vqcpc_vocoder_ar_fwd(*head, out["nll_sum"].ptr, out["n_scored"].ptr, out["n_correct"].ptr, out["cond"].ptr,
                                            out["saved"].ptr, s))
        _lib.check(lib.vqcpc_vocoder_ar_bwd(*head, out["saved"].ptr, None, grads, out["grad_cond"].ptr, s))
        torch.cuda.synchronize()
        for k, o in out.items():
            assert o.guards_intact(), (k, hex(fill))
        runs.append(out)
    voc.check()
    first, second = runs
    word = lambda fill: int.from_bytes(bytes([fill] * 4), "little", signed=True)
    for k in sizes:
        if k == "saved":               # its layout is private, and steps that are not scored need not be written
            continue
        a, b = first[k].words(), second[k].words()
        unwritten = (a == word(0xA5)) & (b == word(0x5A))
        assert not bool(unwritten.any()), (k, int(unwritten.sum()))
        assert torch.equal(a, b), k
        assert torch.equal(a, bits(ref[k]).view(torch.int32)), k     # the Python path's result


# ------------------------------------------------------------------ 3. what lies behind the valid data
def dirty_behind(c, codebook=512):
    """The case's ``audio`` and ``z`` on the GPU with class values -7 and 2^40 in ``audio[b, n_audio[b]:]`` and code indices -1
    and ``codebook`` in ``z[b, n_codes[b]:]``."""
    audio, z = c["audio"].clone(), c["z"].clone()
    for b, (n, nc) in enumerate(zip(c["lengths"], c["n_codes"])):
        audio[b, n:] = torch.tensor([-7, 2 ** 40] * audio.shape[1])[:audio.shape[1] - n]
        z[b, nc:] = torch.tensor([-1, codebook] * z.shape[1])[:z.shape[1] - nc]
    return audio.cuda(), z.cuda()


def nan_past_frames(t, n_codes):
    t = t.clone()
    for b, nc in enumerate(n_codes):
        t[b, 2 * nc:] = float("nan")
    return t


def test_what_lies_behind_the_valid_data_changes_no_bit():
    c = R.load("edge_ends")
    assert any(n < c["L"] for n in c["lengths"]) and any(nc < c["Tc"] for nc in c["n_codes"])
    voc, ref = full("edge_ends")
    audio, z = dirty_behind(c)
    got = voc.ar_gradients(audio, z, c["spk"].cuda(), lengths=c["lengths"], n_codes=c["n_codes"], cond_grad=True)      # ends in check()
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(ref[k])), k
    want = voc.nll(*inputs(c)[0], **inputs(c)[1])
    res = voc.nll(audio, z, c["spk"].cuda(), lengths=c["lengths"], n_codes=c["n_codes"])
    assert torch.equal(bits(res.nll_sum), bits(want.nll_sum)) and torch.equal(res.n_correct, want.n_correct)

    # the chain by hand: NaN behind the frames of the series given (ar_fwd_cond / ar_bwd_cond) and of the upstream of cond_bwd
    chain = chain_vocoder(c)
    args, lens = chain_inputs(c)
    clean = chain.vocoder_gradients(*args, **lens)
    call = chain._nll_call(audio, z, args[2], lens["lengths"], lens["n_codes"])
    nc, dev = call[7], z.device
    cw, aw = chain._cond_weights(chain._cond_params(), dev), chain._ar_weights(chain._ar_params(), dev)
    cond, csaved = chain._cond_fwd(z, args[2], nc, cw)
    cond_in = nan_past_frames(cond, c["n_codes"])
    nll_sum, n_scored, n_correct, cond_out, saved = chain._ar_fwd(call, aw, want_cond=True, cond_in=cond_in)
    ar_grads, gc = chain._ar_bwd(call, saved, aw, None, cond_grad=True, cond_in=cond_in)
    cond_grads = chain._cond_bwd(z, args[2], nc, csaved, nan_past_frames(gc, c["n_codes"]), cw)
    chain.check()
    assert torch.equal(bits(nll_sum), bits(clean["nll_sum"])) and torch.equal(n_correct, clean["n_correct"])
    assert torch.equal(bits(cond_out), bits(cond)) and torch.isfinite(gc).all()
    for k, g in zip(CR.ALL27, cond_grads + ar_grads):
        assert torch.equal(bits(g), bits(clean[k])), k
    for k, n in zip(R.KEYS, CR.AR_NAMES):
        assert torch.equal(bits(clean[n]), bits(ref[k])), k


# ------------------------------------------------------------------ 4. partial requests
def test_each_gradient_alone_has_the_bits_of_the_full_call():
    c = R.load("straddle")
    voc, ref = full("straddle")
    for k in R.KEYS:
        alone = run(voc, c, want=(k,))
        assert {o for o in R.TENSORS if o in alone} == {k}
        assert torch.equal(bits(alone[k]), bits(ref[k])), k
    alone = run(voc, c, want=(), cond_grad=True)
    assert {o for o in R.TENSORS if o in alone} == {"grad_cond"} and torch.equal(bits(alone["grad_cond"]), bits(ref["grad_cond"]))


# ------------------------------------------------------------------ 5. a dirty work space
def test_repeatable_after_nan_went_through_a_larger_work_space():
    """A handle has one model size, so the larger call is ``slab_plus_two``'s batch -- 19 utterances, a chunk of 54 steps, M = 1026
    rows -- on ``straddle``'s model, cut to the 132 steps that 11 codes of 6-step frames cover."""
    small, big = R.load("straddle"), R.load("slab_plus_two")
    voc = vocoder(small, fresh=True)
    first = run(voc, small, cond_grad=True)
    before = voc.workspace_bytes()
    for k, o in big["options"].items():
        voc.set_option(k, o)
    cover = 2 * small["up"] * big["Tc"] + 1
    poisoned = voc.ar_gradients(big["audio"].cuda(), big["z"].cuda(), big["spk"].cuda(), lengths=[min(n, cover) for n in big["lengths"]],
                                grad_loss=float("nan"), cond_grad=True)
    assert all(torch.isnan(poisoned[k]).any() for k in R.TENSORS)    # NaN through dlogit, da, dh, dgi, the carry, the tables
    for k, o in small["options"].items():
        voc.set_option(k, o)
    again = run(voc, small, cond_grad=True)
    for k in OUTPUTS:
        assert torch.equal(bits(first[k]), bits(again[k])) and torch.equal(bits(first[k]), bits(full("straddle")[1][k])), k
        assert torch.isfinite(again[k]).all(), k
    assert voc.workspace_bytes() > before
