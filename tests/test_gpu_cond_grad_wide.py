"""-m gpu: the gradients of the vocoder's conditioning path (``csrc/prenet_grad.hip``, ``vqcpc_vocoder_cond_fwd`` / ``_bwd``) past the
eleven cases of tests/test_gpu_cond_grad.py -- the ten ``WIDE_CASES`` of tests/cond_grad_ref.py: Hp = 512 (``pre_bwd_step_kernel<24>``),
row counts on and two past a slab edge, nine batch tiles with utterances without a frame among them (the first of the batch
included), a whole tile without a frame, tables of 100 x 16 and 1 x 16 and of 1024 x 40 and 7 x 24 (``pre_table_kernel``'s row and
column guards, the speaker table's unaligned column offset), and the two ends of an 80-frame chain of the back-propagation through
time with one code row per position, once through saturated gates.  The chain over all 27 tensors on two wide cases of
tests/voc_grad_ref.py is in tests/test_gpu_voc_grad_wide.py.

Per case: the forward's bits against ``Vocoder.condition`` and the handle's copies, then the eighteen gradients against float64
under two judges (tests/grad_judge.py; both print every figure, then assert): per tensor ``max |G - G64| <= 4 max(e_ref, 2^-24 max
|G64|)``, and for the two tables the same rule per code and per speaker, where ``e_ref`` of a row is the larger of two fp32 CPU
yardsticks that sum in different orders (``nn.GRU`` and a Python loop over the frames).  On ``tail`` the named rows of ``d
code_embedding`` span ten orders of magnitude and sixteen of the forty lie wholly below the tensor-wide bound: the per-tensor judge
accepts any value there.  tests/test_cond_grad_cpu.py shows it: the fp32 loop with the chain cut ``n`` frames from the upstream passes
the first judge on every tensor and fails the second.  Nothing here is measured on the code under test.

Then what no figure shows: guard words in front of and behind every output of the C entry points stay as they were and every word
between them is written; code indices outside the table behind ``n_codes[b]`` and NaN behind an utterance's frames in ``grad_cond``
change no bit and raise nothing; each gradient asked for alone has the bits of the full call; a work space that a call with more
utterances drove NaN through gives the same bits again.

Observed on an MI355X over the ten cases, largest err / bound: the tables 0.338 (speaker_embedding, ``tail_stressed``), w_ih 0.901
(layer 0 forward, ``slab_exact``: R = 1024 rows in the slab order's two accumulators; 0.367 at R = 1026; the next largest 0.593), w_hh
0.327, b_ih 0.457, b_hh 0.376.  Worst per-row ratio: ``d code_embedding`` 0.782 (``tail_stressed``, code 112, 54 frames from the upstream,
max |G64[row]| 1.1e-3 of 1.99), ``d speaker_embedding`` 0.467 (``slab_exact``, speaker 51).  Smallest row held: ``tail`` 1.4e-11 of 0.27
(worst ratio there 0.346 at code 116), ``head`` 6.7e-12 of 0.262 (0.284 at code 113) ("past the cases").
"""
import ctypes

import numpy as np
import pytest
import torch

import cond_grad_ref as R
import vectorquantizedcpc_amd as V
from test_gpu_cond_grad import bits, run, vocoder
from test_gpu_ctx_grad_wide import Guarded
from test_gpu_voc_grad_wide import dirty_behind, nan_past_frames
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

_voc, _full = {}, {}
OUTPUTS = R.KEYS + ("cond",)


def wide_vocoder(c):
    """The Vocoder of a case's sizes, tables and weight set on the GPU: the shared one of tests/test_gpu_cond_grad.py where the
    tables have the default sizes, one per table size otherwise."""
    if (c["K"], c["n_spk"]) == (R.N_CODES, R.N_SPK):
        return vocoder(c)
    key = (c["K"], c["n_spk"], c["dz"], c["ds"], c["C"], c["weights"])
    if key not in _voc:
        v = V.Vocoder(V.ConfVocoder(size_i_codebook=c["K"], n_speakers=c["n_spk"], dim_i_embedding=c["dz"], dim_speaker_embedding=c["ds"],
                                    rnnms=V.ConfRNNMSVocoder(dim_i_feature=c["dz"] + c["ds"], dim_voc_latent=c["C"],
                                                             wave_ar=V.ConfWaveAR(size_h_rnn=512))))
        v.load_state_dict(c["sd"])
        _voc[key] = v.to("cuda").eval()
    return _voc[key]


def full(name):
    """fwd + bwd of a wide case, all eighteen gradients and ``cond``: computed once and shared (read-only)."""
    if name not in _full:
        c = R.load(name)
        _full[name] = run(wide_vocoder(c), c)
    return _full[name]


# ------------------------------------------------------------------ 1. the forward's bits, then both judges
@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_case_against_float64(name):
    c = R.load(name)
    voc, got = wide_vocoder(c), full(name)                           # the caller's pointers
    z, spk = c["z"].cuda(), c["spk"].cuda()
    own = voc._cond_fwd(z, spk, V._lib.int_array(c["n_codes"], c["B"], "n_codes"), None)[0]       # NULL: the handle's copies
    assert torch.equal(bits(own), bits(got["cond"]))
    if c["n_codes"] == [c["Tc"]] * c["B"]:
        assert torch.equal(bits(got["cond"]), bits(voc.condition(z, spk)))
    voc.check()
    host = {k: got[k].cpu().numpy() for k in OUTPUTS}
    for b, n in enumerate(c["n_codes"]):                             # +0 past an utterance's frames
        assert not host["cond"][b, 2 * n:].view(np.uint32).any(), b
    R.judge(name, host, "GPU")
    R.judge_rows(name, host, "GPU")
    # rows of codes and speakers that the batch never names: +0, bit for bit
    code, sp = host["code_embedding.weight"], host["speaker_embedding.weight"]
    named, speakers = R.named_rows(c)
    assert code.shape == (c["K"], c["dz"]) and sp.shape == (c["n_spk"], c["ds"])
    assert not code[[k for k in range(c["K"]) if k not in named]].view(np.uint32).any()
    assert not sp[[s for s in range(c["n_spk"]) if s not in speakers]].view(np.uint32).any()
    assert all(code[k].any() for k in named) and all(sp[s].any() for s in speakers)


# ------------------------------------------------------------------ 2. guard words, through the C entry points
class _Ptr:
    def __init__(self, ptr):
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr


@pytest.mark.parametrize("name", ["tables_small", "dz40_ds24", "b130"])
def test_guard_words_around_every_output(name):
    c = R.load(name)
    voc, ref = wide_vocoder(c), full(name)
    B, Tc = c["B"], c["Tc"]
    z, spk, G = c["z"].cuda(), c["spk"].cuda(), c["G"].cuda()
    nc = _lib.int_array(c["n_codes"], B, "n_codes")
    cw = voc._cond_weights(voc._cond_params(), z.device)
    h, lib, s = voc._sizes_handle(z.device), _lib.load(), _lib.current_stream()
    n = ctypes.c_uint64()
    assert lib.vqcpc_vocoder_cond_saved_bytes(h, B, Tc, ctypes.byref(n)) == 0
    assert n.value == -(-B * 2 * Tc * (c["dz"] + c["ds"] + 2 * c["C"]) * 4 // 256) * 256      # series, out0, out1 over (B, 2 Tc) rows
    sizes = {k: p.numel() * 4 for k, p in zip(R.KEYS, voc._cond_params())}
    sizes.update(cond=B * 2 * Tc * c["C"] * 4, saved=n.value)
    runs = []
    for fill in (0xA5, 0x5A):          # a word that holds the sentinel after both runs was not written (equal inputs give equal bits)
        out = {k: Guarded(v, fill) for k, v in sizes.items()}
        grads = voc._cond_struct([_Ptr(out[k].ptr) for k in R.KEYS])
        _lib.check(lib.vqcpc_vocoder_cond_fwd(h, z.data_ptr(), spk.data_ptr(), B, Tc, nc, voc._cond_struct(cw), out["cond"].ptr,
                                              out["saved"].ptr, s))
        _lib.check(lib.vqcpc_vocoder_cond_bwd(h, z.data_ptr(), spk.data_ptr(), B, Tc, nc, voc._cond_struct(cw), out["saved"].ptr, G.data_ptr(),
                                              grads, s))
        torch.cuda.synchronize()
        for k, o in out.items():
            assert o.guards_intact(), (k, hex(fill))
        runs.append(out)
    voc.check()
    first, second = runs
    word = lambda fill: int.from_bytes(bytes([fill] * 4), "little", signed=True)
    for k in OUTPUTS:                  # saved: its guards only -- its layout is private, rows past the utterances' frames are not used
        a, b = first[k].words(), second[k].words()
        unwritten = (a == word(0xA5)) & (b == word(0x5A))
        assert not bool(unwritten.any()), (k, int(unwritten.sum()))
        assert torch.equal(a, b), k
        assert torch.equal(a, bits(ref[k]).view(torch.int32)), k     # the Python path's result


# ------------------------------------------------------------------ 3. what lies behind the valid data
@pytest.mark.parametrize("name", ["b130", "dead_tile"])
def test_what_lies_behind_the_valid_data_changes_no_bit(name):
    c = R.load(name)
    assert sum(n < c["Tc"] for n in c["n_codes"]) >= 16
    voc, ref = wide_vocoder(c), full(name)
    behind = dict(c, audio=torch.zeros(c["B"], 1, dtype=torch.int64), lengths=[1] * c["B"])
    _, z = dirty_behind(behind, c["K"])                              # -1 and the codebook's size behind n_codes[b]
    G = nan_past_frames(c["G"], c["n_codes"]).cuda()
    got = voc.cond_gradients(z, c["spk"].cuda(), G, n_codes=c["n_codes"])       # ends in check(): nothing is reported
    for k in OUTPUTS:
        assert torch.equal(bits(got[k]), bits(ref[k])), k


# ------------------------------------------------------------------ 4. partial requests
def test_each_gradient_alone_has_the_bits_of_the_full_call():
    c = R.load("tables_small")
    voc, ref = wide_vocoder(c), full("tables_small")
    for k in R.KEYS:
        alone = run(voc, c, want=(k,))
        assert {o for o in R.KEYS if o in alone} == {k}
        assert torch.equal(bits(alone[k]), bits(ref[k])), k


# ------------------------------------------------------------------ 5. a dirty work space
def test_repeatable_after_nan_went_through_a_work_space_of_more_utterances():
    """A handle has one model size, so the NaN call is ``hp512``'s batch -- 17 utterances of 1 to 4 codes, two batch tiles -- on
    ``tail``'s model."""
    small, big = R.load("tail"), R.load("hp512")
    voc = vocoder(small, fresh=True)
    first = run(voc, small)
    G = torch.full((big["B"], 2 * big["Tc"], small["C"]), float("nan"))
    poisoned = voc.cond_gradients(big["z"].cuda(), big["spk"].cuda(), G.cuda(), n_codes=big["n_codes"])    # NaN through dOut, dgi, dgh, the carry, dseries
    assert all(torch.isnan(poisoned[k]).any() for k in R.KEYS)
    again = run(voc, small)
    for k in OUTPUTS:
        assert torch.equal(bits(first[k]), bits(again[k])) and torch.equal(bits(first[k]), bits(full("tail")[k])), k
        assert torch.isfinite(again[k]).all(), k
