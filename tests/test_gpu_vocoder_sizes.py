"""-m gpu: the vocoder against float64 at every model size vqcpc_vocoder_create accepts (cases, references, yardstick and judge:
tests/vocoder_size_cases.py; the judge's own checks: tests/test_vocoder_sizes_cpu.py).

Everything goes through ``Vocoder``.  Per case: every conditioning frame at Tc in {1, 2, 17} x B in {1, 17}; teacher-forced
logits at Ts in {1, upsampling_t + 1, 2 up Tc} (B = 2, Tc = 3) and B = 17; the launch path free-running on ragged utterances, draw
by draw on the GPU's own history -- one tile (fused and three-launch schedules, graphs and plain launches, steps_per_graph dividing
upsampling_t and not: the same bits), two tiles, and on three cases the large-batch kernel at five tiles; every case asserts the
path, the slot count and (kernel_times()[4]) the GRU-step kernel it ran.  The two cases with the reference's 896 / 256 / 8 bit but
other embedding, prenet, glue widths and hop run the resident decoders by default (path 2; path 3 with xcm = 1): bit-equal to the
launch path, checked against float64, and streamed in chunks of k * upsampling_t.  Vocoder.nll at size_h_rnn 1024 and 512 with the
reference head; its explicit error elsewhere; sizes outside the lists raise at first use.

Tolerances are computed when the test runs, from the CPU yardsticks alone: tol = 10 * max(e32, 2^-23 max|ref|) per case and
quantity; every test prints e32, tol and what it observed.  Observed on MI355X (e32 moves by some 10 % with the host's BLAS):

  ===============  ========  ========  ========  =========  =========  =========
  case             cond e32  cond tol  cond GPU  logit e32  logit tol  logit GPU
  ===============  ========  ========  ========  =========  =========  =========
  ref_small_glue   2.4e-7    2.4e-6    2.9e-7    8.8e-8     8.8e-7     1.1e-7
  ref_wide_prenet  6.3e-7    6.3e-6    8.2e-7    2.4e-7     2.4e-6     2.7e-7
  min              2.1e-7    2.1e-6    2.3e-7    5.0e-8     5.0e-7     6.5e-8
  hf512            4.1e-7    4.1e-6    5.0e-7    1.2e-7     1.2e-6     1.3e-7
  hf768            4.5e-7    4.5e-6    4.2e-7    2.5e-7     2.5e-6     2.5e-7
  hf1024_b10       3.6e-7    3.6e-6    4.7e-7    1.3e-7     1.3e-6     1.8e-7
  hr1024           3.3e-7    3.3e-6    4.1e-7    1.2e-7     1.2e-6     1.7e-7
  max              5.8e-7    5.8e-6    7.5e-7    2.8e-7     2.8e-6     2.7e-7
  ===============  ========  ========  ========  =========  =========  =========

All 49 528 draws checked are exact (the share asked for is 99 %, none outside W); Vocoder.nll per sample 9.4e-7 / 9.5e-7 at
size_h_rnn 1024 / 512, 0.094 / 0.092 of its bound.
"""
import re

import numpy as np
import pytest
import torch

import nll_ref
import oracle
import vectorquantizedcpc_amd as V
import vocoder_size_cases as S
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

DEFAULTS = {"xcd": -1, "xcm": -1, "big_min_tiles": 5, "fuse_fc2": 1, "use_graph": 1, "steps_per_graph": 160}
_voc = {}
_mulaw = {}


def vocoder(name):
    if name not in _voc:
        v = V.Vocoder(S.conf(name))
        v.load_state_dict(S.sd(name))
        _voc[name] = v.to("cuda").eval()
    return _voc[name]


def mulaw_table(bits):
    if bits not in _mulaw:
        _mulaw[bits] = np.array([oracle.mulaw_decode(k, bits) for k in range(1 << bits)], np.float32)
    return _mulaw[bits]


def free_run(name, B, opts):
    """generate() of the case's B-utterance input set under `opts` -> (wav, mu, path, slots, GRU kernel kind or None)."""
    voc = vocoder(name)
    z, spk, n_codes, ids = S.draw_inputs(name, B)
    try:
        for k, v in opts.items():
            voc.set_option(k, v)
        wav, mu = voc.generate(z.cuda(), spk.cuda(), n_codes=n_codes, seed=S.SEED, utt_ids=ids, return_mulaw=True)
        path, slots = voc.last_path(), voc.last_slots()
        kind = voc.kernel_times(3)[4] if path == 0 else None
    finally:
        for k in opts:
            voc.set_option(k, DEFAULTS[k])
    return wav.cpu().numpy(), mu.cpu().numpy(), path, slots, kind


def check_waveform(name, B, wav, mu):
    """wav = the mu-law table of the draws; zeros behind every utterance; the upper classes are drawn where there are any."""
    c = S.CASES[name]
    n_codes = S.draw_inputs(name, B)[2]
    tab = mulaw_table(c["bits"])
    assert mu.shape == wav.shape == (B, 2 * c["up"] * max(n_codes))
    assert mu.min() >= 0 and mu.max() < S.n_cls(name)
    for b in range(B):
        L = 2 * c["up"] * n_codes[b]
        assert np.array_equal(wav[b, :L], tab[mu[b, :L]]), (name, b)
        assert not wav[b, L:].any() and not mu[b, L:].any(), (name, b)
    if c["bits"] > 8:
        assert int((mu >= S.n_cls(name) // 2).sum()) > 0, "no draw at or above n_cls / 2"


def check_draws(name, B, mu, what):
    z, spk, n_codes, ids = S.draw_inputs(name, B)
    ok, exact, gap, bad, n = S.judge_draws(name, mu, z, spk, n_codes, ids, rows=S.draw_rows(B), what=what)
    assert ok, (name, what, exact, gap, bad)


def same_bits(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


# ---------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("name", S.NAMES)
def test_conditioning_every_frame(name):
    voc, want = vocoder(name), S.cond_reference(name)
    z, spk = S.cond_inputs(name)
    worst = 0.0
    for Tc in S.COND_TC:
        for B in (1, 17):
            got = voc.condition(z[:B, :Tc].cuda(), spk[:B].cuda()).cpu().numpy()
            assert got.shape == (B, 2 * Tc, 2 * S.CASES[name]["hp"])
            ok, err = S.judge_cond(name, got, want[Tc][:B], "GPU Tc %d B %d" % (Tc, B))
            worst = max(worst, err)
            assert ok, (name, Tc, B, err)
    print("%s: conditioning, max |GPU - f64| = %.3g, e32 %.3g, tol %.3g" % ((name, worst) + S.tolerances(name)["cond"][:2]))


# ---------------------------------------------------------------------- teacher-forced logits
@pytest.mark.parametrize("name", S.NAMES)
def test_teacher_forced_logits(name):
    voc = vocoder(name)
    worst = 0.0
    z, spk, x = S.tf_inputs(name, "b2")
    want = S.tf_reference(name, "b2")
    if S.CASES[name]["bits"] > 8:
        assert int((x >= S.n_cls(name) // 2).sum()) > 0
    for Ts in S.tf_lengths(name):
        got = voc(x[:, :Ts].cuda(), z.cuda(), spk.cuda()).cpu().numpy()
        assert voc.last_path() == 0 and got.shape == (2, Ts, S.n_cls(name))
        ok, err = S.judge_logits(name, got, want[:, :Ts], what="GPU B 2 Ts %d" % Ts)
        worst = max(worst, err)
        assert ok, (name, Ts, err)
    z, spk, x = S.tf_inputs(name, "b17")
    got = voc(x.cuda(), z.cuda(), spk.cuda()).cpu().numpy()
    assert voc.last_path() == 0 and voc.last_slots() == 17
    ok, err = S.judge_logits(name, got, S.tf_reference(name, "b17"), what="GPU B 17")
    worst = max(worst, err)
    assert ok, (name, err)
    print("%s: logits, max |GPU - f64| = %.3g, e32 %.3g, tol %.3g" % ((name, worst) + S.tolerances(name)["logit"][:2]))


# ---------------------------------------------------------------------- launch path, free running
@pytest.mark.parametrize("name", S.NAMES)
def test_launch_path_one_tile_every_schedule(name):
    """B = 3: the fused fc2 || GRU launch (kernel kind 4) against float64; the three-launch schedule (kind 0), plain launches
    instead of graphs, and steps_per_graph = upsampling_t (one conditioning row per replay) and 64 (which divides no case's hop:
    rows fetched per step) give the same bits."""
    up = S.CASES[name]["up"]
    assert up % 2 == 0 and up % 64 != 0
    base = free_run(name, 3, {"xcd": 0})
    assert base[2:] == (0, 3, 4.0), base[2:]
    check_waveform(name, 3, base[0], base[1])
    check_draws(name, 3, base[1], "launch path, one tile")
    for opts, kind in (({"fuse_fc2": 0}, 0.0), ({"use_graph": 0}, 4.0), ({"steps_per_graph": up}, 4.0), ({"steps_per_graph": 64}, 4.0)):
        other = free_run(name, 3, dict(opts, xcd=0))
        assert other[2:] == (0, 3, kind), (opts, other[2:])
        assert same_bits(base, other), (name, opts)


@pytest.mark.parametrize("name", S.NAMES)
def test_launch_path_two_tiles(name):
    got = free_run(name, 20, {"xcd": 0})
    assert got[2:] == (0, 20, 4.0), got[2:]
    check_waveform(name, 20, got[0], got[1])
    check_draws(name, 20, got[1], "launch path, two tiles")


@pytest.mark.parametrize("name", S.BIG)
def test_launch_path_large_batch_kernel(name):
    """80 utterances = 5 tiles with big_min_tiles = 5: ar_gru_big_kernel, fused (kind 5) and three-launch (kind 2), the same bits."""
    got = free_run(name, 80, {"xcd": 0, "big_min_tiles": 5})
    assert got[2:] == (0, 80, 5.0), got[2:]
    check_waveform(name, 80, got[0], got[1])
    check_draws(name, 80, got[1], "large-batch kernel")
    other = free_run(name, 80, {"xcd": 0, "big_min_tiles": 5, "fuse_fc2": 0})
    assert other[2:] == (0, 80, 2.0), other[2:]
    assert same_bits(got, other)


# ---------------------------------------------------------------------- resident decoders at the reference's 896 / 256 / 8 bit
@pytest.mark.parametrize("B,opts,path", [(5, {}, 2), (12, {}, 2), (32, {}, 2), (19, {"xcm": 1}, 3)])
@pytest.mark.parametrize("name", S.RESIDENT)
def test_resident_decoders(name, B, opts, path):
    got = free_run(name, B, opts)
    assert got[2:4] == (path, B), got[2:4]
    check_waveform(name, B, got[0], got[1])
    check_draws(name, B, got[1], "path %d, %d slots" % (path, B))
    launch = free_run(name, B, {"xcd": 0})
    assert launch[2] == 0 and same_bits(got, launch)


@pytest.mark.parametrize("name", S.RESIDENT)
def test_stream_chunks_of_k_hops(name):
    """generate_stream in chunks of upsampling_t and 3 upsampling_t on the resident decoders, and of 2 upsampling_t on the launch path."""
    voc, up = vocoder(name), S.CASES[name]["up"]
    for B, k, opts, path in ((5, 1, {}, 2), (5, 3, {}, 2), (3, 2, {"xcd": 0}, 0)):
        z, spk, n_codes, ids = S.draw_inputs(name, B)
        kw = dict(n_codes=n_codes, seed=S.SEED, utt_ids=ids, return_mulaw=True)
        try:
            for o, v in opts.items():
                voc.set_option(o, v)
            want_w, want_m = voc.generate(z.cuda(), spk.cuda(), **kw)
            assert voc.last_path() == path
            ws, ms = [], []
            for w, m in voc.generate_stream(z.cuda(), spk.cuda(), chunk_samples=k * up, **kw):
                assert voc.last_path() == path
                ws.append(w)
                ms.append(m)
        finally:
            for o in opts:
                voc.set_option(o, DEFAULTS[o])
        assert len(ws) == -(-want_w.shape[1] // (k * up))
        assert torch.equal(torch.cat(ms, 1), want_m) and torch.equal(torch.cat(ws, 1), want_w), (name, B, k)
        assert int((want_m != 0).sum()) > want_m.numel() // 4


# ---------------------------------------------------------------------- Vocoder.nll
@pytest.mark.parametrize("name", ["hr1024", "hr512_refhead"])
def test_nll_with_the_reference_head(name):
    """size_h_rnn 1024 and 512 under size_h_fc 256 / 8 bit: the bound of tests/nll_ref.py with the case's own logit tolerance."""
    c = S.nll_inputs(name)
    ref = nll_ref.Ref(name, c["audio"], c["z"], c["spk"], c["n_codes"], c["lengths"], sd=S.sd(name), upsample=S.CASES[name]["up"],
                      tol=S.tolerances(name)["logit"][1])
    assert ref.ambiguous_fraction() <= nll_ref.AMBIGUOUS_CAP
    res = vocoder(name).nll(c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda(), lengths=c["lengths"], n_codes=c["n_codes"], per_sample=True)
    assert vocoder(name).last_path() == 0
    nll_ref.check_result(ref, res.nll_sum.cpu().numpy(), res.n_scored.cpu().numpy(), res.n_correct.cpu().numpy(), res.nll.cpu().numpy(), what=name)


@pytest.mark.parametrize("name", ["hf768", "hf1024_b10"])
def test_nll_refuses_another_head_and_enqueues_nothing(name):
    voc = vocoder(name)
    c = S.nll_inputs(name)
    with pytest.raises(RuntimeError, match="scoring head is built for size_h_fc 256 and 256 classes"):
        voc.nll(c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda(), lengths=c["lengths"], n_codes=c["n_codes"])
    # the C call itself, on buffers of our own: not one of them is touched (the call's memsets would zero them)
    audio, z, spk = c["audio"].cuda(), c["z"].cuda(), c["spk"].cuda()
    s = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
    n = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    k = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    per = torch.full((3, audio.shape[1] - 1), 7.0, device="cuda")
    rc = _lib.load().vqcpc_vocoder_nll(voc._native(), audio.data_ptr(), z.data_ptr(), spk.data_ptr(), 3, 2, audio.shape[1],
                                       _lib.int_array(c["n_codes"], 3, "n_codes"), _lib.int_array(c["lengths"], 3, "lengths"),
                                       s.data_ptr(), n.data_ptr(), k.data_ptr(), per.data_ptr(), _lib.current_stream())
    assert rc != 0
    torch.cuda.synchronize()
    assert bool((s == 7.0).all()) and bool((n == 7).all()) and bool((k == 7).all()) and bool((per == 7.0).all())
    voc.check()                                                      # and nothing is left latched


# ---------------------------------------------------------------------- sizes outside the lists
@pytest.mark.parametrize("override,message", [
    (dict(h_fc=384), "size_h_fc must be 256"), (dict(bits=7), "bits_mu_law must be 8"), (dict(bits=11), "bits_mu_law must be 8"),
    (dict(hp=96), "Hp %"), (dict(embed_ar=48), "size_i_embed_ar % 32"), (dict(dz=16, ds=32), re.escape("dz+ds %")),
    (dict(up=0), "upsample_t must be positive")])
def test_size_outside_the_lists_raises_at_first_use(override, message):
    v = V.Vocoder(S.conf("min", **override))
    v.load_state_dict(S.state_dict("min", **override))
    v = v.to("cuda").eval()
    z, spk, _, _ = S.draw_inputs("min", 3)
    with pytest.raises(RuntimeError, match=message):
        v.generate(z.cuda(), spk.cuda(), seed=1, utt_base=0, max_steps=8)
