"""The vocoder gradients without a GPU: the float64 reference of tests/voc_grad_ref.py reproduces its pins and equals torch's own
modules, the ctypes struct names the module's tensors, the cases meet the conditions the GPU tests rely on, and the recorded
float64 fit is a trend, not noise.  Past the twelve cases: the wide cases reproduce their pins, row pins included, hold the
arithmetic their table claims, their fp32 CPU run passes both judges, and two seeded faults fail them."""
import numpy as np
import pytest

import grad_judge
import voc_fit_ref
import voc_grad_ref as R
from vectorquantizedcpc_amd import _lib, cli, driver


@pytest.mark.parametrize("name", R.ALL_CASES)
def test_reference_reproduces_its_pins(name):
    grad_judge.check_pins(R.grads64(name), R.pins(), name, R.TENSORS, R.POSITIONS)


@pytest.mark.parametrize("name", R.MODULE_CASES)
def test_reference_equals_torch_modules(name):
    """``nn.Embedding`` + ``nn.GRU`` + ``nn.Linear`` + ``F.cross_entropy`` autograd from the same state dict, within 1e-12 relative."""
    ref, mod = R.grads64(name), R.module_grads(name)
    assert len(set(R.load(name)["lengths"])) == 1
    for k in R.TENSORS + ("loss",):
        top = float(np.abs(mod[k]).max())
        assert top > 0 and float(np.abs(ref[k] - mod[k]).max()) <= 1e-12 * top, (k, float(np.abs(ref[k] - mod[k]).max()), top)


def test_cases_meet_their_conditions():
    cs = {n: R.load(n) for n in R.ALL_CASES}
    for n, c in cs.items():
        assert len(c["lengths"]) == len(c["n_codes"]) == c["B"] and c["L"] >= max(c["lengths"])
        for s, nc in zip(c["slen"], c["n_codes"]):
            assert 0 <= nc <= c["Tc"] and s <= 2 * c["up"] * nc, n
        assert max(c["slen"]) <= 1300 and sum(c["slen"]) > 0
    c = cs["ref_sizes"]
    assert (c["Hr"], c["de"], c["C"], c["up"], c["B"], c["Tc"], c["L"]) == (896, 256, 256, 160, 2, 1, 321) and max(c["slen"]) == 5 * 64
    c = cs["ragged"]
    s, up = c["slen"], c["up"]
    assert c["B"] == 5 and s[0] == 0 and s[1] == 2 * up * c["n_codes"][1] and s[2] % up and s[2] < 2 * up * c["n_codes"][2]
    assert s[4] > 64 and s[4] % 64 and s[3] % 64 and len(set(c["n_codes"])) == 5
    c = cs["chunks"]
    ch = c["options"]["tf_chunk_replays"] * 160                      # steps_per_graph at its default
    s = sorted(c["slen"])
    assert -(-s[-1] // ch) == 3 and s[-1] % ch and any(ch < v < 2 * ch for v in s)
    assert cs["b1"]["B"] == 1 and cs["b17"]["B"] == 17 and cs["b32_big"]["B"] == 32 and cs["b32_big"]["options"] == {"big_min_tiles": 2}
    assert (cs["h512"]["Hr"], cs["h1024"]["Hr"]) == (512, 1024) and all(cs[n]["de"] == 32 and cs[n]["C"] == 128 for n in ("h512", "h1024"))
    assert cs["stressed"]["weights"] == "stressed" and cs["upstream"]["grad_loss"] not in (None, 1.0)
    a = cs["const_audio"]["audio"]
    assert int(a.min()) == int(a.max()) == 77
    emb = R.grads64("const_audio")["embedding"]
    assert not emb[np.arange(256) != 77].any() and emb[77].any()     # the float64 reference: rows of classes never fed are zero
    gc = R.grads64("ragged")["grad_cond"]
    for b, n in enumerate(cs["ragged"]["slen"]):
        assert not gc[b, -(-n // 8):].any()                          # frames no scored step reads
    assert -(-max(cs["long"]["slen"]) // 640) == 3                   # three chunks at the default chunk of 640


# ------------------------------------------------------------------ past the twelve: WIDE_CASES
@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_wide_reference_reproduces_its_pins(name):
    grad_judge.check_pins(R.grads64(name), R.pins(), name, R.TENSORS, R.POSITIONS)
    grad_judge.check_row_pins(R.grads64(name), R.pins(), name, R.ROW_TENSORS)


def test_wide_cases_cover_what_they_name():
    cs = {n: R.load(n) for n in R.ALL_WIDE}
    for n, c in cs.items():
        assert len(c["lengths"]) == len(c["n_codes"]) == c["B"] and c["L"] >= max(c["lengths"])
        for na, nc in zip(c["lengths"], c["n_codes"]):
            assert 0 <= nc <= c["Tc"] and na - 1 <= 2 * c["up"] * nc, n          # n_audio - 1 <= 2 up n_codes
        ch = R.chunk_of(c)
        assert ch % 2 == 0 and ch >= 2 and sum(c["slen"]) > 0
    # straddle: seven chunks, the last with 12 steps; four of the six chunk edges cut a frame; two tiles; de = 96
    c = cs["straddle"]
    ch, up, longest = R.chunk_of(c), c["up"], max(c["slen"])
    assert (ch, up, longest) == (16, 6, 108) and ch % up and -(-longest // ch) == 7 and longest % ch == 12 and c["B"] == 19 and c["de"] == 96
    cut = [f for f in range(longest // up) if (f * up) // ch != (f * up + up - 1) // ch]
    assert cut == [2, 5, 10, 13]                                     # the edges at 16, 32, 64 and 80; 48 and 96 fall between two frames
    assert sorted(set(c["slen"])) == [108 - 5 * i for i in range(6, -1, -1)]
    # frame_over_chunks: a frame spans two and a half chunks, and chunks lie wholly inside one frame
    c = cs["frame_over_chunks"]
    ch, up = R.chunk_of(c), c["up"]
    assert up == 2.5 * ch and any(t0 // up == (t0 + ch - 1) // up and t0 % up for t0 in range(0, max(c["slen"]), ch))
    # edge_ends: on, one past and one short of each chunk edge
    c = cs["edge_ends"]
    assert R.chunk_of(c) == 16 and c["slen"] == [16, 17, 15, 32, 33, 31, 48]
    # the slab edge: M = B CH rows per chunk, GRAD_SLAB = 1024
    c = cs["slab_exact"]
    assert c["B"] * R.chunk_of(c) == 1024 and min(c["slen"]) == 2 * R.chunk_of(c) == 128
    c = cs["slab_plus_two"]
    ch = R.chunk_of(c)
    assert c["B"] * ch == 1026 and (c["C"], c["de"]) == (1024, 32) and -(-max(c["slen"]) // ch) == 3
    for r in (1024, 1025):                                           # rows 1024 and 1025 are live in the first two chunks
        b, tt = divmod(r, ch)
        assert b == 18 and [t0 + tt < c["slen"][b] for t0 in (0, ch, 2 * ch)] == [True, True, False]
    # h1024_tiles: three tiles, the middle one scores nothing, one live column in the last
    c = cs["h1024_tiles"]
    assert (c["Hr"], c["C"], c["B"]) == (1024, 512, 33) and 3 * c["Hr"] // 64 == 48
    assert not any(c["slen"][16:32]) and not any(c["n_codes"][16:32]) and c["lengths"][16:32] == [1] * 16
    assert c["lengths"][5] == 0 and c["slen"][32] == 48 and sum(1 for s in c["slen"][:16] if s) == 15
    c = cs["one_step"]
    assert max(c["slen"]) == 1 and sum(c["slen"]) == 2 and c["slen"] == [1, 0, 0, 1]
    c = cs["stressed_edges"]
    assert c["weights"] == "stressed" and -(-max(c["slen"]) // R.chunk_of(c)) - 1 == 7
    assert sorted({cs[n]["C"] for n in cs}) == [128, 256, 512, 1024]
    # the float64 reference: frames no scored step reads are zero, one_step's dead utterances receive nothing
    for n, c in cs.items():
        gc = R.grads64(n)["grad_cond"]
        for b, s in enumerate(c["slen"]):
            assert not gc[b, -(-s // c["up"]):].any() and all(gc[b, f].any() for f in range(-(-s // c["up"]))), (n, b)


def _as_fp32(g):
    return {k: v.astype(np.float32) for k, v in g.items()}


def _ratios(name, got):
    """err / bound of the per-tensor judge, per tensor."""
    ref, p = R.grads64(name), R.pins()
    return {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) / grad_judge.bound(p, name, k) for k in R.TENSORS}


@pytest.mark.parametrize("name", R.ALL_WIDE)
def test_fp32_yardstick_passes_both_judges(name):
    import torch
    low = _as_fp32(R.grads(name, torch.float32))                     # on one thread: the generator's summation order
    R.judge(name, low, "fp32 CPU")
    R.judge_rows(name, low, "fp32 CPU")


@pytest.mark.parametrize("fault,touched", [("carry", ("embedding", "w_ih", "w_hh", "b_ih", "b_hh", "grad_cond")),
                                           ("straddle", ("w_ih", "b_ih", "grad_cond"))])
def test_seeded_faults_fail_both_judges(fault, touched):
    """The fp32 run of ``straddle`` with a fault seeded by autograd alone: every tensor the fault touches misses the per-tensor bound
    (by four to five orders of magnitude), the others keep theirs, and the per-row judge fails on ``grad_cond``."""
    import torch
    bad = _as_fp32(R.grads("straddle", torch.float32, fault=fault))
    ratios = _ratios("straddle", bad)
    print(fault, {k: f"{v:.3g}" for k, v in ratios.items()})
    for k in R.TENSORS:
        assert (ratios[k] > 100.0) == (k in touched), (k, ratios[k])
    with pytest.raises(AssertionError):
        R.judge("straddle", bad, fault)
    with pytest.raises(AssertionError, match="grad_cond"):
        R.judge_rows("straddle", bad, fault)


def test_b_ih_and_b_hh_differ_in_the_n_third_only():
    g = R.grads64("b1")
    Hr = R.load("b1")["Hr"]
    assert np.abs(g["b_ih"][:2 * Hr] - g["b_hh"][:2 * Hr]).max() <= 1e-15 and np.abs(g["b_ih"][2 * Hr:] - g["b_hh"][2 * Hr:]).max() > 1e-6


def test_recorded_fit_is_a_trend():
    losses = R.pins()["fit_ref_losses"]
    assert losses.shape == (voc_fit_ref.STEPS,)
    dec, spread = voc_fit_ref.decrease(losses), float(losses[-5:].max() - losses[-5:].min())
    print(f"float64 fit: loss {losses[0]:.6f} -> mean of the last five {losses[-5:].mean():.6f}: decrease {dec:.4f}, spread of the last five {spread:.4f}")
    assert dec > 0 and dec >= 3.0 * spread


# ------------------------------------------------------------------ the struct and the module
def test_ar_tensors_struct_mirrors_the_header():
    """``_lib.VocoderArTensors`` against the header: tests/test_abi_cpu.py.  Here: against the module and the reference."""
    import vectorquantizedcpc_amd as V
    assert tuple(n for n, _ in _lib.VocoderArTensors._fields_) == V.Vocoder.AR_KEYS == R.KEYS
    voc = V.Vocoder(V.ConfVocoder())
    assert [tuple(p.shape) for p in voc._ar_params()] == [tuple(voc.state_dict()["rnnms.ar." + n].shape) for n in R.SD_NAMES]


# ------------------------------------------------------------------ argument checks that need no GPU
def test_training_cuts_are_seeded_and_cover_their_samples():
    import torch
    idx = [torch.arange(n) for n in (30, 2, 10, 1)]
    audio = [torch.arange(320 * n + 7) for n in (30, 2, 10, 1)]
    n_codes = [30, 2, 10, 1]
    keep = [driver.scored_samples(a.numel(), n) for a, n in zip(audio, n_codes)]
    a = driver.training_cuts(idx, audio, n_codes, keep, 160, 2, 13)
    b = driver.training_cuts(idx, audio, n_codes, keep, 160, 2, 13)
    assert all(torch.equal(x, y) for x, y in zip(a[0] + a[1], b[0] + b[1])) and a[2:] == b[2:]
    assert a[2] == [2, 2, 2, 1] and a[3] == [641, 641, 641, 321]
    for i, au in zip(a[0], a[1]):
        assert int(au[0]) == 320 * int(i[0])                          # the samples under the cut's first code
    whole = driver.training_cuts(idx, audio, n_codes, keep, 160, None, 13)
    assert whole[2] == n_codes and whole[3] == keep and n_codes == [30, 2, 10, 1]
    with pytest.raises(ValueError, match="clip_codes"):
        driver.training_cuts(idx, audio, n_codes, keep, 160, 0, 13)


def test_cli_fit_vocoder_parses(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["fit-vocoder", "--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    assert all(o in text for o in ("--steps", "--lr", "--clip-codes", "--out", "--in-dir", "--vocoder-checkpoint"))
    assert "fit-vocoder" in cli.__doc__
    with pytest.raises(SystemExit):
        cli.main(["fit-vocoder", "--dataset", "d", "--in-dir", "w", "--out", "o.pt"])      # neither checkpoints nor --random-init
