"""-m gpu: codebook adaptation -- the EMA update of ``VQEmbeddingEMA.forward`` in training mode (``model.py:136-145``) in HIP
(csrc/codebook.hip, ``vqcpc_encoder_vq_adapt``), DESIGN.md 2.6.  Everything goes through the public classes; raw ctypes only where
the C ABI itself is the subject (bad arguments, guard words behind the outputs).

a. Bits: ``ema_count``, ``ema_weight`` and ``embedding`` equal, by value, the numpy restatement ``ema_ref.step_f32`` fed with the GPU's
   own indices.  N in {1, 63, 64, 65, 129, 4 113} x M in {64, 512, 1024} x usage uniform / one code / skewed x zero / warm start,
   a chain of 3 updates compared after each.
b. Every reference fixture (tests/golden/ema_*.npz: the reference's own module in ``.train()``): same indices, and each buffer within
   max(4 x the reference's recorded error against float64, 2 fp32 ulp) of the recorded values -- the bound of tests/test_ema_cpu.py,
   measured from the reference.
c. The three outputs of the training ``forward`` are bit-equal to the eval ``forward`` from the same state.
d. After an update the handle equals a fresh ``Encoder`` loaded from ``state_dict()``: ``encode`` and ``codebook.encode`` bit-equal,
   and a second update gives the same buffers on both.
e. Two runs give the same bits; NaN rows behind the valid rows reach no buffer; guard words behind every output stay.
f. ``Encoder.adapt_codebook`` with ragged ``n_frames`` equals the update on the hand-gathered rows; over 5 passes on one batch the
   loss does not rise and the number of codes in use does not fall.
g. Bad arguments give ``VQCPC_ERR_INVALID``; a gradient request raises ``NotImplementedError``; ``Encoder.forward`` in train mode
   still raises.

Measured on an MI355X (the whole file: 33 tests in under 4 s).  (a), (c), (d), (e), (f) are equalities and hold exactly.  (b), the
GPU's buffers against the reference's recorded ones, errors scaled as ``ema_ref.scaled_errors`` (count, weight, embedding):

  ======================  ============================  ============================
  fixture                 GPU vs the reference          bound = max(4 x reference vs f64, 2 ulp)
  ======================  ============================  ============================
  m64_n160_warm           0        0        0           3.87e-7  3.67e-7  7.15e-7
  m64_n4096_onecode       9.36e-8  7.55e-8  1.62e-7     2.69e-7  3.02e-7  7.81e-7
  m512_n4096_every_zero   0        8.20e-8  8.40e-8     2.38e-7  3.23e-7  4.85e-7
  m512_n4096_warm         0        5.41e-8  7.98e-8     5.20e-7  4.18e-7  1.15e-6
  m1024_n4113_skewed      0        9.24e-8  8.51e-8     6.06e-7  4.22e-7  1.08e-6
  ======================  ============================  ============================

(f) five passes on one batch of 512 rows over 64 codes from a trained state: loss 0.0072505, 0.0072393, 0.0072280, 0.0072167,
0.0072054; codes in use 60 at every pass.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import ema_ref
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import _lib, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BUFFERS = ("ema_count", "ema_weight", "embedding")


@functools.lru_cache(maxsize=None)
def base_state(n_emb):
    return synth.encoder_state_dict(n_embeddings=n_emb)


def encoder_for(case, n_emb):
    """A fresh ``Encoder`` on the GPU whose codebook buffers are the case's."""
    enc = V.Encoder(V.ConfEncoder(80, 512, n_emb, 64, 256))
    sd = dict(base_state(n_emb))
    sd.update({"codebook." + k: torch.from_numpy(case[k]) for k in BUFFERS})
    enc.load_state_dict(sd)
    return enc.cuda().eval()


def buffers(enc):
    return tuple(getattr(enc.codebook, k).cpu().numpy() for k in BUFFERS)


def train_step(enc, x):
    """One training-mode ``forward`` of the codebook; the module is left in eval mode."""
    enc.codebook.train()
    try:
        return enc.codebook(x)
    finally:
        enc.codebook.eval()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("n_emb", [64, 512, 1024])
@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129, 4113])
def test_bits_against_the_restatement(n_rows, n_emb):
    for usage in ("uniform", "one", "skewed"):
        for start in ("zero", "warm"):
            case = ema_ref.make_case(f"gpu_a_{n_rows}_{n_emb}_{usage}", n_emb, n_rows, usage, start)
            enc = encoder_for(case, n_emb)
            x = torch.from_numpy(case["x"]).cuda()[None]
            state = (case["ema_count"], case["ema_weight"], case["embedding"])
            for step in range(3):
                idx = enc.codebook.encode(x)[1].reshape(-1).cpu().numpy()       # the GPU's own indices, from the state it updates
                if step == 0:
                    assert np.array_equal(idx, case["code"])
                train_step(enc, x)
                want = ema_ref.step_f32(case["x"], idx, state[0], state[1])
                got = buffers(enc)
                for name, g, w in zip(BUFFERS, got, want):
                    assert np.array_equal(g, w), (usage, start, step, name, int((g != w).sum()),
                                                  float(np.abs(g.astype(np.float64) - w).max()))
                state = got


# ---------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("name", list(ema_ref.FIXTURE_CASES))
def test_within_the_bound_of_the_reference_fixture(name):
    n_emb, n_rows, usage, start = ema_ref.FIXTURE_CASES[name]
    gold = np.load(os.path.join(GOLDEN, f"ema_{name}.npz"))
    case = ema_ref.make_case(name, n_emb, n_rows, usage, start)
    enc = encoder_for(case, n_emb)
    enc.codebook.decay, enc.codebook.epsilon = float(gold["decay"]), float(gold["epsilon"])
    x = torch.from_numpy(case["x"]).cuda()[None]
    idx = enc.codebook.encode(x)[1].reshape(-1).cpu().numpy()
    assert np.array_equal(idx, gold["indices"].astype(np.int64))
    _, loss, ppl = train_step(enc, x)
    every = int(gold["every"])
    got = buffers(enc)
    err = ema_ref.scaled_errors((got[0], got[1][::every], got[2][::every]),
                                tuple(gold[k].astype(np.float64) for k in BUFFERS))
    bounds = [ema_ref.bound(e) for e in gold["ref_err"]]
    print(f"{name}: GPU vs reference {err[0]:.3g} {err[1]:.3g} {err[2]:.3g} | bounds {bounds[0]:.3g} {bounds[1]:.3g} {bounds[2]:.3g}")
    for what, e, b in zip(BUFFERS, err, bounds):
        assert e <= b, (name, what, e, b)
    # loss / perplexity: the eval-branch values (tests/test_gpu_encoder_f64.py bounds them); here only that they are the old codebook's
    assert abs(float(loss) - float(gold["loss"])) <= 4e-6 * abs(float(gold["loss"]))
    assert abs(float(ppl) - float(gold["perplexity"])) <= 4e-6 * abs(float(gold["perplexity"]))


# ---------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("n_rows,n_emb", [(65, 64), (4113, 512)])
def test_training_forward_outputs_equal_eval_forward(n_rows, n_emb):
    case = ema_ref.make_case(f"gpu_c_{n_rows}", n_emb, n_rows, "skewed", "warm")
    enc = encoder_for(case, n_emb)
    x = torch.from_numpy(case["x"]).cuda().view(1, n_rows, 64)
    z_e, loss_e, ppl_e = enc.codebook(x)
    before = buffers(enc)
    assert all(np.array_equal(a, case[k]) for a, k in zip(before, BUFFERS))      # eval mode moves nothing
    z_t, loss_t, ppl_t = train_step(enc, x)
    assert z_t.shape == x.shape and torch.equal(bits(z_t), bits(z_e))
    assert torch.equal(bits(loss_t), bits(loss_e)) and torch.equal(bits(ppl_t), bits(ppl_e))
    assert not np.array_equal(buffers(enc)[2], before[2])


# ---------------------------------------------------------------------------------------------- d
def test_handle_after_an_update_equals_a_fresh_one():
    n_emb, n_rows = 512, 600
    case = ema_ref.make_case("gpu_d", n_emb, n_rows, "uniform", "warm")
    enc = encoder_for(case, n_emb)
    x = torch.from_numpy(case["x"]).cuda()[None]
    mel = synth.mel("ema_d", 3, 70).cuda()
    enc.encode(mel)                                            # the handle exists and has served before the update
    ptrs = [getattr(enc.codebook, k).data_ptr() for k in BUFFERS]
    handle = enc._native().value
    train_step(enc, x)
    assert [getattr(enc.codebook, k).data_ptr() for k in BUFFERS] == ptrs          # in place, not rebound
    assert enc._native().value == handle                                            # and the handle was not rebuilt
    fresh = V.Encoder(V.ConfEncoder(80, 512, n_emb, 64, 256))
    fresh.load_state_dict({k: v.cpu() for k, v in enc.state_dict().items()})
    fresh = fresh.cuda().eval()
    probe = (torch.from_numpy(case["x"]).cuda() * 1.01)[None]
    for a, b in zip(enc.encode(mel), fresh.encode(mel)):
        assert torch.equal(a, b)
    for a, b in zip(enc.codebook.encode(probe), fresh.codebook.encode(probe)):
        assert torch.equal(a, b)
    out_a, out_b = train_step(enc, probe), train_step(fresh, probe)                # the second update starts from the first's result
    for a, b in zip(out_a, out_b):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(buffers(enc), buffers(fresh)):
        assert np.array_equal(a, b)
    for a, b in zip(enc.encode(mel), fresh.encode(mel)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- e
def test_two_runs_same_bits_and_poison_behind_the_rows():
    n_emb, n_rows = 512, 4113
    case = ema_ref.make_case("gpu_e", n_emb, n_rows, "skewed", "zero")
    results = []
    for run in range(2):
        enc = encoder_for(case, n_emb)
        big = torch.full((n_rows + 200, 64), float("nan"), device="cuda")
        big[:n_rows] = torch.from_numpy(case["x"]).cuda()
        out = train_step(enc, big[:n_rows][None])
        results.append([bits(t) for t in out] + [torch.from_numpy(b).view(torch.int32) for b in buffers(enc)])
        assert all(np.isfinite(b).all() for b in buffers(enc))
        assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]) and torch.isfinite(out[2])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_nothing_is_written_behind_the_outputs():
    n_emb, n_rows, pad = 64, 129, 64
    case = ema_ref.make_case("gpu_e_guard", n_emb, n_rows, "uniform", "warm")
    enc = encoder_for(case, n_emb)
    guard = 12345.0

    def padded(a):
        t = torch.full((a.size + pad,), guard, device="cuda")
        t[:a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        return t

    emb, cnt, wgt = padded(case["embedding"]), padded(case["ema_count"]), padded(case["ema_weight"])
    x = torch.from_numpy(case["x"]).cuda()
    z_st = torch.full((n_rows * 64 + pad,), guard, device="cuda")
    idx = torch.full((n_rows + pad,), -7, dtype=torch.int64, device="cuda")
    stats = torch.full((2 + pad,), guard, device="cuda")
    rc = _lib.load().vqcpc_encoder_vq_adapt(enc._native(), x.data_ptr(), n_rows, 0.999, 1e-5, emb.data_ptr(), cnt.data_ptr(),
                                            wgt.data_ptr(), z_st.data_ptr(), idx.data_ptr(), stats[0:].data_ptr(),
                                            stats[1:].data_ptr(), _lib.current_stream())
    assert rc == 0, _lib.load().vqcpc_last_error()
    torch.cuda.synchronize()
    for t, n in ((emb, n_emb * 64), (cnt, n_emb), (wgt, n_emb * 64), (z_st, n_rows * 64), (stats, 2)):
        assert bool((t[n:] == guard).all()) and not bool((t[:n] == guard).any())
    assert bool((idx[n_rows:] == -7).all()) and np.array_equal(idx[:n_rows].cpu().numpy(), case["code"])
    want = ema_ref.step_f32(case["x"], case["code"], case["ema_count"], case["ema_weight"])
    for t, w in zip((cnt, wgt, emb), want):
        assert np.array_equal(t[:w.size].cpu().numpy(), w.reshape(-1))
    # the module's own buffers were not this call's: untouched
    assert all(np.array_equal(a, case[k]) for a, k in zip(buffers(enc), BUFFERS))


# ---------------------------------------------------------------------------------------------- f
def warm_encoder(n_emb, name, count=0.01, dead=()):
    """An encoder whose codebook sits at the scale of its own ``z_pre`` rows (codes = rows of a probe batch), every ``ema_count`` =
    ``count``.  The default is far below a trained module's, so that one update moves the codes by a large fraction of the way to
    their rows' means: the equality tests want every buffer to move visibly.  ``dead``: codes moved 1000 away in every
    dimension, where no row can reach them -- like a trained checkpoint's dead codes they keep a count like everyone else's."""
    enc = V.Encoder(V.ConfEncoder(80, 512, n_emb, 64, 256))
    enc.load_state_dict(base_state(n_emb))
    enc = enc.cuda().eval()
    rows = enc.stage(synth.mel(name + "/probe", 4, 2 * n_emb).cuda(), 10).reshape(-1, 64)
    pick = rows[:: rows.size(0) // n_emb][:n_emb].contiguous()
    pick[list(dead)] += 1000.0
    sd = {k: v.clone() for k, v in enc.state_dict().items()}
    sd["codebook.embedding"] = pick
    sd["codebook.ema_count"] = torch.full((n_emb,), float(count), device="cuda")
    sd["codebook.ema_weight"] = pick * float(count)
    enc.load_state_dict(sd)
    return enc


def test_adapt_codebook_ragged_equals_the_gathered_rows():
    n_emb = 64
    a, b = warm_encoder(n_emb, "ema_f"), warm_encoder(n_emb, "ema_f")
    mels = synth.mel("ema_f/batch", 3, 90).cuda()                  # 45 output frames each
    n_frames = [45, 17, 0]
    mels[1, :, 2 * 17 + 2:] = float("nan")                          # padding behind the valid frames (+ the conv's reach)
    mels[2] = float("nan")
    for mode in ("eval", "train"):
        getattr(a, mode)()
        loss_a, ppl_a = a.adapt_codebook(mels, n_frames)
        z_pre = b.stage(mels, 10)
        rows = torch.cat([z_pre[i, :n] for i, n in enumerate(n_frames)])
        _, loss_b, ppl_b = train_step(b, rows[None])
        assert torch.equal(bits(loss_a), bits(loss_b)) and torch.equal(bits(ppl_a), bits(ppl_b))
        for u, v in zip(buffers(a), buffers(b)):
            assert np.isfinite(u).all() and np.array_equal(u, v)
    a.eval()
    with pytest.raises(RuntimeError, match="n_frames"):
        a.adapt_codebook(mels, [45, 46, 0])
    with pytest.raises(RuntimeError, match="n_frames"):
        a.adapt_codebook(mels, [45, 17])


def test_repeated_passes_do_not_raise_the_loss_or_lose_codes():
    """The state is a trained checkpoint's: the fixed point of ``count = decay * count + (1 - decay) * hist`` under batches of N
    rows is ``hist`` itself, N / M per code on average -- here 512 rows over 64 codes = 8.  (With counts a thousand times smaller,
    as the equality tests use, a pass is a near-whole k-means step and a code may lose all its rows to a neighbour: 60 -> 54 codes
    was measured there on the GPU, whose buffers are the restatement's bit for bit.  That is the update rule, not this property's
    regime.)"""
    enc = warm_encoder(64, "ema_f5", count=512 / 64)
    mels = synth.mel("ema_f5/batch", 8, 128).cuda()
    losses, in_use = [], []
    for _ in range(5):
        in_use.append(int(torch.unique(enc.encode_indices(mels)).numel()))
        losses.append(float(enc.adapt_codebook(mels)[0]))
    print("loss per pass", ["%.6g" % v for v in losses], "| codes in use", in_use)
    assert all(b <= a for a, b in zip(losses, losses[1:])), losses
    assert all(b >= a for a, b in zip(in_use, in_use[1:])), in_use
    assert losses[-1] < losses[0]


# ---------------------------------------------------------------------------------------------- g
def test_error_surface():
    case = ema_ref.make_case("gpu_g", 64, 65, "uniform", "warm")
    enc = encoder_for(case, 64)
    lib, h = _lib.load(), enc._native()
    x = torch.from_numpy(case["x"]).cuda()
    cb = enc.codebook
    stats = torch.zeros(2, device="cuda")

    def call(x_ptr=x.data_ptr(), n=65, decay=0.999, eps=1e-5, emb=cb.embedding.data_ptr(), cnt=cb.ema_count.data_ptr(),
             wgt=cb.ema_weight.data_ptr(), loss=stats[0:].data_ptr(), ppl=stats[1:].data_ptr(), handle=h):
        return lib.vqcpc_encoder_vq_adapt(handle, x_ptr, n, decay, eps, emb, cnt, wgt, None, None, loss, ppl, _lib.current_stream())

    bad = [dict(handle=None), dict(x_ptr=None), dict(emb=None), dict(cnt=None), dict(wgt=None), dict(loss=None), dict(ppl=None),
           dict(n=0), dict(n=-3), dict(n=(1 << 24) + 1), dict(decay=0.0), dict(decay=1.0), dict(decay=-0.5), dict(decay=1.5),
           dict(decay=float("nan")), dict(eps=0.0), dict(eps=-1e-5), dict(eps=float("nan"))]
    for kw in bad:
        assert call(**kw) == -1, kw                                   # VQCPC_ERR_INVALID
        assert b"vqcpc_encoder_vq_adapt" in lib.vqcpc_last_error()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, case[k]) for a, k in zip(buffers(enc), BUFFERS))       # nothing was enqueued
    assert call() == 0

    enc.train()
    xg = x[None].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="straight-through"):
        enc.codebook(xg)
    with torch.no_grad():
        enc.codebook(xg)                                              # no gradient asked for: runs
    enc.codebook(xg.detach())
    with pytest.raises(NotImplementedError):
        enc(synth.mel("ema_g", 1, 32).cuda())                        # Encoder.forward in train mode: still out of scope


# ---------------------------------------------------------------------------------------------- driver and command line
def corpus(tmp_path=None):
    """Seven mels of 40 .. 90 frames (two length buckets at max_pad_frac 0.25), optionally written as a dataset directory."""
    import json
    lens = [40, 44, 47, 76, 80, 86, 90]
    mels = {f"s{i % 2}_u{i}": synth.mel(f"ema_drv/{i}", 1, T)[0] for i, T in enumerate(lens)}
    if tmp_path is None:
        return mels
    root = tmp_path / "datasets" / "d"
    root.mkdir(parents=True)
    for name, mel in mels.items():
        np.save(root / (name + ".mel.npy"), mel.numpy())
    (root / "test.json").write_text(json.dumps([[0, 0, 0, f"d/{name}"] for name in mels]))
    return root, mels


def test_driver_adapt_codebook_is_the_bucketed_loop():
    """... and ``codes_in_use`` is the number of distinct codes the epoch's rows were assigned to: the odd codes are dead (no
    row can reach them) although their ``ema_count`` is that of the live ones, and are not counted."""
    from vectorquantizedcpc_amd import driver
    mels = list(corpus().values())
    dead = list(range(1, 64, 2))
    a, b = warm_encoder(64, "ema_drv", dead=dead), warm_encoder(64, "ema_drv", dead=dead)
    r = driver.adapt_codebook(a, mels, epochs=2, max_batch=4)
    lengths = [m.shape[-1] for m in mels]
    buckets = driver.make_buckets(lengths, [driver.batch1_conv_mode(80, t) for t in lengths], 4, 0.25)
    assert len(buckets) >= 2 and r["rows"] == [sum(driver.out_frames(lengths[i]) for i in ids) for ids in buckets]
    want, used = [], []
    for _ in range(2):
        seen = set()
        for ids in buckets:                                       # the same update from per-utterance calls' rows, no padding at all
            rows = torch.cat([b.stage(mels[i][None].cuda(), 10, driver.batch1_conv_mode(80, lengths[i]))[0] for i in ids])
            seen |= set(b.codebook.encode(rows[None])[1].reshape(-1).tolist())       # from the codebook this batch is about to move
            want.append(float(train_step(b, rows[None])[1]))
        used.append(len(seen))
        assert not seen & set(dead)
    assert [v for e in r["loss"] for v in e] == want
    for u, v in zip(buffers(a), buffers(b)):
        assert np.array_equal(u, v)
    assert r["codes_in_use"] == used and all(1 <= u <= 32 for u in used)
    assert int((a.codebook.ema_count[dead] > 100 * a.codebook.epsilon).sum()) == len(dead)      # what a count threshold would say
    again = driver.adapt_codebook(warm_encoder(64, "ema_drv", dead=dead), mels, epochs=2, max_batch=4)
    assert again == r                                             # a run is reproducible


def test_cli_adapt_codebook_writes_a_checkpoint_the_other_commands_read(tmp_path, capsys):
    from vectorquantizedcpc_amd import cli, io
    root, mels = corpus(tmp_path)
    src, out = tmp_path / "in.pt", tmp_path / "out.pt"
    enc = warm_encoder(512, "ema_cli", dead=range(0, 512, 4))
    torch.save({"encoder": {k: v.cpu() for k, v in enc.state_dict().items()}, "cpc": {"marker": torch.ones(1)}}, src)
    assert cli.main(["adapt-codebook", "--dataset", str(root), "--cpc-checkpoint", str(src), "--out-checkpoint", str(out),
                     "--epochs", "2"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3 and lines[0].startswith("epoch 1: vq loss:") and "codes in use:" in lines[1]
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert list(ck["encoder"].keys()) == list(synth.encoder_state_dict().keys()) and torch.equal(ck["cpc"]["marker"], torch.ones(1))
    from vectorquantizedcpc_amd import driver
    r = driver.adapt_codebook(enc, list(mels.values()), epochs=2)
    for line, used in zip(lines, r["codes_in_use"]):              # 231 rows and 128 dead codes: far fewer than 512, and said so
        assert line.endswith(f"codes in use:{used}/512") and 1 <= used <= min(231, 384)
    for k, v in enc.state_dict().items():
        assert torch.equal(ck["encoder"][k], v.cpu()), k
    assert not torch.equal(ck["encoder"]["codebook.embedding"], io.load_encoder_checkpoint(src)["codebook.embedding"])
    z_dir = tmp_path / "z"
    assert cli.main(["encode", "--dataset", str(root), "--out-dir", str(z_dir), "--cpc-checkpoint", str(out)]) == 0
    name = next(iter(mels))
    z = enc.encode(mels[name][None].cuda())[0][0]
    io.save_frames_text(tmp_path / "probe", z)
    assert np.array_equal(io.load_frames_text(z_dir / name), io.load_frames_text(tmp_path / "probe"))
