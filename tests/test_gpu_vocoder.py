"""-m gpu: the HIP vocoder path through the C ABI against the CPU oracle.

PARITY UNPINNED for this half: the reference's arithmetic lives in the absent third-party
`rnnms`; the oracle is this project's CPU statement of the same spec (self-oracle).
Tolerances (fp32, different summation order than the oracle's serial chains):
  prenet conditioning and teacher-forced logits: 1e-5 absolute (observed maxima on MI355X: 1.8e-7 and 1.6e-7,
  printed by the tests);
  free-running samples: every GPU draw must be the oracle's Gumbel-max choice for the same
  history, or a class whose oracle score is within 2e-5 of the oracle's best (a rounding-level
  tie); identical sample sequences give identical waveforms (MSE 0 <= 1e-5).
"""
import os

import numpy as np
import pytest
import torch

import decode_harness as H
import oracle
import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

pytestmark = pytest.mark.gpu
# this file exercises the launch-per-step kernels; the per-XCD resident decoders (the default up to 64 utterances) are in test_gpu_xcd.py
vocoder = H.Handles(xcd=0)


def options(voc, **opts):
    return H.options(voc, {**H.DEFAULTS, "xcd": 0}, **opts)


def test_glue_and_prenet_condition(golden_dir):
    voc, sd = vocoder()
    z = synth.randint("cond/z", (3, 6), 512)
    spk = synth.randint("cond/spk", (3,), 102)
    got = voc.condition(z.cuda(), spk.cuda()).cpu().numpy()
    for b in range(3):
        want = oracle.vocoder_condition(sd, z[b].numpy(), int(spk[b]))
        print("prenet conditioning, max |GPU - C oracle| = %.3g" % float(np.abs(got[b] - want).max()))
        assert np.abs(got[b] - want).max() <= 1e-5, b


def test_hip_glue_equals_what_the_reference_hands_to_rnnms(golden_dir):
    """tests/golden/vocoder_glue.npz was captured from the reference's own Vocoder.generate / Vocoder.forward
    (network_vocoder.py:69-77, rnnms replaced by a capture stub): the HIP glue kernel must reproduce it bit for bit."""
    voc, _ = vocoder()
    g = np.load(os.path.join(golden_dir, "vocoder_glue.npz"))
    got = voc.glue(torch.from_numpy(g["z"]).cuda(), torch.from_numpy(g["speaker"]).cuda()).cpu().numpy()
    assert got.shape == g["series"].shape and np.array_equal(got, g["series"])


def test_mulaw_table_equals_the_reference_decode(golden_dir):
    """The waveform value of every class is the fp32 rounding of the reference's own mulaw_decode(2x/255 - 1, 256)
    (tests/golden/preprocess.npz, made from preprocess.py:30-35): checked on the samples a decode call emits."""
    voc, _ = vocoder()
    dec = np.load(os.path.join(golden_dir, "preprocess.npz"))["mulaw_decode_256"].astype(np.float32)
    z = synth.randint("mt/z", (4, 8), 512).cuda()
    spk = synth.randint("mt/spk", (4,), 102).cuda()
    with options(voc) as set_option:
        for xcd in (0, 1):
            set_option("xcd", xcd)
            wav, mu = voc.generate(z, spk, seed=21, utt_base=0, return_mulaw=True)
            wav, mu = wav.cpu().numpy(), mu.cpu().numpy()
            assert np.array_equal(wav, dec[mu])
            assert len(np.unique(mu)) > 200                       # most of the 256 classes occur in 10 240 samples


def test_teacher_forced_logits():
    """Vocoder.forward (network_vocoder.py:41-67): logits for given previous samples."""
    voc, sd = vocoder()
    B, Tc, Ts = 2, 2, 400
    z = synth.randint("tf/z", (B, Tc), 512)
    spk = synth.randint("tf/spk", (B,), 102)
    x = synth.randint("tf/x", (B, Ts), 256)
    got = voc(x.cuda(), z.cuda(), spk.cuda()).cpu().numpy()
    assert got.shape == (B, Ts, 256)
    worst = 0.0
    for b in range(B):
        r = oracle.vocoder_generate(sd, z[b].numpy(), int(spk[b]), seed=0, n_steps=Ts, inputs=x[b].numpy(), want_logits=True)
        worst = max(worst, float(np.abs(got[b] - r["logits"]).max()))
    print("teacher-forced logits, max |GPU - C oracle| = %.3g" % worst)
    assert worst <= 1e-5, worst


def _check_free_run(voc, sd, z, spk, n_codes, seed, utt_base, steps):
    wav, mu = voc.generate(z.cuda(), spk.cuda(), n_codes=n_codes, seed=seed, utt_base=utt_base, return_mulaw=True,
                           max_steps=steps)
    wav, mu = wav.cpu().numpy(), mu.cpu().numpy()
    B = z.shape[0]
    stats = oracle.judge_draws(sd, z, spk, mu, seed=seed, utt_ids=range(utt_base, utt_base + B), rows=range(B), steps=steps,
                               n_codes=n_codes, wav=wav)
    for b, (n, exact) in enumerate(stats):
        assert not mu[b, n:].any()
        if exact == n:      # same samples -> compare with the oracle's own free run as well
            nc = z.shape[1] if n_codes is None else n_codes[b]
            free = oracle.vocoder_generate(sd, z[b, :nc].numpy(), int(spk[b]), seed=seed, utterance=utt_base + b, n_steps=n)
            assert np.array_equal(free["samples"], mu[b, :n])
            assert float(np.mean((free["wav"] - wav[b, :n]) ** 2)) <= 1e-5
    return stats


def test_free_running_generate_matches_oracle_protocol():
    voc, sd = vocoder()
    z = synth.randint("gen/z", (3, 3), 512)
    spk = synth.randint("gen/spk", (3,), 102)
    stats = _check_free_run(voc, sd, z, spk, None, seed=13, utt_base=5, steps=700)
    print("free-run (steps, exact agreement with oracle):", stats)
    assert sum(e for _, e in stats) >= 0.999 * sum(n for n, _ in stats)


def test_ragged_batch_and_batch_independence():
    voc, sd = vocoder()
    z = synth.randint("rag/z", (3, 4), 512)
    spk = synth.randint("rag/spk", (3,), 102)
    n_codes = [4, 2, 1]
    _check_free_run(voc, sd, z, spk, n_codes, seed=7, utt_base=0, steps=500)
    wav, mu = voc.generate(z.cuda(), spk.cuda(), n_codes=n_codes, seed=7, utt_base=0, return_mulaw=True, max_steps=500)
    # utterance 1 alone (same utterance id) must give the same bits as inside the batch
    w1, m1 = voc.generate(z[1:2, :2].cuda(), spk[1:2].cuda(), seed=7, utt_base=1, return_mulaw=True, max_steps=500)
    assert torch.equal(m1[0, :500], mu[1, :500]) and torch.equal(w1[0, :500], wav[1, :500])


def test_graph_replay_equals_eager_launches():
    voc, _ = vocoder()
    z = synth.randint("gr/z", (2, 2), 512).cuda()
    spk = synth.randint("gr/spk", (2,), 102).cuda()
    with options(voc, use_graph=1, steps_per_graph=64) as set_option:
        a = voc.generate(z, spk, seed=3, utt_base=0, return_mulaw=True, max_steps=300)
        set_option("use_graph", 0)
        b = voc.generate(z, spk, seed=3, utt_base=0, return_mulaw=True, max_steps=300)
        set_option("use_graph", 1)
        set_option("steps_per_graph", 160)
        c = voc.generate(z, spk, seed=3, utt_base=0, return_mulaw=True, max_steps=300)
        d = voc.generate(z, spk, seed=4, utt_base=0, return_mulaw=True, max_steps=300)
        set_option("steps_per_graph", 32)              # divides the 160-sample hop: several replays per conditioning
        e = voc.generate(z, spk, seed=3, utt_base=0, return_mulaw=True, max_steps=300)     # frame, Gcond row cached per replay
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and torch.equal(a[1], c[1]) and torch.equal(a[1], e[1])
    assert not torch.equal(a[1], d[1])
    assert a[0].shape == (2, 640) and a[0].abs().max() <= 1.0


def test_full_length_utterance_properties():
    """C3 size (1 utterance, 32 000 samples): finite, in range, class histogram not degenerate."""
    voc, _ = vocoder()
    z = synth.randint("c3/z", (1, 100), 512).cuda()
    spk = torch.zeros(1, dtype=torch.long, device="cuda")
    wav, mu = voc.generate(z, spk, seed=13, utt_base=0, return_mulaw=True)
    assert wav.shape == (1, 32000) and torch.isfinite(wav).all() and wav.abs().max() <= 1.0
    assert mu.min() >= 0 and mu.max() <= 255 and mu.unique().numel() > 32
    ms, n = voc.last_timing()
    assert n == 32000 and ms > 0


def test_continuous_batching_equals_static_batches():
    """Decode slots reused by successive utterances (vqcpc_vocoder_set_option "slots") produce,
    for every utterance, the bits of a plain batched call."""
    voc, _ = vocoder()
    z = synth.randint("cb/z", (7, 4), 512)
    spk = synth.randint("cb/spk", (7,), 102)
    n_codes = [4, 1, 3, 2, 4, 1, 2]
    ids = [11, 12, 13, 14, 15, 16, 17]
    ref_w, ref_m = voc.generate(z.cuda(), spk.cuda(), n_codes=n_codes, seed=21, utt_ids=ids, return_mulaw=True)
    for slots in (2, 3):
        with options(voc, slots=slots):
            w, m = voc.generate(z.cuda(), spk.cuda(), n_codes=n_codes, seed=21, utt_ids=ids, return_mulaw=True)
        assert torch.equal(m, ref_m) and torch.equal(w, ref_w), slots
    assert int((ref_m[1, 320:] != 0).sum()) == 0 and int((ref_m[0] != 0).sum()) > 1000


def test_error_surface_like_nn_embedding():
    voc, _ = vocoder()
    z = torch.zeros(1, 2, dtype=torch.long, device="cuda")
    with pytest.raises(IndexError):
        voc.generate(torch.full((1, 2), 512, device="cuda"), torch.zeros(1, dtype=torch.long, device="cuda"))
    with pytest.raises(IndexError):
        voc.generate(z, torch.tensor([102], device="cuda"))
    with pytest.raises(IndexError):
        voc(torch.full((1, 10), 256, device="cuda"), z, torch.zeros(1, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError):
        voc.generate(z, torch.zeros(2, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError):
        voc.generate(z.float(), torch.zeros(1, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError):
        voc(torch.zeros(1, 641, dtype=torch.long, device="cuda"), z, torch.zeros(1, dtype=torch.long, device="cuda"))


def test_tile_groups_and_large_batch_kernel_are_bit_identical():
    """40 utterances = 3 tiles: one group vs two groups on two streams vs the LDS-staged large-batch
    kernel, with continuous batching on top -- all the same bits (tiles are independent MFMA columns)."""
    voc, _ = vocoder()
    B = 40
    z = synth.randint("tg/z", (B, 3), 512).cuda()
    spk = (torch.arange(B) % 102).cuda()
    n_codes = [1 + (i % 3) for i in range(B)]
    ids = list(range(100, 100 + B))
    outs = {}
    for name, opts in (("one_group", {"two_groups": 0, "big_min_tiles": 0}),
                       ("two_groups", {"two_groups": 1, "big_min_tiles": 0}),
                       ("big_kernel", {"two_groups": 0, "big_min_tiles": 2}),
                       ("two_groups_36_slots", {"two_groups": 1, "big_min_tiles": 0, "slots": 36})):
        with options(voc, **opts):
            outs[name] = voc.generate(z, spk, n_codes=n_codes, seed=9, utt_ids=ids, return_mulaw=True)[1]
    ref = outs["one_group"]
    assert int((ref != 0).sum()) > 10000
    for name, m in outs.items():
        assert torch.equal(m, ref), name


def test_large_batch_kernel_13_tiles_one_group_and_two_groups_bit_identical():
    """200 ragged utterances = 13 tiles, the last one partly filled, on the large-batch kernel: ONE group (7 passes of
    two tiles, the last pass with a single tile), the default (two groups of 7 and 6 tiles on two streams), one group
    without the fused fc2 launch and with continuous batching over 150 slots, all against the small kernel
    (oracle-checked above) -- the same bits."""
    voc, _ = vocoder()
    B = 200
    z = synth.randint("mt/z", (B, 3), 512).cuda()
    spk = (torch.arange(B) * 3 % 102).cuda()
    n_codes = [1 + (i % 3) for i in range(B)]
    ids = list(range(5000, 5000 + B))
    outs = {}
    for name, opts in (("small_kernel", {"two_groups": 0, "big_min_tiles": 0}),
                       ("big_one_group", {"two_groups": 0, "big_min_tiles": 5}),
                       ("big_two_groups", {"two_groups": 1, "big_min_tiles": 5}),
                       ("big_one_group_three_launches", {"two_groups": 0, "big_min_tiles": 5, "fuse_fc2": 0}),
                       ("big_one_group_150_slots", {"two_groups": 0, "big_min_tiles": 5, "slots": 150})):
        with options(voc, **opts):
            outs[name] = voc.generate(z, spk, n_codes=n_codes, seed=17, utt_ids=ids, return_mulaw=True)[1]
    ref = outs["small_kernel"]
    assert int((ref != 0).sum()) > 50000
    for name, m in outs.items():
        assert torch.equal(m, ref), name


def test_default_paths_at_many_batch_sizes_equal_single_utterance_calls():
    """Default options at batch sizes that take different code paths -- one tile with dead columns (5), two
    groups (40: a 2-tile and a 1-tile group), the large-batch kernel with a partly filled last tile (100),
    two large-batch groups (200) -- against calls on single utterances with the same sampling-stream ids."""
    voc, _ = vocoder()
    for B in (5, 40, 100, 200):
        z = synth.randint("mb/z%d" % B, (B, 2), 512).cuda()
        spk = (torch.arange(B) * 7 % 102).cuda()
        n_codes = [1 + (i % 2) for i in range(B)]
        ids = list(range(1000, 1000 + B))
        m = voc.generate(z, spk, n_codes=n_codes, seed=21, utt_ids=ids, return_mulaw=True)[1]
        for i in sorted({0, 1, B // 2, B - 2, B - 1}):
            one = voc.generate(z[i:i + 1, : n_codes[i]], spk[i:i + 1], seed=21, utt_ids=[ids[i]], return_mulaw=True)[1]
            L = 320 * n_codes[i]
            assert torch.equal(m[i, :L], one[0, :L]), (B, i)
            assert not m[i, L:].any(), (B, i)


def _check_rows_direct(voc, sd, B, rows, steps, seed, utt0, tag):
    """The decode kernels a batch of B takes, checked DIRECTLY against the oracles (not via single-utterance HIP
    calls): the C oracle draw by draw on `rows` (5 ms per step, so a spread-out subset: first / last column of every
    tile), and the torch-CPU port teacher-forced on ALL rows (its logits are within 2e-5 of the C oracle's, so the
    tie window is 4e-5 there)."""
    from oracle import torch_ref
    z = synth.randint(f"{tag}/z", (B, 2), 512)
    spk = torch.arange(B) * 5 % 102
    wav, mu = voc.generate(z.cuda(), spk.cuda(), seed=seed, utt_base=utt0, return_mulaw=True, max_steps=steps)
    wav, mu = wav.cpu().numpy(), mu.cpu().numpy()
    assert np.isfinite(wav).all() and not mu[:, steps:].any()
    stats = oracle.judge_draws(sd, z, spk, mu, seed=seed, utt_ids=range(utt0, utt0 + B), rows=rows, steps=steps, wav=wav)
    n_exact = sum(e for _, e in stats)
    assert n_exact >= 0.999 * steps * len(rows)
    tv = torch_ref.TorchVocoder(sd)
    x_in = torch.from_numpy(np.concatenate([np.full((B, 1), 128), mu[:, : steps - 1]], axis=1))
    noise = torch_ref.make_noise(B, steps, seed, utt0)
    _, _, lg = tv.generate(z, spk, seed=seed, utt_base=utt0, n_steps=steps, inputs=x_in, want_logits=True, noise=noise)
    sc = (lg + noise).numpy()
    got = np.take_along_axis(sc, mu[:, :steps, None], axis=2)[..., 0]
    assert float((sc.max(axis=2) - got).max()) <= 4e-5, tag
    return n_exact


def test_bench_kernel_32_utterances_direct_oracle():
    """The kernel bench.py's default workload runs -- ar_gru_kernel<14,2,.> with two full tiles, fc1 in 8-row groups --
    at 32 utterances x 480 samples, against the oracles directly."""
    voc, sd = vocoder()
    _check_rows_direct(voc, sd, 32, [0, 15, 16, 31, 7, 24], 480, seed=13, utt0=0, tag="d32")
    assert voc.kernel_times(20)[4] == 4.0              # kernel kind of the call above: the fused fc2 || GRU launch (two tiles)


def test_large_batch_kernel_96_utterances_direct_oracle():
    """ar_gru_big_kernel (6 tiles: LDS-staged state, full 16-row gate tiles) against the oracles directly."""
    voc, sd = vocoder()
    _check_rows_direct(voc, sd, 96, [0, 17, 47, 64, 95], 480, seed=5, utt0=200, tag="d96")
    assert voc.kernel_times(20)[4] == 5.0              # the fused fc2 || large-batch GRU launch


def test_two_tile_groups_48_utterances_direct_oracle():
    """48 utterances = 3 tiles = a 2-tile and a 1-tile group on two streams (fragments requested 6 ahead), against
    the oracles directly; rows from both groups."""
    voc, sd = vocoder()
    _check_rows_direct(voc, sd, 48, [0, 31, 32, 47, 20], 480, seed=99, utt0=1000, tag="d48")


def test_configs3_shard_full_size_properties():
    """BASELINE configs[3]'s per-GPU shard at full size (32 utterances x 32 000 samples, the bench workload):
    finite, in range, non-degenerate, and three rows equal to single-utterance calls with the same stream ids."""
    voc, _ = vocoder()
    z = synth.randint("c4/z", (32, 100), 512).cuda()
    spk = (torch.arange(32) % 102).cuda()
    wav, mu = voc.generate(z, spk, seed=13, utt_base=0, return_mulaw=True)
    assert wav.shape == (32, 32000) and torch.isfinite(wav).all() and float(wav.abs().max()) <= 1.0
    assert int(mu.min()) >= 0 and int(mu.max()) <= 255
    assert all(mu[b].unique().numel() > 32 for b in range(32))
    for b in (0, 17, 31):
        one = voc.generate(z[b:b + 1], spk[b:b + 1], seed=13, utt_base=b, return_mulaw=True)[1]
        assert torch.equal(one[0], mu[b]), b


def test_teacher_forced_scan_chunks_and_training_shape():
    """Vocoder.forward as a fused scan: GRU steps only, fc1 / fc2 as chunked GEMMs.  Chunk sizes that
    split Ts differently (one replay per chunk: 160 steps, last chunk partial) give the same bits; a batch that takes
    the large-batch GRU kernel agrees with the two-tile kernel's rows; all within 1e-5 of the oracle."""
    voc, sd = vocoder()
    B, Tc, Ts = 3, 3, 700
    z = synth.randint("tf2/z", (B, Tc), 512)
    spk = synth.randint("tf2/spk", (B,), 102)
    x = synth.randint("tf2/x", (B, Ts), 256)
    a = voc(x.cuda(), z.cuda(), spk.cuda())
    with options(voc, tf_chunk_replays=1) as set_option:
        b = voc(x.cuda(), z.cuda(), spk.cuda())
        set_option("use_graph", 0)
        c = voc(x.cuda(), z.cuda(), spk.cuda())
    assert torch.equal(a, b) and torch.equal(a, c)
    r = oracle.vocoder_generate(sd, z[1].numpy(), int(spk[1]), seed=0, n_steps=Ts, inputs=x[1].numpy(), want_logits=True)
    worst = float(np.abs(a[1].cpu().numpy() - r["logits"]).max())
    print("teacher-forced scan (3, 700), max |GPU - C oracle| = %.3g" % worst)
    assert worst <= 1e-5
    # 100 utterances (7 tiles -> large-batch kernel), short: rows 0..2 are the same utterances as above
    B2 = 100
    z2 = torch.cat([z, synth.randint("tf2/z2", (B2 - B, Tc), 512)])
    spk2 = torch.cat([spk, synth.randint("tf2/spk2", (B2 - B,), 102)])
    x2 = torch.cat([x[:, :200], synth.randint("tf2/x2", (B2 - B, 200), 256)])
    d = voc(x2.cuda(), z2.cuda(), spk2.cuda())
    assert d.shape == (B2, 200, 256) and torch.equal(d[:B], a[:, :200])


def test_single_utterance_default_path_equals_the_launch_path():
    """BASELINE configs[2]: one utterance runs on the per-XCD resident decoders by default (this file's fixture turns them off:
    here they are on).  It must produce the bits of the launch-per-step kernels (same fma chains), so an utterance alone still
    equals itself inside a batch; and it is checked against the oracle directly, draw by draw."""
    voc, sd = vocoder()
    z = synth.randint("ps/z", (1, 4), 512)
    spk = torch.tensor([7])
    with options(voc) as set_option:
        w0, m0 = voc.generate(z.cuda(), spk.cuda(), seed=13, utt_base=3, return_mulaw=True)
        assert voc.last_path() == 0
        set_option("xcd", -1)
        w1, m1 = voc.generate(z.cuda(), spk.cuda(), seed=13, utt_base=3, return_mulaw=True)
        assert voc.last_path() == 2
        w2, m2 = voc.generate(z.cuda(), spk.cuda(), seed=13, utt_base=3, return_mulaw=True, max_steps=333)
        assert m0.shape == (1, 1280) and int((m0 != 0).sum()) > 1000
        assert torch.equal(m0, m1) and torch.equal(w0, w1)
        assert torch.equal(m2[0, :333], m0[0, :333]) and not m2[0, 333:].any() and not w2[0, 333:].any()
        stats = _check_free_run(voc, sd, z, spk, None, seed=13, utt_base=3, steps=600)
        assert stats[0][1] >= 0.999 * stats[0][0]
        with pytest.raises(RuntimeError):
            voc.kernel_times(10)               # no launch-per-step state after a resident call


def test_fused_fc2_gru_launch_same_bits_and_direct_oracle():
    """Two launches per sample (the launch path's default: fc2 + draw of sample t-1 ride in front of the GRU step of sample t
    and hand the candidates over in-kernel) and round 1's three launches give the same bits at one tile, two tiles, three
    tiles, on the large-batch kernel and with continuous batching (slots reused by successive utterances); the fused path is
    checked against the oracles directly in
    test_bench_kernel_32_utterances_direct_oracle / test_large_batch_kernel_96_utterances_direct_oracle."""
    voc, _ = vocoder()
    for B, slots in ((5, 0), (32, 0), (48, 0), (40, 20), (100, 0)):
        z = synth.randint("fz/z%d" % B, (B, 3), 512).cuda()
        spk = (torch.arange(B) * 3 % 102).cuda()
        n_codes = [1 + (i % 3) for i in range(B)]
        ids = list(range(500, 500 + B))
        outs = []
        for f2 in (1, 0):
            with options(voc, fuse_fc2=f2, slots=slots):
                outs.append(voc.generate(z, spk, n_codes=n_codes, seed=77, utt_ids=ids, return_mulaw=True))
        for o in outs[1:]:
            assert torch.equal(outs[0][1], o[1]) and torch.equal(outs[0][0], o[0]), (B, slots)
        assert int((outs[0][1] != 0).sum()) > 100 * B
    z = synth.randint("fz/one", (32, 2), 512).cuda()
    voc.generate(z, (torch.arange(32) % 102).cuda(), seed=1, utt_base=0, max_steps=64)
    assert voc.kernel_times(20)[4] == 4.0                   # the default path at 32 utterances is the fused fc2 || GRU launch


def test_other_sizes_9_bit_mulaw_wider_fc_smaller_rnn():
    """config.py:15 / :69 / :76-77 make bits_mu_law, size_h_rnn and size_h_fc configurable: 9-bit mu-law (512 classes = 32
    candidate row groups), size_h_fc 512 (two blocks of four super-steps per fc2 wave) and size_h_rnn 512 on the
    launch-per-step kernels (the resident decoders exist for the reference's sizes only) -- teacher-forced logits and
    free-running draws against the C oracle, fused and three-launch schedules the same bits, large-batch kernel rows equal."""
    sd = synth.vocoder_state_dict(size_h_rnn=512, size_h_fc=512, bits_mu_law=9)
    conf = V.ConfVocoder()
    conf.rnnms.bits_mu_law = 9
    conf.rnnms.wave_ar.size_h_rnn = 512
    conf.rnnms.wave_ar.size_h_fc = 512
    voc, _ = vocoder(conf=conf, sd=sd)
    B, Tc, Ts = 3, 2, 300
    z = synth.randint("sz/z", (B, Tc), 512)
    spk = synth.randint("sz/spk", (B,), 102)
    x = synth.randint("sz/x", (B, Ts), 512)
    got = voc(x.cuda(), z.cuda(), spk.cuda()).cpu().numpy()
    assert got.shape == (B, Ts, 512)
    worst = 0.0
    for b in range(B):
        r = oracle.vocoder_generate(sd, z[b].numpy(), int(spk[b]), seed=0, n_steps=Ts, inputs=x[b].numpy(), want_logits=True, bits=9)
        worst = max(worst, float(np.abs(got[b] - r["logits"]).max()))
    print("9-bit / 512 / 512 teacher-forced logits, max |GPU - C oracle| = %.3g" % worst)
    assert worst <= 1e-5
    outs = []
    with H.options(voc) as set_option:
        for f2 in (1, 0):
            set_option("fuse_fc2", f2)
            outs.append([t.numpy() for t in H.decode(voc, z.cuda(), spk.cuda(), path=0, seed=13, utt_base=40, max_steps=Ts)])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][0], outs[1][0])
    wav, mu = outs[0]
    assert mu.max() > 255                                     # classes beyond 8 bits do occur
    oracle.judge_draws(sd, z, spk, mu, seed=13, utt_ids=range(40, 40 + B), rows=range(B), steps=Ts, wav=wav, bits=9)
    # 100 utterances: the large-batch kernel; rows 0..2 are the utterances above
    z2 = torch.cat([z, synth.randint("sz/z2", (97, Tc), 512)])
    spk2 = torch.cat([spk, synth.randint("sz/s2", (97,), 102)])
    w2, m2 = voc.generate(z2.cuda(), spk2.cuda(), seed=13, utt_base=40, return_mulaw=True, max_steps=Ts)
    voc.check()
    assert np.array_equal(m2[:B].cpu().numpy(), mu) and np.array_equal(w2[:B].cpu().numpy(), wav)
    with pytest.raises(RuntimeError):                         # a size outside the built list is an explicit error
        bad = V.ConfVocoder()
        bad.rnnms.wave_ar.size_h_rnn = 640
        vb = V.Vocoder(bad)
        vb.load_state_dict(synth.vocoder_state_dict(size_h_rnn=640))
        vb.to("cuda").eval().generate(z.cuda(), spk.cuda(), seed=1, utt_base=0, max_steps=8)
