"""-m gpu: ABX scoring (csrc/abx.hip, vectorquantizedcpc_amd/abx.py) against the float64 reference of tests/abx_ref.py.

Cost bound: |cost32 - cost64| <= (Ta + Tb - 1) * delta for EVERY pair, delta = abx_ref.K_DELTA x the largest
frame-distance error of the fp32 numpy restatement against float64 on the same inputs (min-plus is non-expansive, so ties do
not matter for the cost).  Path lengths are compared on every pair whose float64 run has no predecessor gap below
2 (Ta + Tb) delta on its optimal path."""
import ctypes as C

import numpy as np
import pytest
import torch

import abx_ref
from vectorquantizedcpc_amd import _lib, abx, cli, driver, io, synth

pytestmark = pytest.mark.gpu

PATH_CAP = 0.02                   # share of pairs that may be left out of the path-length comparison
TRIPLE_CAP = 0.01                 # share of triples that may be left out of the end-to-end count comparison


def blocks_of(pairs):
    """(a_ids, x_ids) lists -> one-segment blocks (the counts are not what these tests look at)."""
    return [abx.Block(a, [0, len(a)], x, [0] * len(x)) for a, x in pairs]


def run(frames, tokens, blocks):
    r = abx.pair_distances(torch.from_numpy(np.ascontiguousarray(frames)).cuda(), tokens, blocks)
    return (r.cost.cpu().numpy(), r.path_len.cpu().numpy(), r.dist.cpu().numpy(), r.twice_wins.cpu().numpy(), r)


def check_costs(got_cost, c64, steps, delta, what):
    err = np.abs(got_cost.astype(np.float64) - c64)
    bound = steps * delta
    print(f"{what}: max |cost32 - cost64| / bound = {(err / bound).max():.4f} (max error {err.max():.3g}, delta {delta:.3g})")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} pairs outside the bound, worst {(err / bound).max():.3f}"


@pytest.fixture(scope="module")
def cost_runs():
    out = {}
    for D in abx_ref.COST_DS:
        f, tokens = abx_ref.cost_case(D)
        out[D] = run(f, tokens, blocks_of(abx_ref.COST_BLOCKS))[:3]
    return out


@pytest.mark.parametrize("D", abx_ref.COST_DS)
def test_costs_against_float64(cost_runs, D):
    """Random frames with exact duplicates, one all-zero frame and one antiparallel pair; token lengths 1x1, 1x64, 64x1, 64x64,
    3x17, 33x31 and a dense block of short ones; every pair inside the bound, nothing left out."""
    ref = abx_ref.cost_reference(D)
    c64, l64, _, _, steps = ref["f64"]
    cost, plen, dist = cost_runs[D]
    assert cost.shape == c64.shape and np.isfinite(cost).all()
    check_costs(cost, c64, steps, abx_ref.K_DELTA * ref["frame_err"], f"D = {D}")
    # block 6 = tokens (1, 2) x (1, 2): a token against itself costs exactly 0 along the diagonal
    base = sum(len(a) * len(x) for a, x in abx_ref.COST_BLOCKS[:6])
    assert cost[base] == 0.0 and plen[base] == 64 and dist[base] == 0.0
    assert cost[base + 3] == 0.0 and plen[base + 3] == 3
    assert cost[base + 1] > 0.0 and cost[base + 2] > 0.0


def test_costs_against_float64_full_rank_frames():
    """The same lengths on independent random components at D = 512: the long sums with uncorrelated terms.  Only the cost bound
    is asked here (every distance is 0.5 +- 0.01, so the long pairs have near-ties on their paths)."""
    ref = abx_ref.cost_reference(512, rank=0)
    f, tokens = abx_ref.cost_case(512, rank=0)
    cost, plen, dist = run(f, tokens, blocks_of(abx_ref.COST_BLOCKS))[:3]
    c64, _, _, _, steps = ref["f64"]
    check_costs(cost, c64, steps, abx_ref.K_DELTA * ref["frame_err"], "D = 512, full rank")
    assert np.array_equal(dist.view(np.uint32), (cost / plen.astype(np.float32)).astype(np.float32).view(np.uint32))


def test_path_lengths_and_the_returned_distance(cost_runs):
    total = left_out = 0
    for D in abx_ref.COST_DS:
        ref = abx_ref.cost_reference(D)
        c64, l64, _, gap, steps = ref["f64"]
        delta = abx_ref.K_DELTA * ref["frame_err"]
        keep = ~(gap < 2 * (steps + 1) * delta)
        # the seed of cost_case: the fp32 restatement itself agrees with float64 on every pair that is kept
        assert (ref["f32"][1][keep] == l64[keep]).all()
        cost, plen, dist = cost_runs[D]
        assert (plen[keep] == l64[keep]).all(), f"D = {D}: path lengths differ at {np.nonzero(plen != l64)[0]}"
        want = (cost[keep] / plen[keep].astype(np.float32)).astype(np.float32)
        assert np.array_equal(dist[keep].view(np.uint32), want.view(np.uint32))
        assert (plen >= 1).all() and (plen <= steps).all()
        total += keep.size
        left_out += int((~keep).sum())
    print(f"path lengths: {left_out} of {total} pairs left out")
    assert left_out <= PATH_CAP * total


def geometry_case():
    """Short tokens (1..8 frames, D = 20) over 600 rank-3 frames, and blocks of every shape the launch geometry has."""
    D, n = 20, 600
    pts = synth._normalish("abx/geo/pts", (n, 3), synth.SEED).numpy().astype(np.float64)
    mix = synth._normalish("abx/geo/mix", (3, D), synth.SEED).numpy().astype(np.float64)
    frames = (pts @ mix).astype(np.float32)
    lens = 1 + synth.randint("abx/geo/len", (120,), 8).numpy()
    first = synth.randint("abx/geo/first", (120,), n - 8).numpy()
    tokens = [(int(f), int(l)) for f, l in zip(first, lens)]
    ids = lambda name, k: [int(v) for v in synth.randint("abx/geo/" + name, (k,), 120).numpy()]
    pairs = [([3], [7]), (ids("a37", 37), ids("x5", 5)), (ids("a5", 5), ids("x37", 37))]
    within = ids("w", 9)
    pairs.append((within, within))                                     # D[a, a] is computed (and must be 0)
    na = 1 + synth.randint("abx/geo/na", (300,), 6).numpy()
    nx = 1 + synth.randint("abx/geo/nx", (300,), 5).numpy()
    for b in range(300):
        pairs.append((ids("ma%d" % b, int(na[b])), ids("mx%d" % b, int(nx[b]))))
    return frames, tokens, pairs


def test_block_geometry():
    frames, tokens, pairs = geometry_case()
    cost, plen, dist, _, r = run(frames, tokens, blocks_of(pairs))
    c64, l64, _, gap, steps = abx_ref.block_tables(frames, tokens, pairs)
    err = max(abx_ref.max_frame_error(frames, tokens, a, x) for a, x in pairs)
    assert cost.size == sum(len(a) * len(x) for a, x in pairs) == c64.size
    assert r.dist_base[1] == 1 and r.dist_base[2] == 1 + 37 * 5 and r.dist_base[4] == 1 + 2 * 37 * 5 + 81
    check_costs(cost, c64, steps, abx_ref.K_DELTA * err, "geometry, 304 blocks in one call")
    w0 = r.dist_base[3]
    diag = cost[w0:w0 + 81].reshape(9, 9).diagonal()
    assert (diag == 0.0).all() and (plen[w0:w0 + 81].reshape(9, 9).diagonal() == [tokens[k][1] for k in pairs[3][0]]).all()
    # every block alone gives the bits it has inside the big call (first four blocks), and a second call repeats them
    for b in range(4):
        alone = run(frames, tokens, blocks_of(pairs[b:b + 1]))
        n = len(pairs[b][0]) * len(pairs[b][1])
        for got, part in zip((cost, plen, dist), alone[:3]):
            assert np.array_equal(got[r.dist_base[b]:r.dist_base[b] + n], part)
    again = run(frames, tokens, blocks_of(pairs))
    for x, y in zip((cost, plen, dist), again[:3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def test_twice_wins_is_exact():
    """The counts equal the integer numpy count taken from the GPU's OWN distance table."""
    frames, tokens, _ = geometry_case()
    dup = len(tokens)
    tokens = tokens + [tokens[5], tokens[5], tokens[9]]               # other token ids on the same rows: exact distance ties
    blocks = [
        abx.Block([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], [0, 3, 4, 9, 12], [20, 21, 22, 2, 5, 11], [0, 1, 2, 0, 2, 3]),
        abx.Block([5, dup, dup + 1, 9, dup + 2, 30], [0, 2, 4, 6], [5, 9, 40, dup], [0, 1, 2, 0]),        # ties, and a == x
        abx.Block([12, 13, 14], [0, 3], [12, 50], [0, 0]),                                           # one segment: nothing to count
        abx.Block(list(range(40, 80)), [0, 7, 7, 20, 40], list(range(60, 100)), [0] * 10 + [2] * 15 + [3] * 15),   # an empty segment
    ]
    _, _, dist, tw, r = run(frames, tokens, blocks)
    assert tw.dtype == np.int32 and tw.size == sum(len(b.x) * b.n_seg for b in blocks)
    for i, b in enumerate(blocks):
        d = dist[r.dist_base[i]:r.dist_base[i] + len(b.a) * len(b.x)].reshape(len(b.a), len(b.x))
        got = tw[r.out_base[i]:r.out_base[i] + len(b.x) * b.n_seg].reshape(len(b.x), b.n_seg)
        want = abx_ref.twice_wins_of(d, b.a, b.seg, b.x, b.x_seg)
        assert np.array_equal(got, want), f"block {i}"
        assert (want <= 2 * b.n_triples()).all()
    d1 = dist[r.dist_base[1]:r.dist_base[1] + 24].reshape(6, 4)
    assert d1[0, 0] == 0.0 and d1[1, 0] == 0.0 and np.array_equal(d1[1], d1[2]) and np.array_equal(d1[3], d1[4])
    one = tw[r.out_base[2]:r.out_base[2] + 2]
    assert (one == 0).all()
    assert tw[r.out_base[1]:r.out_base[1] + 12].reshape(4, 3).sum() > 0


def cells_from_gpu_distances(items, frames, tokens, mode):
    """Brute-force cells from the GPU's own token distances (every block of the plan in one call)."""
    pl = abx.plan(items, mode)
    _, _, dist, _, r = run(frames, tokens, pl.blocks)
    n = len(items)
    D = np.full((n, n), np.nan)
    for i, b in enumerate(pl.blocks):
        D[np.ix_(b.a, b.x)] = dist[r.dist_base[i]:r.dist_base[i] + len(b.a) * len(b.x)].reshape(len(b.a), len(b.x))
    return D


@pytest.mark.parametrize("mode", ["within", "across"])
@pytest.mark.parametrize("name", ["small", "200"])
def test_score_end_to_end_against_brute_force(name, mode):
    items, feats, frames, tokens, ref = abx_ref.e2e_reference(name)
    delta = abx_ref.K_DELTA * ref["frame_err"]
    skip = abx_ref.near_tie(ref, delta)
    full, _ = abx_ref.brute_force(items, ref["dist"], mode)
    total = sum(n for _, n in full.values())
    want, excluded = abx_ref.brute_force(items, ref["dist"], mode, skip)
    print(f"{name} {mode}: {excluded} of {total} triples left out as near-ties of float64")
    assert excluded <= TRIPLE_CAP * total
    Dg = cells_from_gpu_distances(items, frames, tokens, mode)
    got, _ = abx_ref.brute_force(items, Dg, mode, skip)
    assert got == want                                                  # every cell's (twice_wins, n)
    res = abx.score({f: torch.from_numpy(v).cuda() for f, v in feats.items()}, items, mode=mode)
    assert res["cells"] == abx_ref.brute_force(items, Dg, mode)[0]      # plan + count kernel + aggregate on the GPU's own distances
    assert res["n_triples"] == total
    assert abs(res["score"] - abx_ref.score_of(full, mode)) <= excluded / total + 1e-12
    assert abs(res["error_rate"] - 100.0 * (1.0 - res["score"])) < 1e-9


def test_chunked_score_equals_one_call():
    items, feats, _, _, _ = abx_ref.e2e_reference("small")
    dev = {f: torch.from_numpy(v).cuda() for f, v in feats.items()}
    for mode in ("within", "across"):
        one = abx.score(dev, items, mode=mode)
        pl = abx.plan(items, mode)
        cut = abx.score(dev, items, mode=mode, mem_budget_bytes=3 * max(abx.block_bytes(b) for b in pl.blocks))
        assert one["n_chunks"] == 1 and 1 < cut["n_chunks"] < len(pl.blocks)
        assert np.array_equal(one["twice_wins"], cut["twice_wins"]) and one["score"] == cut["score"]
        each = abx.score(dev, items, mode=mode, mem_budget_bytes=1)
        assert each["n_chunks"] == len(pl.blocks) and each["score"] == one["score"]


def _encoder():
    import vectorquantizedcpc_amd as V
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict())            # what --random-init loads
    return enc.cuda().eval()


def _dataset(tmp_path):
    """Six mels of 40..80 frames under <tmp>/datasets/d, test.json, and an items file over their 20..40 code frames."""
    import json
    root = tmp_path / "datasets" / "d"
    root.mkdir(parents=True)
    lens = [40, 47, 56, 63, 72, 80]
    mels, meta, lines = {}, [], ["#file onset offset #phone prev next speaker"]
    u = synth.uniform01("abx/cli", 400)
    k = 0
    for i, T in enumerate(lens):
        name = f"s{i % 2}_u{i}"
        mel = synth.mel("abx/" + name, 1, T)[0]
        np.save(root / (name + ".mel.npy"), mel.numpy())
        meta.append([0, 0, 0, f"d/{name}"])
        mels[name] = mel
        dur = 0.02 * (T // 2)
        for ph in ("aa", "iy", "uw", "aa", "iy"):
            on = u[k] * (dur - 0.2); ln = 0.03 + 0.15 * u[k + 1]; k += 2
            lines.append(f"{name} {on:.3f} {on + ln:.3f} {ph} {'b' if u[k] < 0.5 else 'd'} t s{i % 2}")
            k += 1
    (root / "test.json").write_text(json.dumps(meta))
    (tmp_path / "x.item").write_text("\n".join(lines) + "\n")
    return root, mels, tmp_path / "x.item"


@pytest.mark.parametrize("feature", ["z", "c"])
def test_driver_score_abx_equals_cli_encode_then_cli_abx(tmp_path, capsys, feature):
    root, mels, items_path = _dataset(tmp_path)
    enc = _encoder()
    res = driver.score_abx(enc, mels, str(items_path), feature=feature, mode="across")
    assert res["n_triples"] > 0 and 0.0 <= res["score"] <= 1.0
    out = tmp_path / "out" / "z"
    args = ["encode", "--dataset", str(root), "--out-dir", str(out), "--random-init"] + (["--save-auxiliary"] if feature == "c" else [])
    assert cli.main(args) == 0
    feat_dir = out if feature == "z" else tmp_path / "out" / "auxiliary_embedding1"
    capsys.readouterr()
    assert cli.main(["abx", "--items", str(items_path), "--mode", "across", "--features", str(feat_dir)]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert line == cli.abx_line(res)
    text = {f: torch.from_numpy(io.load_frames_text(feat_dir / f)).cuda() for f in mels}
    again = abx.score(text, str(items_path), mode="across")
    assert np.array_equal(again["twice_wins"], res["twice_wins"]) and again["score"] == res["score"]
    assert cli.main(["abx", "--items", str(items_path), "--mode", "across", "--dataset", str(root), "--random-init",
                     "--feature", feature]) == 0
    assert capsys.readouterr().out.strip().splitlines()[-1] == line


def test_errors_are_rejected_before_anything_is_enqueued():
    dev = torch.device("cuda")
    blk = [abx.Block([0], [0, 1], [1], [0])]
    with pytest.raises(ValueError, match="D = 6"):
        abx.pair_distances(torch.zeros(100, 6, device=dev), [(0, 2), (2, 2)], blk)
    with pytest.raises(ValueError, match="65 frames"):
        abx.pair_distances(torch.zeros(100, 8, device=dev), [(0, 65), (2, 2)], blk)
    with pytest.raises(IndexError):
        abx.pair_distances(torch.zeros(100, 8, device=dev), [(-1, 2), (2, 2)], blk)
    with pytest.raises(IndexError):
        abx.pair_distances(torch.zeros(100, 8, device=dev), [(0, 2), (2, 2)], [abx.Block([0], [0, 1], [-1], [0])])
    lib = _lib.load()
    n = C.c_uint64()
    assert lib.vqcpc_abx_workspace_bytes(100, 8, C.byref(n)) == 0 and n.value == 3200
    assert lib.vqcpc_abx_workspace_bytes(100, 6, C.byref(n)) == -1 and b"D = 6" in lib.vqcpc_last_error()
    assert lib.vqcpc_abx_workspace_bytes(100, 516, C.byref(n)) == -1
    f = torch.zeros(100, 8, device=dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    tok, lists, segs, rows = i32([0, 2, 2, 2]), i32([0, 1, 0]), i32([0, 1]), i32([0, 1, 1, 1, 0, 1, 0, 0, 2, 0, 0, 0])
    work = torch.zeros(800, device=dev)
    dist = torch.full((1,), -7.0, device=dev)
    tw = torch.full((1,), -7, dtype=torch.int32, device=dev)

    def call(D=8, feats=f, n_blocks=1, n_dist=1, d=dist):
        return lib.vqcpc_abx_score(feats.data_ptr() if feats is not None else None, 100, D, tok.data_ptr(), 2, lists.data_ptr(), 3,
                                   segs.data_ptr(), 2, rows.data_ptr(), n_blocks, 1, n_dist, 1, work.data_ptr(), None, None,
                                   d.data_ptr() if d is not None else None, tw.data_ptr(), None)

    assert call(D=6) == -1 and b"D = 6" in lib.vqcpc_last_error()
    assert call(D=516) == -1 and call(D=0) == -1
    assert call(feats=None) == -1 and b"null" in lib.vqcpc_last_error()
    assert call(d=None) == -1
    assert call(n_blocks=0) == -1 and call(n_dist=0) == -1 and call(n_dist=1 << 31) == -1
    torch.cuda.synchronize()
    assert float(dist[0]) == -7.0 and int(tw[0]) == -7                  # nothing was enqueued
    assert call() == 0                                                  # the same tables are a valid call: cost NULL, path_len NULL
    torch.cuda.synchronize()
    assert float(dist[0]) == 0.0 and int(tw[0]) == 0                    # two zero tokens: distance 0; one segment: nothing counted
