"""-m gpu: the index form of ABX scoring (csrc/abx.hip: code table, index DTW, edit metric; abx.py, driver, cli).

Angular metric: everything is compared with the feature path on ``codebook[codes]`` BIT FOR BIT (no tolerance, nothing left
out); the table itself also against float64 inside the project's delta = abx_ref.K_DELTA x the fp32 numpy restatement's largest
frame-distance error on the same rows.  Edit metric: bit for bit against the numpy reference of tests/abx_index_ref.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import abx_index_ref as R
import abx_ref
from vectorquantizedcpc_amd import _lib, abx, cli, driver

pytestmark = pytest.mark.gpu

SHAPES = [(24, 4), (24, 20), (512, 64), (513, 64), (7, 512), (1, 8)]          # (M, D); D = 20: a partial last chunk


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cost_blocks():
    """abx_ref.COST_BLOCKS as one-segment blocks; the dense block of short tokens gets two segments, so that counts are made."""
    blocks = [abx.Block(a, [0, len(a)], x, [0] * len(x)) for a, x in abx_ref.COST_BLOCKS[:-1]]
    a, x = abx_ref.COST_BLOCKS[-1]
    return blocks + [abx.Block(a, [0, 3, len(a)], x, [k % 2 for k in range(len(x))])]


def assert_same(got, want, what=""):
    for name in ("cost", "path_len", "dist", "twice_wins"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.dtype == w.dtype and torch.equal(g.view(torch.int32), w.view(torch.int32)), f"{what}{name}"
    assert got.dist_base == want.dist_base and got.out_base == want.out_base


@pytest.mark.parametrize("M,D", SHAPES)
def test_index_path_equals_feature_path_bit_for_bit(M, D):
    book = R.codebook(M, D)
    codes, tokens = R.cost_codes(M)
    blocks = cost_blocks()
    want = abx.pair_distances(dev(book[codes]), tokens, blocks)
    table = abx.code_table(dev(book))
    got = abx.pair_distances_indices(dev(codes), tokens, blocks, table=table)
    assert_same(got, want)
    assert_same(abx.pair_distances_indices(dev(codes.astype(np.int32)), tokens, blocks, table=table, n_codes=M), want)
    assert torch.isfinite(got.cost).all()
    if M == 1:
        assert not got.cost.any() and not got.dist.any() and not table.any()
    else:
        assert int(got.twice_wins.sum()) > 0 and got.cost.any()
    nocost = abx.pair_distances_indices(dev(codes), tokens, blocks, table=table, want_cost=False)
    assert nocost.cost is None and nocost.path_len is None and torch.equal(nocost.dist, want.dist)


def rowwise(fn, book, step=64):
    return np.concatenate([fn(book[r:r + step], book) for r in range(0, book.shape[0], step)])


@pytest.mark.parametrize("M,D", [(24, 20), (512, 64)])
def test_the_table_itself(M, D):
    book = R.codebook(M, D)
    table = abx.code_table(dev(book))
    assert table.shape == (M, M) and table.dtype == torch.float32 and table.is_contiguous()
    # the feature path's cost of the 1-frame pair (row i, row j), all M x M of them in one block
    ids = list(range(M))
    pairs = abx.pair_distances(dev(book), [(i, 1) for i in ids], [abx.Block(ids, [0, M], ids, [0] * M)])
    assert torch.equal(table.view(torch.int32), pairs.cost.view(M, M).view(torch.int32))
    assert (pairs.path_len == 1).all()
    t = table.cpu().numpy()
    assert not np.diag(t).any()                                           # exactly 0
    assert np.array_equal(t.view(np.uint32), t.T.view(np.uint32))
    f64 = rowwise(abx_ref.frame_dist, book)
    f32 = rowwise(lambda a, b: abx_ref.frame_dist(a, b, np.float32), book)
    e = float(np.abs(f32.astype(np.float64) - f64).max())
    bound = abx_ref.K_DELTA * e
    err = float(np.abs(t.astype(np.float64) - f64).max())
    print(f"M = {M}, D = {D}: max |table - float64| = {err:.3g}, bound {bound:.3g} (restatement's error {e:.3g})")
    assert err <= bound
    z, (t0, t1), (g, ng) = R.ZERO_ROW, R.TWIN_ROWS, R.NEG_ROWS
    others = np.array([j for j in ids if j != z])
    assert t[z, z] == 0.0 and (t[z, others] == 0.5).all()                 # the zero row: exactly 0.5 from every non-zero row
    assert t[t0, t1] == 0.0 and t[t1, t0] == 0.0 and np.array_equal(t[t0].view(np.uint32), t[t1].view(np.uint32))
    assert abs(float(t[g, ng]) - 1.0) <= bound


def test_block_geometry():
    book, codes, tokens, pairs = R.geometry_case()
    blocks = [abx.Block(a, [0, len(a)], x, [0] * len(x)) for a, x in pairs]
    table = abx.code_table(dev(book))
    r = abx.pair_distances_indices(dev(codes), tokens, blocks, table=table)
    assert r.cost.numel() == sum(len(a) * len(x) for a, x in pairs)
    assert r.dist_base[1] == 1 and r.dist_base[2] == 1 + 37 * 5 and r.dist_base[4] == 1 + 2 * 37 * 5 + 81
    assert_same(r, abx.pair_distances(dev(book[codes]), tokens, blocks))
    w0 = r.dist_base[3]
    assert not r.cost[w0:w0 + 81].view(9, 9).diagonal().any()
    assert r.path_len[w0:w0 + 81].view(9, 9).diagonal().tolist() == [tokens[k][1] for k in pairs[3][0]]
    for metric in ("angular", "edit"):
        big = abx.pair_distances_indices(dev(codes), tokens, blocks, table=table, metric=metric)
        for b in range(4):                                               # a block alone has the bits it has inside the big call
            alone = abx.pair_distances_indices(dev(codes), tokens, blocks[b:b + 1], table=table, metric=metric)
            n = len(pairs[b][0]) * len(pairs[b][1])
            for name in ("cost", "path_len", "dist"):
                assert torch.equal(getattr(big, name)[big.dist_base[b]:big.dist_base[b] + n], getattr(alone, name)), (metric, b, name)
        assert_same(abx.pair_distances_indices(dev(codes), tokens, blocks, table=table, metric=metric), big, metric + " again: ")
    want = R.edit_block_tables(codes, tokens, pairs)
    for g, w in zip((big.cost, big.path_len, big.dist), want):
        assert np.array_equal(g.cpu().numpy(), w.astype(g.cpu().numpy().dtype))


@pytest.mark.parametrize("mode", ["within", "across"])
@pytest.mark.parametrize("name", ["small", "200"])
def test_score_indices_equals_score_on_the_frames(name, mode):
    items, book, idx, _, _ = R.e2e_indices(name)
    feats = {f: dev(book[v]) for f, v in idx.items()}
    want = abx.score(feats, items, mode=mode)
    got = abx.score_indices(dev(book), {f: dev(v) for f, v in idx.items()}, items, mode=mode)
    assert got["metric"] == "angular" and got["mode"] == mode and got["n_triples"] == want["n_triples"] > 0
    assert np.array_equal(got["twice_wins"], want["twice_wins"]) and got["score"] == want["score"] and got["cells"] == want["cells"]
    assert got["n_blocks"] == want["n_blocks"] and got["n_chunks"] == 1
    if name == "small":
        pl = abx.plan(items, mode)
        cut = abx.score_indices(dev(book), {f: dev(v).to(torch.int32) for f, v in idx.items()}, items, mode=mode,
                                mem_budget_bytes=3 * max(abx.block_bytes(b) for b in pl.blocks))
        assert 1 < cut["n_chunks"] < len(pl.blocks)
        assert np.array_equal(cut["twice_wins"], want["twice_wins"]) and cut["score"] == want["score"]


@pytest.mark.parametrize("M", [24, 513, 1])
def test_edit_metric_is_exact(M):
    codes, tokens = R.cost_codes(M)
    blocks = cost_blocks()
    got = abx.pair_distances_indices(dev(codes), tokens, blocks, n_codes=M, metric="edit")
    cost, plen, dist = R.edit_block_tables(codes, tokens, abx_ref.COST_BLOCKS)
    assert got.cost.dtype == torch.float32 and got.path_len.dtype == torch.int32
    assert np.array_equal(got.cost.cpu().numpy().view(np.uint32), cost.view(np.uint32))
    assert np.array_equal(got.path_len.cpu().numpy(), plen.astype(np.int32))
    assert np.array_equal(got.dist.cpu().numpy().view(np.uint32), dist.view(np.uint32))
    a, x = abx_ref.COST_BLOCKS[-1]
    b = blocks[-1]
    d = dist[-len(a) * len(x):].reshape(len(a), len(x))
    tw = got.twice_wins.cpu().numpy()[got.out_base[-1]:].reshape(len(x), b.n_seg)
    assert np.array_equal(tw, abx_ref.twice_wins_of(d, b.a, b.seg, b.x, b.x_seg))
    if M > 1:
        # given a table, the edit metric does not read it: the same bits
        table = abx.code_table(dev(R.codebook(M, 8)))
        assert_same(abx.pair_distances_indices(dev(codes), tokens, blocks, table=table, metric="edit"), got)
        # the two bit-equal codebook rows are ONE frame to the angular metric and TWO symbols to the edit metric
        twins, one = dev(np.array(R.TWIN_ROWS)), [abx.Block([0], [0, 1], [1], [0])]
        ang = abx.pair_distances_indices(twins, [(0, 1), (1, 1)], one, table=table)
        ed = abx.pair_distances_indices(twins, [(0, 1), (1, 1)], one, table=table, metric="edit")
        assert float(ang.cost[0]) == 0.0 and float(ed.cost[0]) == 1.0 and float(ed.dist[0]) == 1.0 and int(ed.path_len[0]) == 1


@pytest.mark.parametrize("mode", ["within", "across"])
@pytest.mark.parametrize("name", ["small", "200"])
def test_edit_score_end_to_end_against_brute_force(name, mode):
    items, book, idx, codes, tokens, D = R.e2e_edit_reference(name)
    want, _ = abx_ref.brute_force(items, D, mode)
    on_dev = {f: dev(v) for f, v in idx.items()}
    res = abx.score_indices(None, on_dev, items, mode=mode, metric="edit")
    assert res["metric"] == "edit" and res["cells"] == want              # every cell, ties included, nothing left out
    assert res["n_triples"] == sum(n for _, n in want.values()) > 0
    assert abs(res["score"] - abx_ref.score_of(want, mode)) < 1e-12
    with_book = abx.score_indices(dev(book), on_dev, items, mode=mode, metric="edit")
    assert np.array_equal(with_book["twice_wins"], res["twice_wins"])


def test_driver_and_cli_on_indices(tmp_path, capsys):
    from test_gpu_abx import _dataset, _encoder
    root, mels, items_path = _dataset(tmp_path)
    enc = _encoder()
    z = driver.score_abx(enc, mels, str(items_path), feature="z", mode="across")
    ind = driver.score_abx(enc, mels, str(items_path), feature="indices", mode="across")
    assert ind["n_triples"] == z["n_triples"] > 0 and np.array_equal(ind["twice_wins"], z["twice_wins"]) and ind["score"] == z["score"]
    assert ind["metric"] == "angular" and cli.abx_line(ind) == cli.abx_line(z)
    base = ["abx", "--items", str(items_path), "--mode", "across", "--dataset", str(root), "--random-init"]
    lines = {}
    for key, extra in (("z", ["--feature", "z"]), ("indices", ["--feature", "indices"]),
                       ("edit", ["--feature", "indices", "--metric", "edit"])):
        capsys.readouterr()
        assert cli.main(base + extra) == 0
        lines[key] = capsys.readouterr().out.strip().splitlines()[-1]
    assert lines["indices"] == lines["z"] == cli.abx_line(z)
    edit = driver.score_abx(enc, mels, str(items_path), feature="indices", mode="across", metric="edit")
    assert lines["edit"] == cli.abx_line(edit) and lines["edit"].endswith(", metric edit") and lines["edit"].startswith("abx across:")
    assert edit["n_triples"] == z["n_triples"] and 0.0 <= edit["score"] <= 1.0
    for bad in (["--feature", "z", "--metric", "edit"],):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    with pytest.raises(SystemExit):
        cli.main(["abx", "--items", str(items_path), "--features", str(tmp_path), "--feature", "indices"])
    capsys.readouterr()


def test_errors_are_rejected_before_anything_is_enqueued():
    d = torch.device("cuda")
    blk = [abx.Block([0], [0, 1], [1], [0])]
    items = [abx.Item("f", 0.0, 0.1, "p0", "a", "b", "s"), abx.Item("f", 0.2, 0.3, "p1", "a", "b", "s"),
             abx.Item("f", 0.4, 0.5, "p0", "a", "b", "s")]
    book = torch.ones(24, 8, device=d)
    codes = torch.zeros(100, dtype=torch.int64, device=d)
    assert abx.score_indices(book, {"f": codes}, items)["n_triples"] > 0
    for bad in (24, -1):
        c = codes.clone()
        c[50] = bad
        for metric in ("angular", "edit"):
            with pytest.raises(IndexError, match="'f'"):
                abx.score_indices(book, {"f": c}, items, metric=metric)
    with pytest.raises(IndexError):
        abx.score_indices(None, {"f": c}, items, metric="edit")          # no codebook: a negative index is still refused
    with pytest.raises(ValueError, match="metric"):
        abx.score_indices(book, {"f": codes}, items, metric="kl")
    with pytest.raises(ValueError, match="metric"):
        abx.pair_distances_indices(codes, [(0, 2), (2, 2)], blk, n_codes=24, metric="kl")
    with pytest.raises(ValueError, match="codebook"):
        abx.score_indices(None, {"f": codes}, items)
    with pytest.raises(ValueError, match="table"):
        abx.pair_distances_indices(codes, [(0, 2), (2, 2)], blk, n_codes=24)
    with pytest.raises(ValueError, match="edit"):
        driver.score_abx(None, {}, items, feature="z", metric="edit")
    with pytest.raises(ValueError, match="kl"):
        driver.score_abx(None, {}, items, feature="indices", metric="kl")
    with pytest.raises(ValueError, match="65 frames"):
        abx.pair_distances_indices(codes, [(0, 65), (2, 2)], blk, n_codes=24, metric="edit")
    with pytest.raises(ValueError, match="integer"):
        abx.pair_distances_indices(codes.float(), [(0, 2), (2, 2)], blk, n_codes=24, metric="edit")
    with pytest.raises(ValueError, match="4097"):
        abx.pair_distances_indices(codes, [(0, 2), (2, 2)], blk, n_codes=4097, metric="edit")
    with pytest.raises(ValueError, match="D = 6"):
        abx.code_table(torch.ones(24, 6, device=d))
    with pytest.raises(ValueError, match="4097"):
        abx.code_table(torch.ones(4097, 8, device=d))

    lib = _lib.load()
    n = C.c_uint64()
    assert lib.vqcpc_abx_index_workspace_bytes(512, 64, C.byref(n)) == 0 and n.value == 512 * 64 * 4 + 512 * 512 * 4
    assert lib.vqcpc_abx_index_workspace_bytes(0, 64, C.byref(n)) == -1 and b"M = 0" in lib.vqcpc_last_error()
    assert lib.vqcpc_abx_index_workspace_bytes(4097, 64, C.byref(n)) == -1 and lib.vqcpc_abx_index_workspace_bytes(512, 6, C.byref(n)) == -1
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=d)
    tok, lists, segs, rows = i32([0, 2, 2, 2]), i32([0, 1, 0]), i32([0, 1]), i32([0, 1, 1, 1, 0, 1, 0, 0, 2, 0, 0, 0])
    cd = torch.zeros(100, dtype=torch.int32, device=d)
    cd[1] = 3
    bk = torch.ones(24, 8, device=d)
    work = torch.zeros(24 * 8, device=d)
    table = torch.full((24, 24), -7.0, device=d)
    dist = torch.full((1,), -7.0, device=d)
    tw = torch.full((1,), -7, dtype=torch.int32, device=d)

    def build(M=24, D=8, book=bk, w=work, t=table):
        p = lambda v: v if isinstance(v, int) or v is None else v.data_ptr()
        return lib.vqcpc_abx_code_table(p(book), M, D, p(w), p(t), None)

    def call(M=24, t=table, metric=0, codes=cd, n_dist=1):
        return lib.vqcpc_abx_score_indices(t.data_ptr() if t is not None else None, M, codes.data_ptr() if codes is not None else None, 100,
                                           tok.data_ptr(), 2, lists.data_ptr(), 3, segs.data_ptr(), 2, rows.data_ptr(), 1, 1, n_dist, 1,
                                           None, None, dist.data_ptr(), tw.data_ptr(), None, metric)

    assert build(M=0) == -1 and b"M = 0" in lib.vqcpc_last_error()
    assert build(M=4097) == -1 and build(D=6) == -1 and b"D = 6" in lib.vqcpc_last_error()
    assert build(book=None) == -1 and build(w=None) == -1 and build(t=None) == -1 and b"null" in lib.vqcpc_last_error()
    assert build(book=bk.data_ptr() + 4) == -1 and build(t=table.data_ptr() + 4) == -1 and build(w=work.data_ptr() + 8) == -1
    assert b"aligned" in lib.vqcpc_last_error()
    assert call(M=0) == -1 and call(M=4097) == -1 and b"M = 4097" in lib.vqcpc_last_error()
    assert call(metric=2) == -1 and b"metric = 2" in lib.vqcpc_last_error() and call(metric=-1) == -1
    assert call(t=None) == -1 and b"table" in lib.vqcpc_last_error()
    assert call(codes=None) == -1 and call(n_dist=0) == -1 and call(n_dist=1 << 31) == -1
    torch.cuda.synchronize()
    assert float(dist[0]) == -7.0 and int(tw[0]) == -7 and float(table[0, 0]) == -7.0          # nothing was enqueued
    assert build() == 0 and call() == 0                               # equal rows: every distance is 0
    torch.cuda.synchronize()
    assert not table.any() and float(dist[0]) == 0.0 and int(tw[0]) == 0
    assert call(t=None, metric=1) == 0                                # the edit metric takes no table: runs (0, 3) and (0, 0)
    torch.cuda.synchronize()
    assert float(dist[0]) == 0.5 and int(tw[0]) == 0
