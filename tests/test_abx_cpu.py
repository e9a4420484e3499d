"""ABX scoring, the parts that need no GPU: items and frame windows, the block plan and the aggregation against a brute-force
enumeration of every triple, the float64 reference's own DTW on hand-checked cases, and the no-fallback rule."""
import numpy as np
import pytest
import torch

import abx_ref
from vectorquantizedcpc_amd import abx

SPEAKERS = ["s0", "s1", "s2"]
CONTEXTS = [("a", "b"), ("c", "d"), ("e", "f")]
PHONES = ["p0", "p1", "p2", "p3"]


def small_set():
    items = abx_ref.item_set("cpu", SPEAKERS, CONTEXTS, PHONES, 1, 3)
    feats = abx_ref.features_for(items, 8, "cpu")
    return items, feats


def test_read_items_and_frame_windows(tmp_path):
    p = tmp_path / "x.item"
    p.write_text("#file onset offset #phone prev-phone next-phone speaker\n"
                 "f1 0.10 0.20 aa b c s1\n"
                 "f1  0.105   0.109 iy b c s1\n"
                 "\n"
                 "f2 0.00 1.27 aa x y s2\n"
                 "f2 0.00 1.29 aa x y s2\n")
    items = abx.read_items(p)
    assert [i.phone for i in items] == ["aa", "iy", "aa", "aa"] and items[0].speaker == "s1" and items[2].prev == "x"
    assert items[1].onset == 0.105 and items[1].offset == 0.109
    n = {"f1": 50, "f2": 100}
    # default: frame j at 0.01 + 0.02 j -> 0.11, 0.13, 0.15, 0.17, 0.19 are frames 5..9
    assert abx.tokens_of(items[:1], n) == [(5, 5)]
    # a token between two frame times takes the frame nearest its midpoint (0.107 -> frame 5 at 0.11)
    assert abx.tokens_of(items[1:2], n) == [(5, 1)]
    # 0.00 .. 1.27: frames 0 (0.01) .. 63 (1.27) = 64 frames, still allowed
    assert abx.tokens_of(items[2:3], n) == [(0, 64)]
    with pytest.raises(ValueError, match=r"f2 0.0 1.29 aa.*65 frames"):
        abx.tokens_of(items[3:], n)
    # another shift and offset: frame j at 0.005 + 0.01 j -> [0.10, 0.20] holds frames 10 (0.105) .. 19 (0.195)
    assert abx.tokens_of(items[:1], n, frame_shift=0.01, frame_offset=0.005) == [(10, 10)]
    # a window is cut to the file's frames
    assert abx.tokens_of(items[:1], {"f1": 8, "f2": 1}) == [(5, 3)]
    with pytest.raises(KeyError):
        abx.tokens_of(items, {"f1": 50})
    bad = tmp_path / "bad.item"
    bad.write_text("f1 0.1 0.2 aa b c s1\n")
    with pytest.raises(ValueError, match="header"):
        abx.read_items(bad)


@pytest.mark.parametrize("mode", ["within", "across"])
def test_plan_and_aggregate_equal_brute_force(mode):
    items, feats = small_set()
    files = sorted(feats)
    first = np.cumsum([0] + [feats[f].shape[0] for f in files])
    tok = abx.tokens_of(items, {f: feats[f].shape[0] for f in files})
    tokens = [(int(first[files.index(it.file)]) + lo, n) for it, (lo, n) in zip(items, tok)]
    frames = np.concatenate([feats[f] for f in files])
    D = abx_ref.all_pairs(frames, tokens)
    want, _ = abx_ref.brute_force(items, D, mode)
    pl = abx.plan(items, mode)
    assert pl.blocks and all(b.context != ("only", "one") for b in pl.blocks)      # the single-phone context drops out
    if mode == "within":
        assert all(b.s_ab == b.s_x and b.s_ab != "lone" for b in pl.blocks)
    else:
        assert all(b.s_ab != b.s_x for b in pl.blocks) and any(b.s_x == "lone" for b in pl.blocks)
    for b in pl.blocks:
        ph = [items[k].phone for k in b.a]
        assert ph == sorted(ph) and [ph[s] for s in b.seg[:-1]] == b.phones
    tw = np.concatenate([abx_ref.twice_wins_of(D[np.ix_(b.a, b.x)], b.a, b.seg, b.x, b.x_seg).reshape(-1) for b in pl.blocks])
    got = abx.aggregate(pl, tw)
    assert got["cells"] == want                                       # (sum twice_wins, sum n) per cell, as integers
    assert got["n_triples"] == sum(n for _, n in want.values()) > 100
    ref = abx_ref.score_of(want, mode)
    assert abs(got["score"] - ref) <= 1e-12 and abs(got["error_rate"] - 100.0 * (1.0 - ref)) <= 1e-10
    assert 0.0 <= got["score"] <= 1.0 and got["n_pairs"] == sum(len(b.a) * len(b.x) for b in pl.blocks)
    pairs = {(k[0], k[1]) for k in want}
    assert set(got["by_phone_pair"]) == pairs


def test_reference_dtw_hand_cases():
    e = np.eye(4)
    # 1 x 1
    c, l, g = abx_ref.dtw(abx_ref.frame_dist(e[:1], e[1:2]))
    assert c == 0.5 and l == 1 and g == np.inf
    # 1 x 5: one row, every cell on the path
    b = np.stack([e[0], e[1], e[0], -e[0], e[2]])
    d = abx_ref.frame_dist(e[:1], b)
    assert np.allclose(d, [[0.0, 0.5, 0.0, 1.0, 0.5]], atol=1e-15) and d[0, 0] == 0.0 and d[0, 2] == 0.0
    c, l, _ = abx_ref.dtw(d)
    assert abs(c - 2.0) < 1e-15 and l == 5
    # identical sequences: cost exactly 0, path = the diagonal
    s = np.random.default_rng(1).normal(size=(7, 6))
    c, l, g = abx_ref.dtw(abx_ref.frame_dist(s, s))
    assert c == 0.0 and l == 7 and g > 0
    # a zero frame: 0.5 against a non-zero frame, 0 against a zero frame
    z = np.zeros((1, 4))
    assert abx_ref.frame_dist(z, e[:1])[0, 0] == 0.5 and abx_ref.frame_dist(z, z)[0, 0] == 0.0
    # an exact tie where the order decides the length: at (1, 1) the diagonal (cost 1) ties (0, 1) (cost 1 + 0);
    # the diagonal is first, so the path has 2 cells; taking (0, 1) would make it 3
    d = np.array([[1.0, 0.0], [5.0, 1.0]])
    c, l, g = abx_ref.dtw(d)
    assert c == 2.0 and l == 2 and g == 0.0
    # ties on two rows: at (1, 1) diagonal, up and left all cost 1 -> the diagonal, length 2; at (2, 1) the diagonal C[1][0]
    # ties up C[1][1], both of length 2 -> the diagonal, 3 cells
    d = np.array([[1.0, 0.0], [0.0, 0.0], [9.0, 0.0]])
    c, l, g = abx_ref.dtw(d)
    assert c == 1.0 and l == 3 and g == 0.0
    # the fp32 restatement agrees with float64 to fp32 precision on random frames
    a, b = s.astype(np.float32), np.random.default_rng(2).normal(size=(5, 6)).astype(np.float32)
    assert np.abs(abx_ref.frame_dist(a, b, np.float32) - abx_ref.frame_dist(a, b)).max() < 5e-7


def test_score_has_no_cpu_fallback():
    items, feats = small_set()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        abx.score({f: torch.from_numpy(v) for f, v in feats.items()}, items)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        abx.pair_distances(torch.zeros(4, 8), [(0, 2), (2, 2)], [abx.Block([0, 1], [0, 1, 2], [0], [0])])


def test_chunk_rule_and_table_validation():
    items, _ = small_set()
    pl = abx.plan(items, "across")
    sizes = [abx.block_bytes(b) for b in pl.blocks]
    one = abx.block_chunks(pl.blocks, 1 << 30)
    assert one == [list(range(len(pl.blocks)))]
    cut = abx.block_chunks(pl.blocks, max(sizes))
    assert len(cut) > 1 and sum(cut, []) == one[0]
    assert all(sum(sizes[i] for i in ids) <= max(sizes) for ids in cut)
    assert abx.block_chunks(pl.blocks, 1) == [[i] for i in one[0]]                # at least one block per call
    blk = abx.Block([0, 1], [0, 1, 2], [0], [0])
    with pytest.raises(ValueError, match="65 frames"):
        abx._tables([(0, 65), (0, 2)], [blk], 100)
    with pytest.raises(IndexError):
        abx._tables([(-1, 2), (0, 2)], [blk], 100)
    with pytest.raises(IndexError):
        abx._tables([(0, 2), (99, 2)], [blk], 100)
    with pytest.raises(IndexError):
        abx._tables([(0, 2)], [blk], 100)
    tok, lists, segs, rows, wg, nd, no = abx._tables([(0, 2), (2, 3)], [blk, abx.Block([1, 0, 1, 0, 1], [0, 5], [1, 0], [0, 0])], 100)
    assert rows.shape == (2, 12) and wg == 1 + 2 * 2 and nd == 2 + 10 and no == 2 + 2
    assert list(rows[1][[6, 7, 9]]) == [2, 2, 1]


@pytest.mark.parametrize("mode", ["within", "across"])
def test_fp32_restatement_stays_under_the_triple_cap(mode):
    """What pins the seed of the end-to-end GPU test: on the small set the triples left out as near-ties of float64 stay under the
    1 % cap, and outside them the fp32 numpy restatement's distances give every cell the count float64's give."""
    items, feats, frames, tokens = abx_ref.e2e_set("small")
    ref = abx_ref.context_tables(items, frames, tokens, restate=True)
    skip = abx_ref.near_tie(ref, abx_ref.K_DELTA * ref["frame_err"])
    total = sum(n for _, n in abx_ref.brute_force(items, ref["dist"], mode)[0].values())
    want, excluded = abx_ref.brute_force(items, ref["dist"], mode, skip)
    got, _ = abx_ref.brute_force(items, ref["dist32"].astype(np.float64), mode, skip)
    assert 0 < total and excluded <= 0.01 * total
    assert got == want


def test_fp32_restatement_of_the_cost_cases_is_inside_the_bound():
    """K_DELTA comes from here, not from a GPU: the fp32 numpy restatement's own cost error, DP additions included, stays
    below (Ta + Tb - 1) x its largest frame-distance error, on the rank-3 frames and on full-rank ones; the kernel, which sums
    in another order, is allowed K_DELTA = 4 times that."""
    for D, rank in ((20, abx_ref.RANK), (512, 0)):
        ref = abx_ref.cost_reference(D, rank=rank)
        c64, _, _, _, steps = ref["f64"]
        err = np.abs(ref["f32"][0].astype(np.float64) - c64) / (steps * ref["frame_err"])
        assert err.max() <= 1.0, (D, rank, err.max())
