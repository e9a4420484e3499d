"""The index form of ABX scoring, the parts that need no GPU: the numpy edit-distance reference of tests/abx_index_ref.py
against the recursion and known values, plan + aggregate on its counts against the brute-force enumeration, the builders, and
the no-fallback rule of the new entry points."""
import numpy as np
import pytest
import torch

import abx_index_ref as R
import abx_ref
from vectorquantizedcpc_amd import _lib, abx

RUNS = [[0], [5], [0, 0], [0, 1], [1, 0, 1], [2, 2, 2, 2], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [1, 1, 2, 3, 3, 3, 0],
        [7, 0, 1, 2, 3, 4, 9, 9], list(range(10, 20))]


def test_numpy_edit_distance_equals_the_recursion():
    for a in RUNS:
        for b in RUNS:
            assert R.levenshtein(a, b) == R.levenshtein_recursive(a, b), (a, b)


def test_known_values():
    for a in RUNS:
        assert R.levenshtein(a, a) == 0 and R.edit_dist(a, a) == 0.0
    for m in (1, 2, 5, 9):
        for n in (1, 3, 9, 64):
            assert R.levenshtein(range(m), range(100, 100 + n)) == max(m, n)          # disjoint alphabets
            assert R.edit_dist(range(m), range(100, 100 + n)) == 1.0
    kitten, sitting = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert R.levenshtein(kitten, sitting) == 3
    assert R.edit_dist(kitten, sitting) == np.float32(3.0) / np.float32(7.0)
    assert R.levenshtein([1, 2, 3], [1, 3]) == 1 and R.levenshtein([1, 2, 2, 2], [1, 2]) == 2      # repeats are not collapsed
    # equal ratios have equal bits (what the count kernel's tie term relies on)
    assert np.float32(1.0) / np.float32(2.0) == np.float32(2.0) / np.float32(4.0) == np.float32(32.0) / np.float32(64.0)
    assert (np.float32(3.0) / np.float32(9.0)).view(np.uint32) == (np.float32(7.0) / np.float32(21.0)).view(np.uint32)


def test_reference_is_symmetric_and_within_0_1():
    for a in RUNS:
        for b in RUNS:
            d = R.edit_dist(a, b)
            assert d == R.edit_dist(b, a) and 0.0 <= d <= 1.0 and d.dtype == np.float32
            assert (d == 0.0) == (list(a) == list(b))
    codes, tokens = R.cost_codes(24)
    c, l, d = R.edit_pair_table(codes, tokens, list(range(12, 27)), list(range(12, 27)))
    assert np.array_equal(c, c.T) and np.array_equal(d, d.T) and (d >= 0).all() and (d <= 1).all() and (np.diag(c) == 0).all()
    assert (c >= np.abs(np.subtract.outer([tokens[k][1] for k in range(12, 27)], [tokens[k][1] for k in range(12, 27)]))).all()
    assert (c <= l).all()


@pytest.mark.parametrize("mode", ["within", "across"])
def test_plan_and_aggregate_on_edit_counts_equal_brute_force(mode):
    items, _, _, codes, tokens, D = R.e2e_edit_reference("small")
    pl = abx.plan(items, mode)
    assert pl.blocks
    tw = [abx_ref.twice_wins_of(D[np.ix_(b.a, b.x)], b.a, b.seg, b.x, b.x_seg).reshape(-1) for b in pl.blocks]
    res = abx.aggregate(pl, np.concatenate(tw))
    want, _ = abx_ref.brute_force(items, D, mode)
    assert res["cells"] == want                                       # every cell's (twice_wins, n)
    assert res["n_triples"] == sum(n for _, n in want.values()) > 0
    assert abs(res["score"] - abx_ref.score_of(want, mode)) < 1e-12
    assert sum(int((t % 2).sum()) for t in tw) > 0                    # small integers over small lengths: exact ties are common


def test_builders():
    for M, D in ((24, 20), (513, 64), (7, 512)):
        book = R.codebook(M, D)
        assert not book[R.ZERO_ROW].any() and np.array_equal(book[R.TWIN_ROWS[0]], book[R.TWIN_ROWS[1]])
        assert np.array_equal(book[R.NEG_ROWS[1]], -book[R.NEG_ROWS[0]]) and book[R.NEG_ROWS[0]].all()
        codes, tokens = R.cost_codes(M)
        assert codes.min() >= 0 and codes.max() < min(M, R.POOL) and len(tokens) == len(abx_ref.COST_LENS)
        for f, n in tokens:
            assert n < 3 or len(set(codes[f:f + n].tolist())) < n      # a repeated code in every token of 3 or more frames
        assert set(range(1, 6)) <= set(codes[tokens[12][0]:tokens[13][0] + tokens[13][1]].tolist())
    assert R.codebook(1, 8).shape == (1, 8) and not R.cost_codes(1)[0].any()
    items, book, idx, codes, tokens = R.e2e_indices("small")           # asserts book[idx] == abx_ref.features_for(..)
    assert codes.shape == (400 * len(idx),) and len(tokens) == len(items)


def test_index_entry_points_are_declared_and_have_no_cpu_fallback():
    for name in ("vqcpc_abx_index_workspace_bytes", "vqcpc_abx_code_table", "vqcpc_abx_score_indices"):
        assert name in _lib.SYMBOLS and hasattr(_lib.load(), name)
    blk = [abx.Block([0], [0, 1], [1], [0])]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        abx.code_table(torch.zeros(24, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        abx.pair_distances_indices(torch.zeros(100, dtype=torch.int64), [(0, 2), (2, 2)], blk, n_codes=24, metric="edit")
    items = [abx.Item("f", 0.0, 0.1, "p", "a", "b", "s")]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        abx.score_indices(None, {"f": torch.zeros(100, dtype=torch.int64)}, items, metric="edit")
    with pytest.raises(ValueError, match="metric"):
        abx.score_indices(None, {"f": torch.zeros(100, dtype=torch.int64)}, items, metric="kl")
