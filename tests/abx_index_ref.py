"""Reference and builders for the index form of ABX scoring: a numpy Levenshtein distance with the tables the
GPU tests compare against bit for bit, seeded codebooks with the special rows, index runs on the geometry of
``abx_ref.COST_LENS`` / ``COST_BLOCKS``, and the indices behind ``abx_ref.features_for``.  Shares no code with
``vectorquantizedcpc_amd.abx``."""
import functools

import numpy as np

import abx_ref
from vectorquantizedcpc_amd import synth

ZERO_ROW, TWIN_ROWS, NEG_ROWS = 1, (2, 3), (4, 5)      # codebook(): row 1 is 0, rows 2 and 3 are bit-equal, row 5 = -row 4
POOL = 24                                              # codes are drawn from the first POOL rows, so they repeat


def levenshtein(a, b):
    """E(len(a), len(b)) of E(0, 0) = 0, E(i, 0) = i, E(0, j) = j, E(i, j) = min(E(i-1, j-1) + [a_i != b_j], E(i-1, j) + 1,
    E(i, j-1) + 1), row by row: the minimum over the two candidates from the row above, then the chain of left neighbours as
    a running minimum of row[j] - j."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    j = np.arange(len(b) + 1)
    row = j.copy()
    for i in range(1, len(a) + 1):
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[:-1] + (b != a[i - 1]), row[1:] + 1)
        row = np.minimum.accumulate(new - j) + j
    return int(row[-1])


def levenshtein_recursive(a, b):
    """The definition, written as the recursion over prefixes."""
    a, b = tuple(int(v) for v in a), tuple(int(v) for v in b)

    @functools.lru_cache(maxsize=None)
    def e(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(e(i - 1, j - 1) + (a[i - 1] != b[j - 1]), e(i - 1, j) + 1, e(i, j - 1) + 1)
    return e(len(a), len(b))


def edit_dist(a, b):
    """The normalised distance as the kernel defines it: fp32(E) / fp32(max(len))."""
    return np.float32(levenshtein(a, b)) / np.float32(max(len(a), len(b)))


_memo = {}


def edit_pair_table(codes, tokens, a_ids, x_ids):
    """cost (fp32), path_len (int64), dist (fp32) as (nA, nX) arrays for token lists over the index run ``codes``."""
    codes = np.asarray(codes)
    run = lambda t: tuple(int(v) for v in codes[tokens[t][0]:tokens[t][0] + tokens[t][1]])
    cost = np.zeros((len(a_ids), len(x_ids)), np.float32)
    plen = np.zeros((len(a_ids), len(x_ids)), np.int64)
    for i, a in enumerate(a_ids):
        ra = run(a)
        for j, x in enumerate(x_ids):
            rx = run(x)
            if (ra, rx) not in _memo:
                _memo[(ra, rx)] = levenshtein(ra, rx)
            cost[i, j] = _memo[(ra, rx)]
            plen[i, j] = max(len(ra), len(rx))
    return cost, plen, (cost / plen.astype(np.float32)).astype(np.float32)


def edit_block_tables(codes, tokens, blocks):
    """cost, path_len, dist of every pair of every (a_ids, x_ids) block, flat in the order of the device tables."""
    parts = [edit_pair_table(codes, tokens, a, x) for a, x in blocks]
    return tuple(np.concatenate([p[k].reshape(-1) for p in parts]) for k in range(3))


def edit_context_table(items, codes, tokens):
    """(n, n) fp32 edit distances between every two items of one context (nan elsewhere), computed once per set."""
    n = len(items)
    D = np.full((n, n), np.nan, np.float32)
    by = {}
    for k, it in enumerate(items):
        by.setdefault((it.prev, it.next), []).append(k)
    for ids in by.values():
        D[np.ix_(ids, ids)] = edit_pair_table(codes, tokens, ids, ids)[2]
    return D


# ------------------------------------------------------------------------------------------------ codebooks and index runs
def codebook(M, D):
    """(M, D) fp32, seeded, every component non-zero; with at least 6 rows: one all-zero row, two bit-equal rows and one row
    that is the negative of another (ZERO_ROW, TWIN_ROWS, NEG_ROWS)."""
    book = synth._normalish("abx/index/book/%d/%d" % (M, D), (M, D), synth.SEED).numpy().astype(np.float32).copy()
    if M >= 6:
        book[ZERO_ROW] = 0.0
        book[TWIN_ROWS[1]] = book[TWIN_ROWS[0]]
        book[NEG_ROWS[1]] = -book[NEG_ROWS[0]]
    return book


def cost_codes(M):
    """Index runs on the geometry of ``abx_ref.COST_LENS``: -> codes (n,) int64 drawn from the first min(M, POOL) rows, tokens.
    Every token of 3 or more frames holds a code twice (its second frame is made a copy of its first where the draw has no
    repeat).  With the special rows (M >= 6): token 12 = twin, twin, zero, g, ...; token 13 = the other twin, zero, -g, ...:
    the pair (12, 13) of COST_BLOCKS meets bit-equal rows under two indices, the zero row and the antiparallel pair."""
    lens = abx_ref.COST_LENS
    first = np.concatenate([[0], np.cumsum(lens)])
    codes = synth.randint("abx/index/codes/%d" % M, (int(first[-1]),), min(M, POOL)).numpy().astype(np.int64)
    if M >= 6:
        a, x = int(first[12]), int(first[13])
        codes[a:a + 4] = [TWIN_ROWS[0], TWIN_ROWS[0], ZERO_ROW, NEG_ROWS[0]]
        codes[x:x + 3] = [TWIN_ROWS[1], ZERO_ROW, NEG_ROWS[1]]
    for k, n in enumerate(lens):
        run = codes[first[k]:first[k] + n]
        if n >= 3 and len(set(run.tolist())) == n:
            run[1] = run[0]
    return codes, [(int(first[k]), lens[k]) for k in range(len(lens))]


def geometry_case():
    """Short tokens (1..8 frames) over 600 indices into a 24-row codebook of D = 20, and (a_ids, x_ids) blocks of every shape
    the launch geometry has: nA = nX = 1, 37 x 5, 5 x 37, a list against itself, and 300 mixed blocks."""
    n = 600
    codes = synth.randint("abx/index/geo/codes", (n,), POOL).numpy().astype(np.int64)
    lens = 1 + synth.randint("abx/index/geo/len", (120,), 8).numpy()
    first = synth.randint("abx/index/geo/first", (120,), n - 8).numpy()
    tokens = [(int(f), int(l)) for f, l in zip(first, lens)]
    ids = lambda name, k: [int(v) for v in synth.randint("abx/index/geo/" + name, (k,), 120).numpy()]
    pairs = [([3], [7]), (ids("a37", 37), ids("x5", 5)), (ids("a5", 5), ids("x37", 37))]
    within = ids("w", 9)
    pairs.append((within, within))
    na = 1 + synth.randint("abx/index/geo/na", (300,), 6).numpy()
    nx = 1 + synth.randint("abx/index/geo/nx", (300,), 5).numpy()
    for b in range(300):
        pairs.append((ids("ma%d" % b, int(na[b])), ids("mx%d" % b, int(nx[b]))))
    return codebook(POOL, 20), codes, tokens, pairs


def e2e_indices(name, D=8, n_frames=400, n_codes=24):
    """The codebook and the per-file indices behind ``abx_ref.features_for(items, D, name)``: its two ``synth`` calls, restated,
    so that ``book[idx[f]]`` is that file's feature array.  -> items, book (n_codes, D) fp32, idx by file, flat codes, tokens."""
    items, feats, _, tokens = abx_ref.e2e_set(name, D)
    book = synth._normalish("abx/book/" + name, (n_codes, D), synth.SEED).numpy().astype(np.float32)
    idx = {f: synth.randint("abx/codes/" + name + f, (n_frames,), n_codes).numpy().astype(np.int64) for f in sorted(feats)}
    for f in idx:
        assert np.array_equal(book[idx[f]].view(np.uint32), feats[f].view(np.uint32)), f
    return items, book, idx, np.concatenate([idx[f] for f in sorted(idx)]), tokens


def e2e_edit_reference(name):
    """``e2e_indices(name)`` with the reference's edit-distance table between the items of each context, computed once."""
    if ("edit", name) not in abx_ref._cache:
        items, book, idx, codes, tokens = e2e_indices(name)
        abx_ref._cache[("edit", name)] = (items, book, idx, codes, tokens, edit_context_table(items, codes, tokens))
    return abx_ref._cache[("edit", name)]
