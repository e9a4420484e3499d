"""Float64 reference of the ABX protocol of DESIGN.md 2.5 (plain numpy), with an fp32 restatement of the frame distance and
the DP from which the GPU tests take their tolerances.  It shares no code with ``vectorquantizedcpc_amd.abx``: the score is a
brute-force enumeration of every (A, B, X) triple over the items, without blocks, so it checks ``plan`` / ``aggregate`` too.

Frame distance: each frame is divided by its norm (a zero frame stays zero), then theta = 2 atan2(|u - v|, |u + v|) / pi --
the angular distance arccos(cos) / pi in a form that is well conditioned at cos -> +-1 and exactly 0 for equal frames.
DTW: C[i][j] = d[i][j] + min(C[i-1][j-1], C[i-1][j], C[i][j-1]), predecessor = the FIRST minimum in that order,
L[i][j] = L[pred] + 1, L[0][0] = 1; distance = C[-1][-1] / L[-1][-1].
"""
import numpy as np

from vectorquantizedcpc_amd import synth

INV_PI32 = np.float32(0.318309886183790672)


def normalise(frames, dtype=np.float64):
    f = np.asarray(frames).astype(dtype)
    n = np.sqrt((f * f).sum(axis=1, dtype=dtype)).astype(dtype)
    inv = np.where(n > 0, dtype(1.0) / np.where(n > 0, n, dtype(1.0)), dtype(0.0)).astype(dtype)
    return (f * inv[:, None]).astype(dtype)


def frame_dist(a, b, dtype=np.float64):
    """(Ta, Tb) frame distances between the frame runs ``a`` (Ta, D) and ``b`` (Tb, D), all arithmetic in ``dtype``
    (np.float64: the reference; np.float32: the restatement of what the kernel computes, in numpy's summation order)."""
    u, v = normalise(a, dtype)[:, None, :], normalise(b, dtype)[None, :, :]
    m, p = (u - v).astype(dtype), (u + v).astype(dtype)
    sd = (m * m).sum(axis=2, dtype=dtype)
    sp = (p * p).sum(axis=2, dtype=dtype)
    th = dtype(2.0) * np.arctan2(np.sqrt(sd), np.sqrt(sp)).astype(dtype)
    return (th * INV_PI32).astype(np.float32) if dtype == np.float32 else th / np.pi


def dtw(d):
    """One pair, in the dtype of ``d`` -> (cost, path_len, min_gap): ``min_gap`` = the smallest gap between the best and the
    second-best predecessor over the cells of the pair's own optimal path (inf where a cell has one predecessor)."""
    c, l, g = dtw_batch([np.asarray(d)])
    return c[0], int(l[0]), g[0]


def dtw_batch(ds):
    """The same for a list of (Ta, Tb) matrices of one dtype, vectorised over the pairs."""
    P = len(ds)
    dt = ds[0].dtype
    ta = np.array([d.shape[0] for d in ds]); tb = np.array([d.shape[1] for d in ds])
    A, B = int(ta.max()), int(tb.max())
    d = np.full((P, A, B), np.inf, dt)
    for k, m in enumerate(ds):
        d[k, :m.shape[0], :m.shape[1]] = m
    Cc = np.full((P, A + 1, B + 1), np.inf, dt)          # one row / column of inf in front
    Ll = np.zeros((P, A + 1, B + 1), np.int64)
    pred = np.zeros((P, A, B), np.int8)
    gap = np.full((P, A, B), np.inf, np.float64)
    for i in range(A):
        for j in range(B):
            if i == 0 and j == 0:
                Cc[:, 1, 1] = d[:, 0, 0]
                Ll[:, 1, 1] = 1
                continue
            cand = np.stack([Cc[:, i, j], Cc[:, i, j + 1], Cc[:, i + 1, j]], axis=1)         # diagonal, (i-1, j), (i, j-1)
            lens = np.stack([Ll[:, i, j], Ll[:, i, j + 1], Ll[:, i + 1, j]], axis=1)
            k = np.argmin(cand, axis=1)                                                     # first minimum
            best = cand[np.arange(P), k]
            rest = cand.astype(np.float64).copy()
            rest[np.arange(P), k] = np.inf
            with np.errstate(invalid="ignore"):
                gap[:, i, j] = np.where(np.isfinite(rest.min(axis=1)), rest.min(axis=1) - best.astype(np.float64), np.inf)
            pred[:, i, j] = k
            Cc[:, i + 1, j + 1] = (d[:, i, j] + best).astype(dt)
            Ll[:, i + 1, j + 1] = lens[np.arange(P), k] + 1
    cost = Cc[np.arange(P), ta, tb]
    plen = Ll[np.arange(P), ta, tb]
    mg = np.full(P, np.inf)
    for k in range(P):                                   # walk each pair's own path back
        i, j = ta[k] - 1, tb[k] - 1
        while i > 0 or j > 0:
            mg[k] = min(mg[k], gap[k, i, j])
            s = pred[k, i, j]
            i, j = (i - 1, j - 1) if s == 0 else ((i - 1, j) if s == 1 else (i, j - 1))
    return cost, plen, mg


def pair_table(frames, tokens, a_ids, x_ids, dtype=np.float64):
    """cost, path_len, dist, min_gap as (nA, nX) arrays for token lists over ``frames`` (n, D); ``tokens`` = (first, n)."""
    fr = np.asarray(frames)
    ds = []
    for a in a_ids:
        for x in x_ids:
            fa = fr[tokens[a][0]:tokens[a][0] + tokens[a][1]]
            fx = fr[tokens[x][0]:tokens[x][0] + tokens[x][1]]
            ds.append(frame_dist(fa, fx, dtype))
    c, l, g = dtw_batch(ds)
    shape = (len(a_ids), len(x_ids))
    c = c.reshape(shape)
    l = l.reshape(shape)
    dist = (c / l.astype(c.dtype)).astype(c.dtype)
    return c, l, dist, g.reshape(shape)


def max_frame_error(frames, tokens, a_ids, x_ids):
    """Largest |fp32 restatement - float64| over every frame distance of the pairs."""
    fr = np.asarray(frames)
    worst = 0.0
    for a in a_ids:
        fa = fr[tokens[a][0]:tokens[a][0] + tokens[a][1]]
        for x in x_ids:
            fx = fr[tokens[x][0]:tokens[x][0] + tokens[x][1]]
            worst = max(worst, float(np.abs(frame_dist(fa, fx, np.float32).astype(np.float64) - frame_dist(fa, fx)).max()))
    return worst


def twice_wins_of(dist, a_ids, seg, x_ids, x_seg):
    """The integer counts of DESIGN.md 2.5 from a (nA, nX) distance table -> (nX, n_seg) int64."""
    ns = len(seg) - 1
    out = np.zeros((len(x_ids), ns), np.int64)
    for xi, (x, p) in enumerate(zip(x_ids, x_seg)):
        rows = [r for r in range(seg[p], seg[p + 1]) if a_ids[r] != x]
        for q in range(ns):
            if q == p:
                continue
            for r in rows:
                db = dist[seg[q]:seg[q + 1], xi]
                out[xi, q] += 2 * int((dist[r, xi] < db).sum()) + int((dist[r, xi] == db).sum())
    return out


def all_pairs(frames, tokens, dtype=np.float64):
    """(n, n) distance table of every token against every token."""
    ids = list(range(len(tokens)))
    return pair_table(frames, tokens, ids, ids, dtype)[2]


def brute_force(items, D, mode, skip=None):
    """Every triple (a, b, x): a, b of one speaker s_ab and one context, phone(a) == phone(x) != phone(b), x of the same context,
    a != x, speaker(x) == s_ab (within) or != s_ab (across).  ``D[a, x]`` = token distances.  ``skip(a, b, x)`` -> True leaves a
    triple out.  -> (cells {(p, q, s_ab, s_x, context): (twice_wins, n)}, skipped)."""
    cells, skipped = {}, 0
    n = len(items)
    for x in range(n):
        ix = items[x]
        for a in range(n):
            ia = items[a]
            if a == x or ia.phone != ix.phone or (ia.prev, ia.next) != (ix.prev, ix.next):
                continue
            if (ia.speaker == ix.speaker) != (mode == "within"):
                continue
            for b in range(n):
                ib = items[b]
                if ib.speaker != ia.speaker or (ib.prev, ib.next) != (ia.prev, ia.next) or ib.phone == ia.phone:
                    continue
                if skip is not None and skip(a, b, x):
                    skipped += 1
                    continue
                key = (ia.phone, ib.phone, ia.speaker, ix.speaker, (ia.prev, ia.next))
                t, m = cells.get(key, (0, 0))
                cells[key] = (t + (2 if D[a, x] < D[b, x] else (1 if D[a, x] == D[b, x] else 0)), m + 1)
    return cells, skipped


def score_of(cells, mode):
    """The means of DESIGN.md 2.5 over the cells, written out level by level."""
    phones = sorted({(k[0], k[1]) for k in cells})
    pair_scores = []
    for p, q in phones:
        ab_scores = []
        for s_ab in sorted({k[2] for k in cells if k[:2] == (p, q)}):
            x_scores = []
            for s_x in sorted({k[3] for k in cells if k[:3] == (p, q, s_ab)}):
                ctx = [t / (2.0 * n) for k, (t, n) in cells.items() if k[:4] == (p, q, s_ab, s_x) and n > 0]
                if ctx:
                    x_scores.append(float(np.mean(ctx)))
            if x_scores:
                ab_scores.append(float(np.mean(x_scores)))
        if ab_scores:
            pair_scores.append(float(np.mean(ab_scores)))
    return float(np.mean(pair_scores)) if pair_scores else float("nan")


# ------------------------------------------------------------------------------------------------ seeded test sets
def item_set(name, speakers, contexts, phones, lo, hi, n_frames=400, lone_speaker=True, single_phone_context=True):
    """Seeded items over one file per speaker: per (speaker, context, phone) ``lo``..``hi`` tokens of 0.05-0.3 s, plus (asked
    for) a context that holds a single phone, which must drop out, and a speaker with one token."""
    from vectorquantizedcpc_amd.abx import Item
    u = synth.uniform01("abx/items/" + name, 8 * len(speakers) * len(contexts) * len(phones) * (hi + 1) + 64)
    k, items = 0, []
    dur = n_frames * 0.02
    for s in speakers:
        for c in contexts:
            for p in phones:
                cnt = lo + int(u[k] * (hi - lo + 1)); k += 1
                for _ in range(min(cnt, hi)):
                    on = u[k] * (dur - 0.5); ln = 0.05 + 0.25 * u[k + 1]; k += 2
                    items.append(Item("f_" + s, round(on, 4), round(on + ln, 4), p, c[0], c[1], s))
    if single_phone_context:
        for s in speakers[:2]:
            for _ in range(2):
                on = u[k] * (dur - 0.5); k += 1
                items.append(Item("f_" + s, round(on, 4), round(on + 0.1, 4), phones[0], "only", "one", s))
    if lone_speaker:
        items.append(Item("f_lone", 0.1, 0.22, phones[0], contexts[0][0], contexts[0][1], "lone"))
    return items


def features_for(items, D, name, n_frames=400, codebook=24):
    """file -> (n_frames, D) fp32: rows of a small seeded codebook (quantised: equal frames repeat)."""
    files = sorted({it.file for it in items})
    book = synth._normalish("abx/book/" + name, (codebook, D), synth.SEED).numpy()
    out = {}
    for f in files:
        idx = synth.randint("abx/codes/" + name + f, (n_frames,), codebook).numpy()
        out[f] = book[idx].astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the cost cases of the GPU tests
COST_DS = (4, 20, 64, 256, 512)
# token lengths: 0..5 the A side and 6..11 the X side of the pairs 1x1, 1x64, 64x1, 64x64, 3x17, 33x31; 12, 13 the special
# tokens; 14..19 and 20..26 short tokens of a dense block
COST_LENS = (1, 64, 3, 33, 64, 1, 1, 64, 17, 31, 64, 1, 6, 6, 2, 5, 7, 9, 12, 4, 3, 6, 8, 10, 11, 5, 2)
COST_BLOCKS = (([0], [6]), ([5], [7]), ([1], [11]), ([4], [10]), ([2], [8]), ([3], [9]),
               ([1, 2], [1, 2]),                        # a token against itself (and the other one)
               ([12], [13]),
               ([14, 15, 16, 17, 18, 19], [20, 21, 22, 23, 24, 25, 26]))
K_DELTA = 4.0                                          # delta = K_DELTA * the restatement's largest frame-distance error
RANK = 3
_cache = {}


def cost_case(D, seed=synth.SEED, rank=RANK):
    """-> frames (n, D) fp32, tokens.  Frames: normal-ish points of a ``rank``-dimensional subspace of R^D (every component is
    non-zero, the distances spread over [0, 1] at every D as they do between real units -- between independent points of R^512
    every distance is 0.5 +- 0.01 and every long pair has a near-tie somewhere on its path, which matters for the path
    lengths); ``rank`` 0: independent normal-ish components, full rank -- for the cost bound, which no tie touches.  Token 12 holds a frame twice in a
    row, a zero frame and g; token 13 holds the same frame, a zero frame and -g (antiparallel), and its last two frames are equal."""
    first = np.concatenate([[0], np.cumsum(COST_LENS)])
    if rank:
        pts = synth._normalish("abx/cost/pts/%d" % D, (int(first[-1]), rank), seed).numpy().astype(np.float64)
        mix = synth._normalish("abx/cost/mix/%d" % D, (rank, D), seed).numpy().astype(np.float64)
        f = (pts @ mix).astype(np.float32)
    else:
        f = synth._normalish("abx/cost/full/%d" % D, (int(first[-1]), D), seed).numpy().copy()
    a, x = int(first[12]), int(first[13])
    f[a + 1] = f[a]
    f[a + 2] = 0.0
    f[x] = f[a]
    f[x + 1] = 0.0
    f[x + 2] = -f[a + 3]
    f[x + 5] = f[x + 4]
    return f, [(int(first[k]), COST_LENS[k]) for k in range(len(COST_LENS))]


def block_tables(frames, tokens, blocks, dtype=np.float64):
    """cost, path_len, dist, min_gap, steps (= Ta + Tb - 1) of every pair of every (a_ids, x_ids) block, flat in the order
    of the device tables (block after block, each (nA, nX) row-major)."""
    parts = [pair_table(frames, tokens, a, x, dtype) + (steps_of(tokens, a, x),) for a, x in blocks]
    return tuple(np.concatenate([p[k].reshape(-1) for p in parts]) for k in range(5))


def cost_reference(D, seed=synth.SEED, rank=RANK):
    """The float64 tables, the fp32 restatement's tables and its largest frame-distance error for ``cost_case(D)``, computed once."""
    if (D, seed, rank) not in _cache:
        f, tokens = cost_case(D, seed, rank)
        err = max(max_frame_error(f, tokens, a, x) for a, x in COST_BLOCKS)
        _cache[(D, seed, rank)] = {"f64": block_tables(f, tokens, COST_BLOCKS), "f32": block_tables(f, tokens, COST_BLOCKS, np.float32),
                                   "frame_err": err}
    return _cache[(D, seed, rank)]


def steps_of(tokens, a_ids, x_ids):
    """(nA, nX) of Ta + Tb - 1: the cells of the longest path."""
    return np.array([[tokens[a][1] + tokens[x][1] - 1 for x in x_ids] for a in a_ids])


# ------------------------------------------------------------------------------------------------ end to end
def context_tables(items, frames, tokens, restate=False):
    """Token distances between every two items of one context (the only ones a triple can hold; nan elsewhere), float64:
    -> dict with ``dist``, ``plen``, ``steps`` (n, n), ``frame_err`` (largest fp32-restatement error of a frame distance) and,
    with ``restate``, ``dist32`` = the fp32 restatement's table."""
    n = len(items)
    out = {"dist": np.full((n, n), np.nan), "plen": np.zeros((n, n), np.int64), "steps": np.zeros((n, n), np.int64),
           "frame_err": 0.0}
    if restate:
        out["dist32"] = np.full((n, n), np.nan, np.float32)
    fr = np.asarray(frames)
    by = {}
    for k, it in enumerate(items):
        by.setdefault((it.prev, it.next), []).append(k)
    for ids in by.values():
        d64, d32 = [], []
        for a in ids:
            fa = fr[tokens[a][0]:tokens[a][0] + tokens[a][1]]
            for x in ids:
                fx = fr[tokens[x][0]:tokens[x][0] + tokens[x][1]]
                d64.append(frame_dist(fa, fx))
                d32.append(frame_dist(fa, fx, np.float32))
                out["frame_err"] = max(out["frame_err"], float(np.abs(d32[-1].astype(np.float64) - d64[-1]).max()))
        c, l, _ = dtw_batch(d64)
        ix = np.ix_(ids, ids)
        out["dist"][ix] = (c / l).reshape(len(ids), len(ids))
        out["plen"][ix] = l.reshape(len(ids), len(ids))
        out["steps"][ix] = steps_of(tokens, ids, ids)
        if restate:
            c, l, _ = dtw_batch(d32)
            out["dist32"][ix] = (c / l.astype(np.float32)).reshape(len(ids), len(ids))
    return out


def near_tie(ref, delta):
    """skip(a, b, x) for ``brute_force``: float64's own |d(a, x) - d(b, x)| is below what the cost bound (Ta + Tb - 1) delta of
    either pair, divided by its path length, allows."""
    tol = ref["steps"] * delta / np.maximum(ref["plen"], 1)
    D = ref["dist"]
    return lambda a, b, x: abs(D[a, x] - D[b, x]) < tol[a, x] + tol[b, x]


E2E_SETS = {
    "small": dict(speakers=["s0", "s1", "s2"], contexts=[("a", "b"), ("c", "d"), ("e", "f")], phones=["p0", "p1", "p2", "p3"], lo=1, hi=3),
    "200": dict(speakers=["s0", "s1", "s2", "s3"], contexts=[("a", "b"), ("c", "d"), ("e", "f")], phones=["p0", "p1", "p2", "p3"], lo=3, hi=5),
}


def e2e_set(name, D=8):
    """items, features by file, flat frames, tokens (rows of the flat frames) of a seeded set."""
    from vectorquantizedcpc_amd import abx
    k = E2E_SETS[name]
    items = item_set(name, k["speakers"], k["contexts"], k["phones"], k["lo"], k["hi"])
    feats = features_for(items, D, name)
    files = sorted(feats)
    first = np.cumsum([0] + [feats[f].shape[0] for f in files])
    tok = abx.tokens_of(items, {f: feats[f].shape[0] for f in files})
    tokens = [(int(first[files.index(it.file)]) + lo, n) for it, (lo, n) in zip(items, tok)]
    return items, feats, np.concatenate([feats[f] for f in files]), tokens


def e2e_reference(name):
    """``e2e_set(name)`` with its float64 tables, computed once: -> (items, feats, frames, tokens, tables)."""
    if ("e2e", name) not in _cache:
        items, feats, frames, tokens = e2e_set(name)
        _cache[("e2e", name)] = (items, feats, frames, tokens, context_tables(items, frames, tokens))
    return _cache[("e2e", name)]
