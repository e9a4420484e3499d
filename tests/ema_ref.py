"""Restatements of the codebook update of ``VQEmbeddingEMA.forward`` in training mode (``model.py:136-145``), DESIGN.md 2.6.

``step_f32``  numpy, every step a separately rounded fp32 operation in exactly the order the HIP kernels keep.
``step_f64``  the same update in float64 with the fp32-rounded constants, taking the indices as given: the yardstick both the
              reference and this project are measured against.
Both take the rows ``x`` (N, 64), their code indices, the three buffers and return ``(ema_count, ema_weight, embedding)``; no
argument is modified.
"""
import numpy as np

CHUNK = 64
f32 = np.float32


def constants(decay: float, epsilon: float, n_emb: int):
    """(decay_f, omd_f, eps_f, meps_f): ``1 - decay`` and ``M * epsilon`` are formed in double, as Python forms them, then
    rounded once.  (``np.float32(1) - np.float32(0.999)`` is off by 1.3e-5 relative.)"""
    return f32(decay), f32(1.0 - decay), f32(epsilon), f32(n_emb * epsilon)


def tree_sum(parts):
    """Adjacent-pair tree over the leading axis: (0+1), (2+3), ..., an odd last one carried up, until one remains."""
    parts = list(parts)
    while len(parts) > 1:
        nxt = [parts[i] + parts[i + 1] for i in range(0, len(parts) - 1, 2)]
        if len(parts) & 1:
            nxt.append(parts[-1])
        parts = nxt
    return parts[0]


def code_sums_f32(x: np.ndarray, idx: np.ndarray, n_emb: int) -> np.ndarray:
    """dw[m] = sum of x[r] over idx[r] == m: 64-row chunks, ascending rows inside a chunk, chunk partials by ``tree_sum``."""
    x = np.ascontiguousarray(x, f32)
    idx = np.asarray(idx).reshape(-1)
    used = np.unique(idx)                                   # unused codes: every partial an exact zero
    slot = np.full(n_emb, -1, np.int64)
    slot[used] = np.arange(used.size)
    parts = []
    for c0 in range(0, x.shape[0], CHUNK):
        p = np.zeros((used.size, x.shape[1]), f32)
        for r in range(c0, min(c0 + CHUNK, x.shape[0])):
            p[slot[idx[r]]] += x[r]                         # one fp32 add per element, ascending r
        parts.append(p)
    dw = np.zeros((n_emb, x.shape[1]), f32)
    dw[used] = tree_sum(parts)
    return dw


def count_total_f32(count: np.ndarray) -> np.float32:
    """n = sum(count): part[l] = count[l] + count[64 + l] + ... in sequence, then the upper half onto the lower, 32 ... 1."""
    rows = np.ascontiguousarray(count, f32).reshape(-1, 64)
    part = rows[0].copy()
    for j in range(1, rows.shape[0]):
        part = part + rows[j]
    h = 32
    while h >= 1:
        part = part[:h] + part[h:2 * h]
        h //= 2
    return f32(part[0])


def step_f32(x, idx, ema_count, ema_weight, decay: float = 0.999, epsilon: float = 1e-5):
    n_emb = ema_count.shape[0]
    dec, omd, eps, meps = constants(decay, epsilon, n_emb)
    hist = np.bincount(np.asarray(idx).reshape(-1), minlength=n_emb).astype(f32)        # <= 2^24: exact
    count = dec * np.asarray(ema_count, f32) + omd * hist
    n = count_total_f32(count)
    count = (count + eps) / (n + meps) * n
    dw = code_sums_f32(x, idx, n_emb)
    weight = dec * np.asarray(ema_weight, f32) + omd * dw
    emb = weight / count[:, None]
    assert count.dtype == f32 and weight.dtype == f32 and emb.dtype == f32
    return count, weight, emb


def step_f64(x, idx, ema_count, ema_weight, decay: float = 0.999, epsilon: float = 1e-5):
    n_emb = ema_count.shape[0]
    dec, omd, eps, meps = (float(v) for v in constants(decay, epsilon, n_emb))
    idx = np.asarray(idx).reshape(-1)
    hist = np.bincount(idx, minlength=n_emb).astype(np.float64)
    count = dec * np.asarray(ema_count, np.float64) + omd * hist
    n = count.sum()
    count = (count + eps) / (n + meps) * n
    dw = np.zeros((n_emb, x.shape[1]), np.float64)
    np.add.at(dw, idx, np.asarray(x, np.float64))
    weight = dec * np.asarray(ema_weight, np.float64) + omd * dw
    return count, weight, weight / count[:, None]


def scaled_errors(got, want64):
    """The three errors the fixtures record and the tests bound: ``ema_count`` relative to its largest value, ``ema_weight`` and
    ``embedding`` per code relative to that code's largest |value| in float64 -- (count, weight, embedding), each the worst."""
    out = []
    for g, w in zip(got, want64):
        g = np.asarray(g, np.float64)
        scale = np.abs(w).max() if w.ndim == 1 else np.abs(w).max(axis=1, keepdims=True)
        err = np.abs(g - w) / np.where(scale > 0, scale, 1.0)
        out.append(float(err.max()))
    return tuple(out)


ULP2 = 2.0 * 2.0 ** -23          # 2 fp32 ulp of a value scaled to [1, 2)


def bound(ref_err: float) -> float:
    """max(4 x the reference's own recorded error against float64, 2 fp32 ulp)."""
    return max(4.0 * float(ref_err), ULP2)


# ------------------------------------------------------------------------------------------
# cases: inputs rebuilt from a seed (nothing but the seed travels): x = codebook[code] + noise
# ------------------------------------------------------------------------------------------
# name -> (n_emb, n_rows, usage, start); the five the fixtures tests/golden/ema_<name>.npz record from the reference
FIXTURE_CASES = {
    "m64_n160_warm": (64, 160, "uniform", "warm"),
    "m64_n4096_onecode": (64, 4096, "one", "warm"),
    "m512_n4096_every_zero": (512, 4096, "every", "zero"),
    "m512_n4096_warm": (512, 4096, "uniform", "warm"),
    "m1024_n4113_skewed": (1024, 4113, "skewed", "warm"),
}
NOISE = 0.05            # against a U(+-1.5) codebook in 64 dimensions: every row is far from a tie, so indices do not depend on the back end


def make_case(name: str, n_emb: int, n_rows: int, usage: str, start: str):
    """-> dict of fp32 / int64 numpy arrays: x (n_rows, 64), code (the intended index of every row), embedding, ema_count,
    ema_weight.  usage: uniform | one (code 5 owns every row) | every (code r mod n_emb, each used) | skewed (density ~ u^4).
    start: zero (a fresh module: ema_count 0, ema_weight = embedding) | warm (counts in [0.5, 20.5), weight = embedding * count)."""
    from vectorquantizedcpc_amd import synth
    u = lambda what, n: synth.uniform01(f"ema/{name}/{what}", n)
    emb = ((u("codebook", n_emb * 64) * 2.0 - 1.0) * 1.5).astype(f32).reshape(n_emb, 64)
    if usage == "uniform":
        code = np.minimum((u("code", n_rows) * n_emb).astype(np.int64), n_emb - 1)
    elif usage == "one":
        code = np.full(n_rows, 5, np.int64)
    elif usage == "every":
        code = np.arange(n_rows, dtype=np.int64) % n_emb
    elif usage == "skewed":
        code = np.minimum((u("code", n_rows) ** 4 * n_emb).astype(np.int64), n_emb - 1)
    else:
        raise ValueError(usage)
    x = (emb[code].astype(np.float64) + (u("noise", n_rows * 64).reshape(n_rows, 64) * 2.0 - 1.0) * NOISE).astype(f32)
    if start == "zero":
        count, weight = np.zeros(n_emb, f32), emb.copy()
    elif start == "warm":
        count = (u("count", n_emb) * 20.0 + 0.5).astype(f32)
        weight = emb * count[:, None]
    else:
        raise ValueError(start)
    return {"x": x, "code": code, "embedding": emb, "ema_count": count, "ema_weight": weight}
