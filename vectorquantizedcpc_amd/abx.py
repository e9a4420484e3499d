"""ABX scoring of encoded units on MI355X -- the project's OWN protocol (``DESIGN.md`` 2.5, parity unpinned).

The reference judges a checkpoint's units by an outside package: README 4-B "Run ABX evaluation script" over the text files
``encode.py:48-52`` writes.  This module does that step in-process: tokens (runs of frames) from an items file, dense blocks of
(context, A/B speaker, X speaker), batched DTW over angular frame distances and the integer ABX counts in one three-launch HIP
call (``csrc/abx.hip``), and the score as a mean over contexts, speakers and ordered phone pairs.  No equality with any outside
tool is claimed.

The units are discrete, so the same protocol also takes them as codebook INDICES (``code_table``, ``pair_distances_indices``,
``score_indices``): every frame distance of a call is one of ``M x M`` table entries with the bits the frames would give, or,
with ``metric="edit"``, the tokens are compared by the Levenshtein distance of their index runs.

Pure-host parts (no GPU): ``read_items``, ``tokens_of``, ``plan``, ``aggregate``.  Device parts: ``pair_distances``, ``score``,
``code_table``, ``pair_distances_indices``, ``score_indices`` (no CPU fallback).
"""
import ctypes as C
from collections import namedtuple
from typing import Dict, List, Sequence

import numpy as np

from . import _lib

T_MAX = 64                       # frames per token (csrc/abx.hip)
A_TILE = 4                       # A tokens per workgroup of the DTW launch (csrc/abx.hip: ABX_AT)
# frame j of a file is at frame_offset + j * frame_shift seconds: the 10 ms mel hop (preprocess.py: hop_length 160 at 16 kHz)
# halved in rate by the encoder's Conv1d(k=4, s=2, p=1) (model.py:43)
FRAME_SHIFT = 0.02
FRAME_OFFSET = 0.01
M_MAX = 4096                     # codebook rows of the index form (include/vqcpc.h)
METRICS = {"angular": 0, "edit": 1}   # VQCPC_ABX_ANGULAR, VQCPC_ABX_EDIT

Item = namedtuple("Item", "file onset offset phone prev next speaker")


class Block:
    """One dense block: ``a`` token ids sorted by phone with ``seg`` offsets (len(phones) + 1), ``x`` token ids with ``x_seg`` =
    the segment of each X token's own phone; ``context``, ``s_ab``, ``s_x``, ``phones`` name what it stands for."""

    def __init__(self, a, seg, x, x_seg, context=None, s_ab=None, s_x=None, phones=None):
        self.a, self.seg, self.x, self.x_seg = list(a), list(seg), list(x), list(x_seg)
        self.context, self.s_ab, self.s_x = context, s_ab, s_x
        self.phones = list(phones) if phones is not None else list(range(len(self.seg) - 1))

    @property
    def n_seg(self):
        return len(self.seg) - 1

    def n_triples(self):
        """(nX, n_seg) int64: triples behind every count -- (|segment p| - [x is in it]) * |segment q|, 0 for q == p."""
        size = np.diff(np.asarray(self.seg, np.int64))
        own = np.zeros(len(self.x), np.int64)
        pos = {}
        for s in range(self.n_seg):
            for t in self.a[self.seg[s]:self.seg[s + 1]]:
                pos[t] = s
        for k, (t, s) in enumerate(zip(self.x, self.x_seg)):
            own[k] = size[s] - (1 if pos.get(t) == s else 0)
        n = own[:, None] * size[None, :]
        n[np.arange(len(self.x)), np.asarray(self.x_seg, np.int64)] = 0
        return n


def read_items(path) -> List[Item]:
    """Items file: one header line starting with ``#``, then ``file onset offset phone prev next speaker`` per line, split on
    whitespace, times in seconds."""
    items = []
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or not lines[0].startswith("#"):
        raise ValueError(f"{path}: the first line must be a header starting with '#'")
    for n, line in enumerate(lines[1:], 2):
        if not line.strip():
            continue
        p = line.split()
        if len(p) != 7:
            raise ValueError(f"{path}:{n}: expected 7 fields (file onset offset phone prev next speaker), got {len(p)}")
        items.append(Item(p[0], float(p[1]), float(p[2]), p[3], p[4], p[5], p[6]))
    return items


def tokens_of(items: Sequence[Item], n_frames_by_file: Dict[str, int], frame_shift: float = FRAME_SHIFT,
              frame_offset: float = FRAME_OFFSET):
    """Per item ``(first_frame, n_frames)`` inside its file: the frames with ``onset <= frame_offset + j * frame_shift <= offset``;
    an item that would be empty takes the one frame nearest its midpoint; an item longer than ``T_MAX`` frames is an error."""
    out = []
    for it in items:
        if it.file not in n_frames_by_file:
            raise KeyError(f"item {it.file} {it.onset} {it.offset} {it.phone}: no features for file {it.file!r}")
        n = int(n_frames_by_file[it.file])
        if n < 1:
            raise ValueError(f"file {it.file!r} has no frames")
        lo = int(np.ceil((it.onset - frame_offset) / frame_shift - 1e-9))
        hi = int(np.floor((it.offset - frame_offset) / frame_shift + 1e-9))
        lo, hi = max(lo, 0), min(hi, n - 1)
        if hi < lo:
            mid = 0.5 * (it.onset + it.offset)
            lo = hi = min(max(int(np.floor((mid - frame_offset) / frame_shift + 0.5)), 0), n - 1)
        if hi - lo + 1 > T_MAX:
            raise ValueError(f"item {it.file} {it.onset} {it.offset} {it.phone}: {hi - lo + 1} frames, more than T_MAX = {T_MAX}")
        out.append((lo, hi - lo + 1))
    return out


class Plan:
    def __init__(self, mode, items, blocks):
        self.mode, self.items, self.blocks = mode, list(items), blocks

    @property
    def n_pairs(self):
        return sum(len(b.a) * len(b.x) for b in self.blocks)

    @property
    def n_out(self):
        return sum(len(b.x) * b.n_seg for b in self.blocks)


def plan(items: Sequence[Item], mode: str = "within") -> Plan:
    """The dense blocks of ``mode`` ("within": X from the A/B speaker, "across": X from another speaker): one per (context, A/B
    speaker, X speaker), A/B tokens sorted by phone; token ids are positions in ``items``.  X tokens that no triple can hold
    (no other A of their phone) are left out of a block, and a block with no (p, q) triple is dropped."""
    if mode not in ("within", "across"):
        raise ValueError(f"mode must be 'within' or 'across', got {mode!r}")
    by = {}
    for k, it in enumerate(items):
        by.setdefault((it.prev, it.next), {}).setdefault(it.speaker, []).append(k)
    blocks = []
    for ctx in sorted(by):
        spk = by[ctx]
        for s_ab in sorted(spk):
            a = sorted(spk[s_ab], key=lambda k: (items[k].phone, k))
            phones, seg = [], []
            for pos, k in enumerate(a):
                if not phones or items[k].phone != phones[-1]:
                    phones.append(items[k].phone)
                    seg.append(pos)
            seg.append(len(a))
            if len(phones) < 2:
                continue
            size = {p: seg[s + 1] - seg[s] for s, p in enumerate(phones)}
            for s_x in ([s_ab] if mode == "within" else [s for s in sorted(spk) if s != s_ab]):
                need = 2 if mode == "within" else 1
                x = [k for k in sorted(spk[s_x], key=lambda k: (items[k].phone, k)) if size.get(items[k].phone, 0) >= need]
                if x:
                    blocks.append(Block(a, seg, x, [phones.index(items[k].phone) for k in x], ctx, s_ab, s_x, phones))
    return Plan(mode, items, blocks)


def aggregate(pl: Plan, twice_wins) -> dict:
    """``twice_wins``: the blocks' (nX, n_seg) int tables, flat, in plan order.  Cell (p, q, s_ab, s_x, context) = (sum of
    twice_wins, sum of triples); score = sum / (2 n) per cell, mean over contexts, then over speakers (across: over s_x, then
    over s_ab), then over the ordered phone pairs.  Cells without a triple are in no mean."""
    tw = np.asarray(twice_wins, np.int64).reshape(-1)
    if tw.size != pl.n_out:
        raise ValueError(f"twice_wins has {tw.size} entries, the plan's blocks have {pl.n_out}")
    cells, base = {}, 0
    for b in pl.blocks:
        nx, ns = len(b.x), b.n_seg
        t = tw[base:base + nx * ns].reshape(nx, ns)
        n = b.n_triples()
        base += nx * ns
        for s in sorted(set(b.x_seg)):
            rows = np.asarray(b.x_seg) == s
            for q in range(ns):
                nn = int(n[rows, q].sum())
                if q != s and nn > 0:
                    key = (b.phones[s], b.phones[q], b.s_ab, b.s_x, b.context)
                    old = cells.get(key, (0, 0))
                    cells[key] = (old[0] + int(t[rows, q].sum()), old[1] + nn)
    over_ctx = {}
    for (p, q, s_ab, s_x, _), (t, n) in cells.items():
        over_ctx.setdefault((p, q, s_ab, s_x), []).append(t / (2.0 * n))
    over_x = {}
    for (p, q, s_ab, _), v in sorted(over_ctx.items()):
        over_x.setdefault((p, q, s_ab), []).append(float(np.mean(v)))
    over_ab = {}
    for (p, q, _), v in sorted(over_x.items()):
        over_ab.setdefault((p, q), []).append(float(np.mean(v)))
    by_pair = {k: float(np.mean(v)) for k, v in sorted(over_ab.items())}
    n_triples = sum(n for _, n in cells.values())
    score = float(np.mean(list(by_pair.values()))) if by_pair else float("nan")
    return {"score": score, "error_rate": 100.0 * (1.0 - score), "n_triples": n_triples, "n_pairs": pl.n_pairs,
            "by_phone_pair": by_pair, "cells": cells}


# ------------------------------------------------------------------------------------------------ device part
BLOCK_WORDS = 12                 # ints per row of the block table (include/vqcpc.h)
BYTES_PER_PAIR = 4               # the distance table, fp32 (cost and path length are not kept by score)
BYTES_PER_COUNT = 4              # twice_wins, int32
BYTES_PER_LIST_ENTRY = 4         # token ids of the A/B and X lists, X segments, segment offsets: int32


def block_bytes(b: Block) -> int:
    """Device bytes one block adds to a call: its (nA, nX) distance table, its (nX, n_seg) counts and its rows of the tables."""
    return (len(b.a) * len(b.x) * BYTES_PER_PAIR + len(b.x) * b.n_seg * BYTES_PER_COUNT
            + (len(b.a) + 2 * len(b.x) + b.n_seg + 1 + BLOCK_WORDS) * BYTES_PER_LIST_ENTRY)


def block_chunks(blocks: Sequence[Block], mem_budget_bytes: int) -> List[List[int]]:
    """Block ids, in order, cut into calls whose per-block tables stay under ``mem_budget_bytes`` (at least one block per call),
    as ``driver.decode_chunks`` cuts decode calls.  The budget covers what grows with the blocks (``block_bytes``); every call
    also holds the frames, their normalised work copy (``n_frames * D * 4`` bytes each) and the token table, and normalises
    the frames again: a budget so small that it makes many calls pays that once per call."""
    chunks, cur, used = [], [], 0
    for i, b in enumerate(blocks):
        need = block_bytes(b)
        if cur and used + need > mem_budget_bytes:
            chunks.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += need
    if cur:
        chunks.append(cur)
    return chunks


def _tables(tokens, blocks, n_frames):
    """Validate and flatten: -> (tokens (n, 2) int32, lists, segs, block table (n_blocks, 12), n_workgroups, n_dist, n_out)."""
    tok = np.ascontiguousarray(np.asarray(tokens, dtype=np.int64).reshape(-1, 2))
    if tok.shape[0] < 1 or not blocks:
        raise ValueError("abx: need at least one token and one block")
    if (tok[:, 1] < 1).any() or (tok[:, 1] > T_MAX).any():
        k = int(np.nonzero((tok[:, 1] < 1) | (tok[:, 1] > T_MAX))[0][0])
        raise ValueError(f"abx: token {k} has {int(tok[k, 1])} frames, supported 1..{T_MAX}")
    if (tok[:, 0] < 0).any() or (tok[:, 0] + tok[:, 1] > n_frames).any():
        k = int(np.nonzero((tok[:, 0] < 0) | (tok[:, 0] + tok[:, 1] > n_frames))[0][0])
        raise IndexError(f"abx: token {k} covers rows {int(tok[k, 0])}..{int(tok[k, 0] + tok[k, 1]) - 1} of {n_frames} frames")
    lists, segs, rows = [], [], []
    wg = nd = no = 0
    for i, b in enumerate(blocks):
        ids = np.asarray(list(b.a) + list(b.x), np.int64)
        if len(b.a) < 1 or len(b.x) < 1 or b.n_seg < 1:
            raise ValueError(f"abx: block {i} is empty")
        if (ids < 0).any() or (ids >= tok.shape[0]).any():
            raise IndexError(f"abx: block {i} names a token outside [0, {tok.shape[0]})")
        sg = np.asarray(b.seg, np.int64)
        if sg[0] != 0 or sg[-1] != len(b.a) or (np.diff(sg) < 0).any():
            raise ValueError(f"abx: block {i}: segment offsets must ascend from 0 to nA = {len(b.a)}")
        xs = np.asarray(b.x_seg, np.int64)
        if len(xs) != len(b.x) or (xs < 0).any() or (xs >= b.n_seg).any():
            raise IndexError(f"abx: block {i}: x_seg must name one segment in [0, {b.n_seg}) per X token")
        if 2 * len(b.a) ** 2 >= 1 << 31:
            raise ValueError(f"abx: block {i}: nA = {len(b.a)} overflows the int32 counts")
        a_off = len(lists); lists += list(b.a)
        x_off = len(lists); lists += list(b.x)
        xs_off = len(lists); lists += list(b.x_seg)
        rows.append([a_off, len(b.a), x_off, len(b.x), len(segs), b.n_seg, nd, no, xs_off, wg, 0, 0])
        segs += list(b.seg)
        wg += len(b.x) * (-(-len(b.a) // A_TILE))
        nd += len(b.a) * len(b.x)
        no += len(b.x) * b.n_seg
    if max(wg, nd, no) >= 1 << 31:
        raise ValueError(f"abx: {nd} pairs / {no} counts / {wg} workgroups in one call: cut the blocks into chunks (block_chunks)")
    if len(segs) < 2:
        segs = segs + [0]
    return (tok.astype(np.int32), np.asarray(lists, np.int32), np.asarray(segs, np.int32), np.asarray(rows, np.int32).reshape(-1, BLOCK_WORDS),
            wg, nd, no)


PairTables = namedtuple("PairTables", "cost path_len dist twice_wins dist_base out_base")


def pair_distances(feats, tokens, blocks: Sequence[Block], want_cost: bool = True) -> PairTables:
    """The three-launch call on ``feats`` (n_frames, D) fp32 on the device, ``tokens`` (n_tokens, 2) int (first_row, n_frames)
    and dense ``blocks`` -> device tensors ``cost`` / ``path_len`` (None unless ``want_cost``), ``dist`` (flat, block after block,
    each (nA, nX) row-major from ``dist_base[i]``) and ``twice_wins`` (each (nX, n_seg) from ``out_base[i]``).  Does not
    synchronise.  Raises before the call on anything the kernels would have to clamp."""
    import torch
    if not isinstance(feats, torch.Tensor):
        raise TypeError("abx.pair_distances: feats must be a torch tensor on the device")
    _lib.require_cuda(feats, "abx features")
    if feats.dim() != 2 or feats.dtype != torch.float32:
        raise ValueError(f"abx: feats must be (n_frames, D) float32, got {tuple(feats.shape)} {feats.dtype}")
    n_frames, D = int(feats.shape[0]), int(feats.shape[1])
    if D % 4 or not 4 <= D <= 512:
        raise ValueError(f"abx: D = {D}, supported: a multiple of 4 in [4, 512]")
    if n_frames < 1:
        raise ValueError("abx: no frames")
    feats = feats.contiguous()
    work = torch.empty(n_frames * D, dtype=torch.float32, device=feats.device)
    lib = _lib.load()
    return _enqueue(feats.device, tokens, blocks, n_frames, want_cost, (feats, work),
                    lambda t, n, out, stream: lib.vqcpc_abx_score(feats.data_ptr(), n_frames, D, *t, *n, work.data_ptr(), *out, stream))


def _enqueue(dev, tokens, blocks, n_frames, want_cost, borrowed, call) -> PairTables:
    """What every pair call shares: ``_tables``, one upload of all four tables, the outputs, ``call(tables, counts, outputs,
    stream)`` with the arguments in the C ABI's order, and ``record_stream`` on what the enqueued work borrows."""
    import torch
    tok, lists, segs, rows, wg, nd, no = _tables(tokens, blocks, n_frames)
    with _lib.device_guard(dev):
        flat = np.concatenate([tok.reshape(-1), lists, segs, rows.reshape(-1)])
        # through pinned memory: a copy from pageable memory ends in a stream synchronisation, and these calls promise none
        # (torch's host allocator keeps the pinned block until the copy has run)
        d = torch.from_numpy(flat).pin_memory().to(dev, non_blocking=True)
        o1 = tok.size; o2 = o1 + lists.size; o3 = o2 + segs.size
        cost = torch.empty(nd, dtype=torch.float32, device=dev) if want_cost else None
        plen = torch.empty(nd, dtype=torch.int32, device=dev) if want_cost else None
        dist = torch.empty(nd, dtype=torch.float32, device=dev)
        twice = torch.empty(no, dtype=torch.int32, device=dev)
        t = (d[:o1].data_ptr(), tok.shape[0], d[o1:o2].data_ptr(), lists.size, d[o2:o3].data_ptr(), segs.size, d[o3:].data_ptr(), rows.shape[0])
        out = (cost.data_ptr() if want_cost else None, plen.data_ptr() if want_cost else None, dist.data_ptr(), twice.data_ptr())
        _lib.check(call(t, (wg, nd, no), out, _lib.current_stream()))
        for b in borrowed + (d,):                        # borrowed until the enqueued work is done
            b.record_stream(torch.cuda.current_stream())
    return PairTables(cost, plen, dist, twice, [int(r[6]) for r in rows], [int(r[7]) for r in rows])


def code_table(codebook):
    """``codebook`` (M, D) fp32 on the device -> the (M, M) device table of frame distances between its rows, each with the bits
    ``pair_distances`` computes for that pair of frames (``vqcpc_abx_code_table``: two launches, no synchronisation)."""
    import torch
    if not isinstance(codebook, torch.Tensor):
        raise TypeError("abx.code_table: codebook must be a torch tensor on the device")
    _lib.require_cuda(codebook, "abx codebook")
    if codebook.dim() != 2 or codebook.dtype != torch.float32:
        raise ValueError(f"abx: codebook must be (M, D) float32, got {tuple(codebook.shape)} {codebook.dtype}")
    M, D = int(codebook.shape[0]), int(codebook.shape[1])
    if not 1 <= M <= M_MAX:
        raise ValueError(f"abx: codebook of {M} rows, supported 1..{M_MAX}")
    if D % 4 or not 4 <= D <= 512:
        raise ValueError(f"abx: D = {D}, supported: a multiple of 4 in [4, 512]")
    lib = _lib.load()
    book = codebook.detach().contiguous()
    n = C.c_uint64()
    _lib.check(lib.vqcpc_abx_index_workspace_bytes(M, D, C.byref(n)))
    with _lib.device_guard(book.device):
        buf = torch.empty(n.value // 4, dtype=torch.float32, device=book.device)      # work (M, D), then the table
        table = buf[M * D:].view(M, M)
        _lib.check(lib.vqcpc_abx_code_table(book.data_ptr(), M, D, buf.data_ptr(), table.data_ptr(), _lib.current_stream()))
        book.record_stream(torch.cuda.current_stream())
    return table


def _metric(metric):
    if metric not in METRICS:
        raise ValueError(f"abx: metric must be one of {sorted(METRICS)}, got {metric!r}")
    return METRICS[metric]


def pair_distances_indices(codes, tokens, blocks: Sequence[Block], table=None, n_codes=None, metric: str = "angular",
                           want_cost: bool = True) -> PairTables:
    """``pair_distances`` on runs of codebook indices: ``codes`` (n_frames,) integer device tensor, ``tokens`` rows of it.
    ``metric="angular"``: ``table`` = ``code_table(codebook)``; every output has the bits ``pair_distances(codebook[codes], ..)``
    gives.  ``metric="edit"``: Levenshtein distance of the raw runs, ``cost`` = the distance, ``path_len`` = max(Ta, Tb),
    ``dist`` = cost / path_len; no table is needed, ``n_codes`` (default: the table's M) bounds the codes.  Does not
    synchronise, so codes outside [0, n_codes) are clamped on the device, not reported (``score_indices`` checks them)."""
    import torch
    m = _metric(metric)
    if not isinstance(codes, torch.Tensor):
        raise TypeError("abx.pair_distances_indices: codes must be a torch tensor on the device")
    _lib.require_cuda(codes, "abx codes")
    if codes.dim() != 1 or codes.dtype.is_floating_point or codes.dtype.is_complex or codes.dtype == torch.bool:
        raise ValueError(f"abx: codes must be a 1-D integer tensor, got {tuple(codes.shape)} {codes.dtype}")
    if table is not None:
        _lib.require_cuda(table, "abx code table")
        _lib.require_same_device(table, codes, "the code table")
        if table.dim() != 2 or table.shape[0] != table.shape[1] or table.dtype != torch.float32 or not table.is_contiguous():
            raise ValueError(f"abx: table must be a contiguous (M, M) float32 tensor, got {tuple(table.shape)} {table.dtype}")
        if n_codes is not None and int(n_codes) != table.shape[0]:
            raise ValueError(f"abx: n_codes = {n_codes}, but the table has {table.shape[0]} rows")
        n_codes = int(table.shape[0])
    elif m == METRICS["angular"]:
        raise ValueError("abx: metric 'angular' needs table = code_table(codebook)")
    elif n_codes is None:
        raise ValueError("abx: give n_codes (or a table) with metric 'edit'")
    M = int(n_codes)
    if not 1 <= M <= M_MAX:
        raise ValueError(f"abx: n_codes = {M}, supported 1..{M_MAX}")
    n_frames = int(codes.shape[0])
    if n_frames < 1:
        raise ValueError("abx: no frames")
    codes = codes.to(torch.int32).contiguous()
    tab = table if m == METRICS["angular"] else None
    lib = _lib.load()
    return _enqueue(codes.device, tokens, blocks, n_frames, want_cost, (codes,) + ((tab,) if tab is not None else ()),
                    lambda t, n, out, stream: lib.vqcpc_abx_score_indices(tab.data_ptr() if tab is not None else None, M, codes.data_ptr(),
                                                                          n_frames, *t, *n, *out, stream, m))


def _layout(by_file, items, frame_shift, frame_offset, what):
    """The files the items name, in order, checked to be device tensors, and the items' tokens as rows of their concatenation."""
    import torch
    files = sorted({it.file for it in items})
    for f in files:
        if f not in by_file:
            raise KeyError(f"abx.score: no {what} for file {f!r}")
        t = by_file[f]
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"abx.score: {what} of {f!r} must be a torch tensor on the device")
        _lib.require_cuda(t, f"abx {what} of {f!r}")
    first, rows = {}, 0
    for f in files:
        first[f] = rows
        rows += int(by_file[f].shape[0])
    tok = tokens_of(items, {f: int(by_file[f].shape[0]) for f in files}, frame_shift, frame_offset)
    return files, [(first[it.file] + lo, n) for it, (lo, n) in zip(items, tok)]


def _score_chunks(items, mode, mem_budget_bytes, prepare):
    """plan -> chunks of blocks -> ``run = prepare()`` once, ``run(blocks)`` -> twice_wins per chunk -> ``aggregate``."""
    import torch
    pl = plan(items, mode)
    res_tw = np.zeros(pl.n_out, np.int32)
    chunks = block_chunks(pl.blocks, mem_budget_bytes) if pl.blocks else []
    if chunks:
        run = prepare()
        res_tw = torch.cat([run([pl.blocks[i] for i in ids]) for ids in chunks]).cpu().numpy()
    res = aggregate(pl, res_tw)
    res.update(twice_wins=res_tw, n_blocks=len(pl.blocks), n_chunks=len(chunks), mode=mode)
    return res


def score(features_by_file, items, mode: str = "within", frame_shift: float = FRAME_SHIFT, frame_offset: float = FRAME_OFFSET,
          mem_budget_bytes: int = 1 << 30) -> dict:
    """ABX score of ``features_by_file`` (file -> (T, D) fp32 device tensor) on ``items`` (a path or a list of ``Item``): the
    frames are uploaded / gathered once, the plan's blocks run in chunks of ``block_chunks(.., mem_budget_bytes)`` (the budget
    is for the per-block tables; the frames, their work copy and the token table come on top in every call), and
    ``aggregate`` makes the score.  Adds ``twice_wins`` (int32 numpy, plan order), ``n_blocks`` and ``n_chunks``."""
    import torch
    if not isinstance(items, (list, tuple)):
        items = read_items(items)
    files, tokens = _layout(features_by_file, items, frame_shift, frame_offset, "features")

    def prepare():
        feats = torch.cat([features_by_file[f].to(torch.float32) for f in files], dim=0).contiguous()
        return lambda blocks: pair_distances(feats, tokens, blocks, want_cost=False).twice_wins
    return _score_chunks(items, mode, mem_budget_bytes, prepare)


def score_indices(codebook, indices_by_file, items, mode: str = "within", metric: str = "angular", frame_shift: float = FRAME_SHIFT,
                  frame_offset: float = FRAME_OFFSET, mem_budget_bytes: int = 1 << 30) -> dict:
    """``score`` on the units' indices: ``indices_by_file`` (file -> (T,) integer device tensor), ``codebook`` (M, D) fp32 on the
    device.  ``metric="angular"``: the counts, and so the score, are those of ``score`` on ``codebook[indices]``, bit for bit;
    the device holds 4 bytes per frame and one (M, M) table, built once per call.  ``metric="edit"``: tokens are compared by the
    Levenshtein distance of their index runs over the longer run's length; ``codebook`` may be None (the number of codes is
    then the largest index + 1).  An index outside [0, M) raises IndexError naming the file before anything is scored.  The
    result gains ``metric``."""
    import torch
    m = _metric(metric)
    if not isinstance(items, (list, tuple)):
        items = read_items(items)
    files, tokens = _layout(indices_by_file, items, frame_shift, frame_offset, "indices")
    for f in files:
        t = indices_by_file[f]
        if t.dim() != 1 or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError(f"abx.score_indices: indices of {f!r} must be a 1-D integer tensor, got {tuple(t.shape)} {t.dtype}")
    if codebook is None and m == METRICS["angular"]:
        raise ValueError("abx.score_indices: metric 'angular' needs the codebook")
    if codebook is not None:
        if not isinstance(codebook, torch.Tensor):
            raise TypeError("abx.score_indices: codebook must be a torch tensor on the device")
        _lib.require_cuda(codebook, "abx codebook")

    def prepare():
        codes = torch.cat([indices_by_file[f].to(torch.int64) for f in files])
        lo, hi = torch.stack([codes.min(), codes.max()]).tolist()                     # the one range check, on the device
        M = int(codebook.shape[0]) if codebook is not None else max(hi, 0) + 1
        if lo < 0 or hi >= M:
            for f in files:
                t = indices_by_file[f]
                if t.numel() and (int(t.min()) < 0 or int(t.max()) >= M):
                    raise IndexError(f"abx.score_indices: file {f!r} holds an index outside [0, {M}): {int(t.min())}..{int(t.max())}")
        table = code_table(codebook) if m == METRICS["angular"] else None
        codes = codes.to(torch.int32)
        return lambda blocks: pair_distances_indices(codes, tokens, blocks, table=table, n_codes=M, metric=metric, want_cost=False).twice_wins
    res = _score_chunks(items, mode, mem_budget_bytes, prepare)
    res["metric"] = metric
    return res
