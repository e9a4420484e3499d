#!/usr/bin/env python3
"""Times of ABX scoring on one synthetic workload: the three-launch call ``vqcpc_abx_score`` and, on the same units given as
codebook indices, ``vqcpc_abx_score_indices`` (angular metric from the code table, edit metric) and the table build
``vqcpc_abx_code_table`` on its own, with the device bytes each path holds -- against (a) the float64 numpy restatement of ``tests/abx_ref.py`` spread over the host's threads and (b) a batched PyTorch composition of the same protocol on
the same GPU (one ``bmm`` for the frame cosines, ``acos``, and one anti-diagonal DP step per torch op group).

    python tools/abx_times.py [--out profiles/abx_times.txt] [--windows 20] [--window-ms 40] [--threads 16]

HIP events; every variant is warmed up; a window is as many back-to-back calls as fill ``--window-ms``; the GPU variants take
turns window by window inside one process; median [min .. max] over the windows.  (a) is wall time of whole runs.
"""
import argparse
import math
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from timing import measure  # noqa: E402
from vectorquantizedcpc_amd import _lib, abx, synth  # noqa: E402

SPEAKERS, CONTEXTS, PHONES, PER_CELL = 8, 5, 10, 5          # 8 x 5 x 10 x 5 = 2 000 tokens
D, FRAMES_PER_FILE, CODEBOOK = 64, 4000, 512
PAIRS_PER_TORCH_BATCH = 1 << 17


def workload():
    """2 000 items of 3..25 frames over one file per speaker; frames = rows of a 512-entry codebook (quantised units)."""
    u = synth.uniform01("abx/times", 2 * SPEAKERS * CONTEXTS * PHONES * PER_CELL)
    items, k = [], 0
    for s in range(SPEAKERS):
        for c in range(CONTEXTS):
            for p in range(PHONES):
                for _ in range(PER_CELL):
                    n = 3 + int(u[k] * 23)
                    j = int(u[k + 1] * (FRAMES_PER_FILE - 30)); k += 2
                    on = 0.01 + 0.02 * j
                    items.append(abx.Item(f"f{s}", round(on - 0.005, 4), round(on + 0.02 * (n - 1) + 0.005, 4), f"p{p}", f"l{c}", f"r{c}", f"s{s}"))
    book = synth._normalish("abx/times/book", (CODEBOOK, D), synth.SEED).numpy()
    idx = {f"f{s}": synth.randint(f"abx/times/codes{s}", (FRAMES_PER_FILE,), CODEBOOK).numpy() for s in range(SPEAKERS)}
    feats = {f: book[v].astype(np.float32) for f, v in idx.items()}
    files = sorted(feats)
    first = np.cumsum([0] + [feats[f].shape[0] for f in files])
    tok = abx.tokens_of(items, {f: feats[f].shape[0] for f in files})
    tokens = [(int(first[files.index(it.file)]) + lo, n) for it, (lo, n) in zip(items, tok)]
    return items, np.concatenate([feats[f] for f in files]), tokens, book.astype(np.float32), np.concatenate([idx[f] for f in files])


def fused_call(frames, tokens, blocks, dev):
    """The device tables of one call and a closure that enqueues its three launches."""
    lib = _lib.load()
    tok, lists, segs, rows, wg, nd, no = abx._tables(tokens, blocks, frames.shape[0])
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (tok, lists, segs, rows)]
    f = torch.from_numpy(frames).to(dev)
    work = torch.empty(f.numel(), device=dev)
    dist = torch.empty(nd, device=dev)
    tw = torch.empty(no, dtype=torch.int32, device=dev)
    stream = _lib.current_stream()

    def call():
        _lib.check(lib.vqcpc_abx_score(f.data_ptr(), f.shape[0], f.shape[1], t[0].data_ptr(), tok.shape[0], t[1].data_ptr(), lists.size,
                                       t[2].data_ptr(), segs.size, t[3].data_ptr(), rows.shape[0], wg, nd, no, work.data_ptr(), None, None,
                                       dist.data_ptr(), tw.data_ptr(), stream))
    held = {"frames": f.numel() * 4, "normalised copy of the frames": work.numel() * 4}
    common = sum(a.numel() * 4 for a in t) + dist.numel() * 4 + tw.numel() * 4
    return call, dist, tw, (f, work, t), held, common


def table_call(book, dev):
    """The code table of the workload's codebook and a closure that enqueues its two launches."""
    lib = _lib.load()
    b = torch.from_numpy(book).to(dev)
    M, Dm = b.shape
    work = torch.empty(M * Dm, device=dev)
    table = torch.empty(M, M, device=dev)
    stream = _lib.current_stream()

    def call():
        _lib.check(lib.vqcpc_abx_code_table(b.data_ptr(), M, Dm, work.data_ptr(), table.data_ptr(), stream))
    return call, table, (b, work)


def index_call(codes, table, tokens, blocks, dev, metric):
    """The same tables on the indices: a closure that enqueues the two launches of ``vqcpc_abx_score_indices``."""
    lib = _lib.load()
    tok, lists, segs, rows, wg, nd, no = abx._tables(tokens, blocks, codes.shape[0])
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (tok, lists, segs, rows)]
    c = torch.from_numpy(codes.astype(np.int32)).to(dev)
    dist = torch.empty(nd, device=dev)
    tw = torch.empty(no, dtype=torch.int32, device=dev)
    stream = _lib.current_stream()
    M = table.shape[0]

    def call():
        _lib.check(lib.vqcpc_abx_score_indices(table.data_ptr() if metric == 0 else None, M, c.data_ptr(), c.shape[0], t[0].data_ptr(),
                                               tok.shape[0], t[1].data_ptr(), lists.size, t[2].data_ptr(), segs.size, t[3].data_ptr(),
                                               rows.shape[0], wg, nd, no, None, None, dist.data_ptr(), tw.data_ptr(), stream, metric))
    return call, dist, tw, (c, t)


def torch_call(frames, tokens, blocks, dev):
    """(b): normalise, gather padded tokens, per batch of pairs one bmm -> acos / pi -> anti-diagonal DP with torch ops -> per
    block the counts by broadcasting.  Same protocol (first minimum: diagonal, up, left), written as a user would in PyTorch."""
    f = torch.from_numpy(frames).to(dev)
    tk = torch.tensor(tokens, device=dev)
    T = int(tk[:, 1].max())
    rows = (tk[:, :1] + torch.arange(T, device=dev)[None, :]).clamp(max=f.shape[0] - 1)
    pa = torch.cat([torch.tensor(b.a, device=dev).repeat_interleave(len(b.x)) for b in blocks])
    px = torch.cat([torch.tensor(b.x, device=dev).repeat(len(b.a)) for b in blocks])
    P = pa.numel()
    seg_masks = []
    for b in blocks:
        s = torch.zeros(b.n_seg, len(b.a), device=dev)
        for q in range(b.n_seg):
            s[q, b.seg[q]:b.seg[q + 1]] = 1
        own = s[torch.tensor(b.x_seg, device=dev)].clone()                       # (nX, nA): A tokens of x's own phone
        own[torch.tensor(b.x, device=dev)[:, None] == torch.tensor(b.a, device=dev)[None, :]] = 0
        seg_masks.append((s, own))
    inf = float("inf")

    def call():
        fn = torch.nn.functional.normalize(f, dim=1)
        tokf = fn[rows]                                                         # (n_tokens, T, D)
        dist = torch.empty(P, device=dev)
        for p0 in range(0, P, PAIRS_PER_TORCH_BATCH):
            a, x = pa[p0:p0 + PAIRS_PER_TORCH_BATCH], px[p0:p0 + PAIRS_PER_TORCH_BATCH]
            d = torch.acos(torch.bmm(tokf[a], tokf[x].transpose(1, 2)).clamp(-1.0, 1.0)) * (1.0 / math.pi)
            n = a.numel()
            Cc = torch.full((n, T + 1, T + 1), inf, device=dev)
            Ll = torch.zeros((n, T + 1, T + 1), dtype=torch.int32, device=dev)
            Cc[:, 1, 1] = d[:, 0, 0]
            Ll[:, 1, 1] = 1
            for k in range(1, 2 * T - 1):
                i = torch.arange(max(0, k - T + 1), min(k, T - 1) + 1, device=dev)
                j = k - i
                cand = torch.stack([Cc[:, i, j], Cc[:, i, j + 1], Cc[:, i + 1, j]], dim=2)
                lens = torch.stack([Ll[:, i, j], Ll[:, i, j + 1], Ll[:, i + 1, j]], dim=2)
                best, arg = cand.min(dim=2, keepdim=True)
                arg = (cand == best).to(torch.int8).argmax(dim=2, keepdim=True)   # the first minimum
                Cc[:, i + 1, j + 1] = d[:, i, j] + best[:, :, 0]
                Ll[:, i + 1, j + 1] = lens.gather(2, arg)[:, :, 0] + 1
            ar = torch.arange(n, device=dev)
            ta, tb = tk[a, 1], tk[x, 1]
            dist[p0:p0 + n] = Cc[ar, ta, tb] / Ll[ar, ta, tb]
        out, base = [], 0
        for b, (s, own) in zip(blocks, seg_masks):
            na, nx = len(b.a), len(b.x)
            Dm = dist[base:base + na * nx].view(na, nx)
            base += na * nx
            w = 2.0 * (Dm[:, None, :] < Dm[None, :, :]) + 1.0 * (Dm[:, None, :] == Dm[None, :, :])      # (a, b, x)
            out.append(torch.einsum("xa,abx,qb->xq", own, w, s))
        return dist, out
    return call


def host_block(args):
    import abx_ref
    frames, tokens, b = args
    d = abx_ref.pair_table(frames, tokens, b.a, b.x)[2]
    return abx_ref.twice_wins_of(d, b.a, b.seg, b.x, b.x_seg)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=40.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--host-runs", type=int, default=2)
    args = ap.parse_args()
    import multiprocessing as mp
    dev = torch.device("cuda:0")
    items, frames, tokens, book, codes = workload()
    lens = [n for _, n in tokens]
    lines = [f"ABX scoring, HIP-event ms per call: median [min .. max] over {args.windows} windows of >= {args.window_ms:g} ms, GPU variants alternated",
             "device: (filled in below)",
             f"workload: {len(items)} tokens of {min(lens)}..{max(lens)} frames (mean {np.mean(lens):.1f}), D = {D}, {SPEAKERS} speakers x "
             f"{CONTEXTS} contexts x {PHONES} phones x {PER_CELL} tokens, frames = rows of a {CODEBOOK}-entry codebook"]
    host_tw = {}
    # (a) first: the pool is created, used and closed before the first torch.cuda call of this process, so no child ever
    # inherits an initialised HIP runtime and only this process opens the GPU
    assert not torch.cuda.is_initialized()
    with mp.get_context("fork").Pool(args.threads) as pool:
        host = {}
        for mode in ("within", "across"):
            pl = abx.plan(items, mode)
            runs = []
            for _ in range(args.host_runs):
                t0 = time.perf_counter()
                host_tw[mode] = pool.map(host_block, [(frames, tokens, b) for b in pl.blocks], chunksize=1)
                runs.append(1e3 * (time.perf_counter() - t0))
            host[mode] = runs
    lines[1] = f"device: {torch.cuda.get_device_name(0)}"
    FUSED, INDEX, EDIT, TABLE = ("fused three-launch call", "indices (table gather + DTW, count)", "indices, edit metric",
                                 "code table build (once per score)")
    build, table, keep_table = table_call(book, dev)
    build()
    for mode in ("within", "across"):
        pl = abx.plan(items, mode)
        fused, dist, tw, keep, held, common = fused_call(frames, tokens, pl.blocks, dev)
        icall, idist, itw, ikeep = index_call(codes, table, tokens, pl.blocks, dev, 0)
        ecall, edist, etw, ekeep = index_call(codes, table, tokens, pl.blocks, dev, 1)
        tcall = torch_call(frames, tokens, pl.blocks, dev)
        fused(); icall(); ecall()
        torch.cuda.synchronize()
        same = bool(torch.equal(dist.view(torch.int32), idist.view(torch.int32)) and torch.equal(tw, itw))
        want = np.concatenate([t.reshape(-1) for t in host_tw[mode]])
        got = tw.cpu().numpy()
        td, tout = tcall()
        ttw = torch.cat([o.reshape(-1) for o in tout]).cpu().numpy()
        flop = sum(lens[a] * lens[x] for b in pl.blocks for a in b.a for x in b.x) * D * 8
        r = measure({FUSED: fused, INDEX: icall, EDIT: ecall, TABLE: build, "torch on the GPU (bmm + DP as torch ops)": lambda: tcall()},
                    args.windows, args.window_ms, probe=2, min_reps=1)
        lines.append(f"\n{mode}: {len(pl.blocks)} blocks, {pl.n_pairs} pairs, {int(abx.aggregate(pl, got)['n_triples'])} triples, "
                     f"{flop / 1e9:.2f} GFLOP of frame distances")
        for name, (med, lo, hi, reps) in r.items():
            lines.append(f"  {name:44s} {med:10.4f} ms  [{lo:.4f} .. {hi:.4f}]  {reps} calls / window")
        h = host[mode]
        lines.append(f"  {'float64 numpy restatement, ' + str(args.threads) + ' processes':44s} {statistics.median(h):10.1f} ms  [{min(h):.1f} .. {max(h):.1f}]  "
                     f"{len(h)} runs, wall time")
        fm = r[FUSED][0]
        once = r[INDEX][0] + r[TABLE][0]
        lines.append(f"  indices + one table build = {once:.4f} ms (medians) against the fused call's fastest window {r[FUSED][1]:.4f} ms: "
                     f"{r[FUSED][1] / once:.2f}x; fused / indices = {fm / r[INDEX][0]:.2f}x, fused / edit = {fm / r[EDIT][0]:.2f}x")
        lines.append(f"  indices against the fused call, dist and twice_wins bit for bit: {'equal' if same else 'DIFFERENT'}; "
                     f"edit-metric score {abx.aggregate(pl, etw.cpu().numpy())['score']:.6f}")
        ibytes = {"codes": codes.size * 4, "code table": table.numel() * 4, "normalised codebook": book.size * 4}
        lines.append(f"  device bytes held: fused {sum(held.values())} (" + ", ".join(f"{k} {v}" for k, v in held.items()) + f"); indices "
                     f"{sum(ibytes.values())} (" + ", ".join(f"{k} {v}" for k, v in ibytes.items()) + f"; edit: codes only); both: {common} "
                     "of token / block tables, dist and twice_wins")
        lines.append(f"  torch / fused = {r['torch on the GPU (bmm + DP as torch ops)'][0] / fm:.1f}x, numpy / fused = {statistics.median(h) / fm:.0f}x")
        lines.append(f"  counts differing from float64: fused {int((got != want).sum())} of {want.size} (scores {abx.aggregate(pl, got)['score']:.6f} / "
                     f"{abx.aggregate(pl, want)['score']:.6f}), torch composition {int((ttw != want).sum())} (score {abx.aggregate(pl, ttw)['score']:.6f})")
        del keep, ikeep, ekeep
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"),
                          os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", "abx.hip")], capture_output=True, text=True)
    lines.append("\nkernel resources (tools/kernel_resources.py vectorquantizedcpc_amd/csrc/abx.hip):")
    lines += ["  " + l for l in res.stdout.splitlines()]
    rem = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-c",
                          os.path.join(ROOT, "vectorquantizedcpc_amd", "csrc", "abx.hip"), "-o", os.devnull,
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True).stderr
    lines.append("  LDS bytes per workgroup, in the same order: " + ", ".join(re.findall(r"LDS Size \[bytes/block\]: (\d+)", rem)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
