"""-m gpu: ``vqcpc_adam_step`` and ``optim.Adam`` past the twelve cases -- the ``WIDE`` cases of tests/adam_ref.py bit for bit against
the numpy restatement and judged against ``torch.optim.Adam`` in float64 (the ladders per tensor), canaries around the buffers of
the three cases with irregular tables and tails, an update number past 2^32 and non-finite / overflowing gradients through the C
interface, and what ``optim.Adam``'s cached rows must survive between two steps: a state dict loaded in place, storage of a
parameter or of a moment replaced, a group reordered or appended to, a parameter that is not 16-byte aligned.

Nothing here is measured on the code under test: the restatement is numpy's, the judge's ``e_ref`` is torch's own fp32 run on the
CPU (tests/adam_ref.py computes both).
"""
import copy

import numpy as np
import pytest
import torch

import adam_ref as R
from adam_ref import arena_case, bits, hyper
from vectorquantizedcpc_amd import _lib, optim

pytestmark = pytest.mark.gpu


def same_bits(a, b, what):
    """``a`` has the bits of ``b``; else the element index and both values."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    assert a.dtype == b.dtype == np.float32 and a.size == b.size, (what, a.dtype, b.dtype, a.size, b.size)
    diff = np.flatnonzero(bits(a) != bits(b))
    assert diff.size == 0, f"{what} ({a.size} elements): {diff.size} elements differ, first at {diff[0]}: {a[diff[0]]!r} != {b[diff[0]]!r}"


# ------------------------------------------------------------------ a. the kernel's bits are the restatement's; the judge
@pytest.mark.parametrize("name", list(R.WIDE))
def test_bits_equal_the_restatement_and_float64_judges_them(name):
    want = R.restated(name)
    ref64, ref32 = R.reference(name)
    got = R.run_torch(name, torch.float32, "cuda", optim.Adam)
    assert len(got) == len(want) == R.WIDE[name]["steps"]
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want), 1):
        for key in R.KEYS:
            assert len(g[key]) == len(w[key]) == len(R.WIDE[name]["numels"])
            for i, (a, b) in enumerate(zip(g[key], w[key])):
                same_bits(a, b, f"{name}: update {k}, {key} of tensor {i}")
        worst = max(worst, R.judge_snapshot(name, k, g, ref64[k - 1], ref32[k - 1], "vqcpc_adam_step"))
    print(f"{name}: bit for bit the restatement over {len(got)} updates; largest err / bound against float64 = {worst:.3f}")
    assert worst <= 1.0


# ------------------------------------------------------------------ b. canaries
def device():
    return torch.device("cuda", torch.cuda.current_device())


def check_arena(name, arena, want, arrays, what):
    """No canary word changed, no gradient written, p / exp_avg / exp_avg_sq of every tensor with elements as ``want`` has them."""
    words = arena.read()
    assert arena.canaries_intact(words), what
    live = [i for i, n in enumerate(R.case(name)["numels"]) if n]
    assert len(arrays) == 4 * len(live)
    for j, i in enumerate(live):
        same_bits(arena.array(words, 4 * j), want["p"][i], f"{what}: p of tensor {i}")
        same_bits(arena.array(words, 4 * j + 1), arrays[4 * j + 1], f"{what}: the gradient of tensor {i} was written")
        same_bits(arena.array(words, 4 * j + 2), want["exp_avg"][i], f"{what}: exp_avg of tensor {i}")
        same_bits(arena.array(words, 4 * j + 3), want["exp_avg_sq"][i], f"{what}: exp_avg_sq of tensor {i}")


@pytest.mark.parametrize("name", ["full_table_mixed", "two_launches_mixed", "tails"])
def test_canaries_around_every_buffer_keep_their_bits(name):
    arena, table, n, arrays = arena_case(name)
    assert n == sum(1 for x in R.WIDE[name]["numels"] if x)
    _lib.adam_step(table, n, hyper(name), device())
    torch.cuda.synchronize()
    check_arena(name, arena, R.restated(name)[0], arrays, name)


# ------------------------------------------------------------------ c. an update number past 2^32
def one_update(name, gs, t, state=None):
    """The restatement's update number ``t`` of the case's start (or of ``state`` = (p, m, v), updated in place) with the gradients ``gs``."""
    c = R.case(name)
    p, m, v = state if state is not None else (R.params(name), *R.start_state(name))
    sc = R.scalars(c["lr"], *c["betas"], c["eps"], t)
    with np.errstate(all="ignore"):
        for pi, gi, mi, vi in zip(p, gs, m, v):
            R.update(pi, gi, mi, vi, sc)
    return {"p": p, "exp_avg": m, "exp_avg_sq": v}


def test_update_number_past_32_bits_reaches_the_scalars():
    """``state["step"]`` of torch is fp32 and cannot hold the number: through the C interface.  Truncated to 32 bits it would be
    update 1."""
    name, t = "lr_1", 2 ** 32 + 1
    c = R.WIDE[name]
    assert c["betas"] == R.REF_BETAS and c["numels"] == [R.CHUNK + 3, 37] and c["first"] == 1
    big, one = R.scalars(c["lr"], *c["betas"], c["eps"], t), R.scalars(c["lr"], *c["betas"], c["eps"], 1)
    assert big["rb"] != one["rb"] and big["ss"] != one["ss"] and big["rb"] == np.float32(1.0) and big["ss"] == np.float32(c["lr"])
    gs = R.grads(name, 1)
    want, first = one_update(name, gs, t), one_update(name, gs, 1)
    assert not np.array_equal(bits(want["p"][0]), bits(first["p"][0]))   # the moments' scalars do not depend on the update number
    arena, table, n, arrays = arena_case(name)
    h = hyper(name, step=t)
    assert h.step == t
    _lib.adam_step(table, n, h, device())
    torch.cuda.synchronize()
    check_arena(name, arena, want, arrays, f"{name} at update 2^32 + 1")
    assert not np.array_equal(bits(arena.array(arena.read(), 0)), bits(first["p"][0]))


# ------------------------------------------------------------------ d. non-finite and overflowing gradients
def test_nonfinite_and_overflowing_gradients_follow_ieee_and_touch_no_neighbour():
    """include/vqcpc.h: g * g that overflows freezes the element's p (v' = inf, m' / d = 0), an infinite or NaN g makes it NaN,
    no other element of the call is affected.  One special in the first vector, in the last element of chunk 0, in the first of
    chunk 1, three in the scalar tail.  NaN payloads are not compared."""
    name, C = "nonfinite", R.CHUNK
    c = R.case(name)
    assert c["numels"] == [C + 7] and c["first"] == 50000 and c["steps"] == 2
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    special = {0: np.float32(3e19), 1: np.float32(-3e19), 5: inf, C - 1: -inf, C: nan, C + 4: np.float32(3e19), C + 5: nan, C + 6: inf}
    frozen, poisoned = [0, 1, C + 4], [5, C - 1, C, C + 5, C + 6]
    plain = [R.grads(name, 1), R.grads(name, 2)]
    g1 = plain[0][0].copy()
    for i, x in special.items():
        g1[i] = x
    with np.errstate(all="ignore"):
        assert np.isinf(g1[frozen] * g1[frozen]).all() and np.isfinite(g1[frozen]).all()
    gs = [[g1], plain[1]]
    # the restatement does what the header says -- asserted on the host, before the kernel is held to it
    p0 = R.params(name)[0]
    state, state_plain, want = None, None, []
    others = np.setdiff1d(np.arange(C + 7), list(special))
    for k in (1, 2):
        snap = one_update(name, gs[k - 1], c["first"] + k - 1, state)
        state = (snap["p"], snap["exp_avg"], snap["exp_avg_sq"])
        want.append({key: [a.copy() for a in snap[key]] for key in R.KEYS})
        snap_plain = one_update(name, plain[k - 1], c["first"] + k - 1, state_plain)
        state_plain = (snap_plain["p"], snap_plain["exp_avg"], snap_plain["exp_avg_sq"])
        p = snap["p"][0]
        assert np.array_equal(bits(p[frozen]), bits(p0[frozen])), "an overflowing g * g freezes p"
        assert np.isinf(snap["exp_avg_sq"][0][frozen]).all() and np.isfinite(snap["exp_avg"][0][frozen]).all()
        assert np.isnan(p[poisoned]).all(), "an infinite or NaN g makes p NaN"
        for key in R.KEYS:
            assert np.array_equal(bits(snap[key][0][others]), bits(snap_plain[key][0][others])), "no other element is affected"
            assert np.isfinite(snap[key][0][others]).all()
    # the kernel: NaN exactly where the restatement has it, every other element (inf included) with the restatement's bits
    arena, table, n, arrays = arena_case(name, gs=gs[0])
    assert n == 1
    for k in (1, 2):
        if k == 2:                                                       # the second update's gradient, into the same buffer
            at, size = arena.spans[1]
            arena.dev[at:at + size] = torch.from_numpy(gs[1][0].view(np.int32)).cuda()
        _lib.adam_step(table, n, hyper(name, k), device())
        torch.cuda.synchronize()
        words = arena.read()
        assert arena.canaries_intact(words)
        assert np.array_equal(bits(arena.array(words, 1)), bits(gs[k - 1][0])), "the gradient was written"
        for j, key in ((0, "p"), (2, "exp_avg"), (3, "exp_avg_sq")):
            got, exp = arena.array(words, j), want[k - 1][key][0]
            assert np.array_equal(np.isnan(got), np.isnan(exp)), (k, key, np.flatnonzero(np.isnan(got) != np.isnan(exp)))
            ok = ~np.isnan(exp)
            same_bits(got[ok], exp[ok], f"update {k}, {key}, the elements that are not NaN")


# ------------------------------------------------------------------ e. what the cached rows survive between two steps
NAME = "vector_and_tail"


class Shadow:
    """The restatement's p, exp_avg, exp_avg_sq and update count of tensor ``i`` of ``NAME``, stepped one tensor at a time."""

    def __init__(self, i):
        self.i, self.p = i, R.params(NAME)[i]
        self.m, self.v, self.t = np.zeros_like(self.p), np.zeros_like(self.p), 0

    def step(self, k):
        """One update with the gradient of the case's update ``k``."""
        self.t += 1
        c = R.CASES[NAME]
        R.update(self.p, R.grads(NAME, k)[self.i], self.m, self.v, R.scalars(c["lr"], *c["betas"], c["eps"], self.t))


def make(n=4):
    c = R.CASES[NAME]
    ps = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in R.params(NAME)[:n]]
    return ps, optim.Adam(ps, lr=c["lr"], betas=c["betas"], eps=c["eps"]), [Shadow(i) for i in range(n)]


def give(ps, shadows, k, only=None):
    """The gradients of the case's update ``k`` (None for a parameter not in ``only``), and the shadows stepped likewise."""
    for p, s in zip(ps, shadows):
        take = only is None or s.i in only
        p.grad = torch.from_numpy(R.grads(NAME, k)[s.i]).cuda() if take else None
        if take:
            s.step(k)


def check(ps, opt, shadows, what):
    torch.cuda.synchronize()
    for p, s in zip(ps, shadows):
        st = opt.state[p]
        assert float(st["step"]) == s.t, (what, s.i, float(st["step"]), s.t)
        same_bits(p.detach().cpu().numpy(), s.p, f"{what}: p of parameter {s.i}")
        same_bits(st["exp_avg"].cpu().numpy(), s.m, f"{what}: exp_avg of parameter {s.i}")
        same_bits(st["exp_avg_sq"].cpu().numpy(), s.v, f"{what}: exp_avg_sq of parameter {s.i}")


def test_rewind_in_place_by_load_state_dict():
    ps, opt, shadows = make()
    for k in (1, 2):
        give(ps, shadows, k)
        opt.step()
    check(ps, opt, shadows, "update 2")
    saved, kept = copy.deepcopy(opt.state_dict()), [p.detach().clone() for p in ps]
    give(ps, shadows, 3)
    opt.step()
    check(ps, opt, shadows, "update 3")
    first = [p.detach().clone() for p in ps]
    with torch.no_grad():
        for p, x in zip(ps, kept):
            p.copy_(x)
    opt.load_state_dict(saved)                                           # the same optimizer: its rows and mirrored counts exist
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0] * 4
    opt.step()                                                           # the gradients of update 3 are still in place
    check(ps, opt, shadows, "update 3 again")
    assert all(torch.equal(p.view(torch.int32), x.view(torch.int32)) for p, x in zip(ps, first))
    for i, p in enumerate(ps):
        same_bits(p.detach().cpu().numpy(), R.restated(NAME)[2]["p"][i], f"update 3 again: parameter {i} against the case")


def test_storage_of_a_parameter_moves():
    ps, opt, shadows = make()
    give(ps, shadows, 1)
    opt.step()
    check(ps, opt, shadows, "update 1")
    old = [p.data for p in ps]
    after_1 = [x.clone() for x in old]
    for p in ps:
        p.data = p.data.clone()
    assert all(p.data_ptr() != x.data_ptr() for p, x in zip(ps, old))
    give(ps, shadows, 2)
    opt.step()
    check(ps, opt, shadows, "update 2 in the new storage")
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(old, after_1)), "the old storage was written"


def test_storage_of_a_moment_moves():
    """``.data =`` replaces the storage under the same tensor object: the row check has to look at the moments' pointers too."""
    ps, opt, shadows = make()
    give(ps, shadows, 1)
    opt.step()
    check(ps, opt, shadows, "update 1")
    old, after_1 = [], []
    for p in ps:
        st = opt.state[p]
        for key in ("exp_avg", "exp_avg_sq"):
            t = st[key]
            old.append(t.data)
            after_1.append(t.data.clone())
            t.data = t.clone()
            assert st[key] is t and t.data_ptr() != old[-1].data_ptr()
    give(ps, shadows, 2)
    opt.step()
    check(ps, opt, shadows, "update 2 with the moments in new storage")
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(old, after_1)), "the old storage was written"


@pytest.mark.parametrize("n,absent,order", [(2, {1: (1, 2)}, [1, 0]), (3, {1: (1,), 2: (1, 2)}, [1, 2, 0]), (3, {1: (1,), 2: (1, 2)}, [2, 0, 1])],
                         ids=["swap_of_two", "rotation_of_three", "rotation_the_other_way"])
def test_reorder_at_different_counts(n, absent, order):
    """``absent``: parameter -> the updates it has no gradient at.  After three updates the parameters stand at distinct counts; the
    group is reordered; in the next update everyone takes ITS next update number."""
    ps, opt, shadows = make(n)
    for k in (1, 2, 3):
        give(ps, shadows, k, only=[i for i in range(n) if k not in absent.get(i, ())])
        opt.step()
    counts = [s.t for s in shadows]
    assert len(set(counts)) == n and counts[0] == 3
    check([p for p, s in zip(ps, shadows) if s.t], opt, [s for s in shadows if s.t], "before the reorder")
    group = opt.param_groups[0]
    group["params"] = [ps[i] for i in order]
    ps, shadows = [ps[i] for i in order], [shadows[i] for i in order]
    for k in (1, 2):                                                     # gradients for everyone, twice: the counts stay apart
        give(ps, shadows, k)
        opt.step()
        assert sorted(s.t for s in shadows) == sorted(t + k for t in counts)
        check(ps, opt, shadows, f"update {k} after the reorder")


def test_append_to_a_group(monkeypatch):
    calls = []
    real = _lib.adam_step
    monkeypatch.setattr(_lib, "adam_step", lambda table, n, h, dev: (calls.append((n, h.step)), real(table, n, h, dev))[1])
    every, _, shadows = make()
    ps = every[:3]
    c = R.CASES[NAME]
    opt = optim.Adam(ps, lr=c["lr"], betas=c["betas"], eps=c["eps"])
    for k in (1, 2):
        give(ps, shadows[:3], k)
        opt.step()
    assert calls == [(3, 1), (3, 2)]
    opt.param_groups[0]["params"].append(every[3])
    give(every, shadows, 3)
    opt.step()
    assert calls[2:] == [(3, 3), (1, 1)]
    check(every, opt, shadows, "update 3, the appended parameter's first")
    give(every, shadows, 1)
    opt.step()
    assert calls[4:] == [(3, 4), (1, 2)]
    check(every, opt, shadows, "update 4, the appended parameter's second")


def test_misaligned_parameter_is_refused_by_name_with_nothing_written():
    c = R.CASES[NAME]
    big = torch.from_numpy(R.params("around_a_chunk")[0][:12].copy()).cuda()
    before = big.clone()
    p = torch.nn.Parameter(big[1:7])
    assert p.is_contiguous() and p.data_ptr() % 16 == 4
    p.grad = torch.ones(6, device="cuda")
    every, _, shadows = make()
    q, shadow = every[3], shadows[3]
    opt = optim.Adam([{"params": [q]}, {"params": [p]}], lr=c["lr"], betas=c["betas"], eps=c["eps"])
    give([q], [shadow], 1)
    with pytest.raises(ValueError, match=r"parameter 0 of the group \(shape \(6,\)\) is not 16-byte aligned"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(big.view(torch.int32), before.view(torch.int32))
    st = opt.state[p]
    assert len(st) == 0 or float(st["step"]) == 0
    check([q], opt, [shadow], "the group before the refused one: updated once, as torch steps group by group")
    assert shadow.t == 1
