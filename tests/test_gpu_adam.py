"""-m gpu: ``vqcpc_adam_step`` (``csrc/optim.hip``) through ``optim.Adam`` -- its bits against the numpy restatement of
``include/vqcpc.h``'s order after every update of every case of tests/adam_ref.py, the same outputs against
``torch.optim.Adam`` in float64 by the project's judge, what must stay untouched (a parameter without a gradient, a cold state under
an all-zero gradient, canaries around every buffer, every buffer after a refused call), state dicts moving between the two
optimizers, and one library call per ``step()`` per param group.

Nothing here is measured on the code under test: the restatement is numpy's, the judge's ``e_ref`` is torch's own fp32 run on the
CPU (tests/adam_ref.py computes both).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as R
from adam_ref import arena_case, bits, hyper                       # the arena of canaries: shared with tests/test_gpu_adam_wide.py
from vectorquantizedcpc_amd import _lib, optim

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1. the kernel's bits are the restatement's; 2. the judge
@pytest.mark.parametrize("name", list(R.CASES))
def test_bits_equal_the_restatement_and_float64_judges_them(name):
    want = R.restated(name)
    ref64, ref32 = R.reference(name)
    got = R.run_torch(name, torch.float32, "cuda", optim.Adam)
    assert len(got) == len(want) == R.CASES[name]["steps"]
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want), 1):
        for key in R.KEYS:
            for i, (a, b) in enumerate(zip(g[key], w[key])):
                diff = np.flatnonzero(bits(a) != bits(b))
                assert diff.size == 0, (f"{name}: update {k}, {key} of tensor {i} ({a.size} elements): {diff.size} elements differ, first at "
                                        f"{diff[0]}: {a.reshape(-1)[diff[0]]!r} != {b.reshape(-1)[diff[0]]!r}")
        worst = max(worst, R.judge_snapshot(name, k, g, ref64[k - 1], ref32[k - 1], "vqcpc_adam_step"))
    print(f"{name}: bit for bit the restatement over {len(got)} updates; largest err / bound against float64 = {worst:.3f}")


# ------------------------------------------------------------------ 3. what a step leaves alone
def test_a_parameter_without_a_gradient_is_untouched():
    ps = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in R.params("vector_and_tail")]
    opt = optim.Adam(ps, lr=R.LR)
    for step in (1, 2):
        before = [p.detach().clone() for p in ps]
        versions = [p._version for p in ps]
        for i, (p, g) in enumerate(zip(ps, R.grads("vector_and_tail", step))):
            p.grad = None if i == 2 else torch.from_numpy(g).cuda()
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(ps[2].view(torch.int32), before[2].view(torch.int32)) and ps[2]._version == versions[2]
        assert len(opt.state[ps[2]]) == 0
        for i in (0, 1, 3):
            assert not torch.equal(ps[i], before[i]) and ps[i]._version > versions[i]      # the native handles key on _version
            assert float(opt.state[ps[i]]["step"]) == step
    # the parameter joins late: its own count starts at 1 while the others stand at 3 -- two calls, each with its own update number
    for p, g in zip(ps, R.grads("vector_and_tail", 3)):
        p.grad = torch.from_numpy(g).cuda()
    opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [3.0, 3.0, 1.0, 3.0]
    want = R.params("vector_and_tail")[2]
    m, v = np.zeros_like(want), np.zeros_like(want)
    R.update(want, R.grads("vector_and_tail", 3)[2], m, v, R.scalars(R.LR, *R.REF_BETAS, R.EPS, 1))
    assert np.array_equal(bits(ps[2].detach().cpu().numpy()), bits(want))
    assert np.array_equal(bits(R.restated("vector_and_tail")[2]["p"][0]), bits(ps[0].detach().cpu().numpy()))


def test_all_zero_gradient_on_a_cold_state_changes_no_bit():
    p0 = np.concatenate([R.params("around_a_chunk")[3], np.array([-0.0, 0.0, -1.0], np.float32)])
    p = torch.nn.Parameter(torch.from_numpy(p0).cuda())
    p.grad = torch.zeros_like(p)
    opt = optim.Adam([p], lr=R.LR)
    opt.step()
    st = opt.state[p]
    assert np.array_equal(bits(p.detach().cpu().numpy()), bits(p0))
    assert not bits(st["exp_avg"].cpu().numpy()).any() and not bits(st["exp_avg_sq"].cpu().numpy()).any()     # +0, not -0
    assert float(st["step"]) == 1.0


# ------------------------------------------------------------------ 4. canaries; 5. refused calls
@pytest.mark.parametrize("name", ["vector_and_tail", "around_a_chunk", "second_launch", "loaded_at_10000"])
def test_canaries_around_every_buffer_keep_their_bits(name):
    arena, table, n, arrays = arena_case(name)
    _lib.adam_step(table, n, hyper(name), torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    words = arena.read()
    assert arena.canaries_intact(words)
    want = R.restated(name)[0]
    live = [i for i, a in enumerate(R.params(name)) if a.size]
    for j, i in enumerate(live):
        assert np.array_equal(bits(arena.array(words, 4 * j)), bits(want["p"][i])), (name, i)
        assert np.array_equal(bits(arena.array(words, 4 * j + 1)), bits(arrays[4 * j + 1])), (name, i, "the gradient was written")
        assert np.array_equal(bits(arena.array(words, 4 * j + 2)), bits(want["exp_avg"][i])), (name, i)
        assert np.array_equal(bits(arena.array(words, 4 * j + 3)), bits(want["exp_avg_sq"][i])), (name, i)


def test_every_invalid_argument_is_refused_with_nothing_written():
    name = "vector_and_tail"
    arena, table, n, _ = arena_case(name)
    lib, s = _lib.load(), _lib.current_stream()
    before = arena.read().copy()
    INVALID = -1

    def call(tab=table, count=n, h=None, hyper_null=False):
        h = h if h is not None else hyper(name)
        return lib.vqcpc_adam_step(tab, count, None if hyper_null else C.byref(h), s)

    def with_member(i, member, value):
        tab = (_lib.AdamTensor * n)(*[_lib.AdamTensor(t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.numel) for t in table])
        setattr(tab[i], member, value)
        return tab

    got = [call(tab=None), call(hyper_null=True), call(count=0), call(count=-2)]
    assert b"null argument" in lib.vqcpc_last_error() or b"n_tensors" in lib.vqcpc_last_error()
    for member in ("param", "grad", "exp_avg", "exp_avg_sq"):
        for i in (0, n - 1):
            got.append(call(tab=with_member(i, member, None)))
            assert b"null member" in lib.vqcpc_last_error()
            got.append(call(tab=with_member(i, member, getattr(table[i], member) + 4)))
            assert b"16-byte aligned" in lib.vqcpc_last_error()
    got += [call(h=hyper(name, step=0)), call(h=hyper(name, step=-1))]
    assert b"step" in lib.vqcpc_last_error()
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        got += [call(h=hyper(name, lr=bad)), call(h=hyper(name, eps=bad))]
    for bad in (1.0, -0.5, 2.0, float("nan")):
        got += [call(h=hyper(name, beta1=bad)), call(h=hyper(name, beta2=bad))]
    host = np.zeros(64, np.float32)                                      # page-aligned host memory is not memory of the device
    base = (host.ctypes.data + 15) // 16 * 16
    got.append(call(tab=with_member(0, "param", base)))
    assert b"current device" in lib.vqcpc_last_error()
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            got.append(call())
    torch.cuda.synchronize()
    assert got == [INVALID] * len(got), got
    assert np.array_equal(arena.read(), before)
    # an empty tensor's members are not looked at; and the call as it stands is accepted
    tab = with_member(1, "numel", 0)
    for member in ("param", "grad", "exp_avg", "exp_avg_sq"):
        setattr(tab[1], member, None)
    assert call(tab=tab) == 0
    torch.cuda.synchronize()
    words = arena.read()
    assert arena.canaries_intact(words) and np.array_equal(arena.array(words, 4), arena.array(before, 4))
    assert not np.array_equal(arena.array(words, 0), arena.array(before, 0))


# ------------------------------------------------------------------ 6. step-time rejections name the tensor
def test_step_refuses_what_the_kernel_does_not_take():
    def one(p, g, **kw):
        p = torch.nn.Parameter(p)
        p.grad = g
        return optim.Adam([{"params": [p], **kw}], lr=R.LR), p

    opt, p = one(torch.zeros(4, 6, device="cuda", dtype=torch.float16), torch.zeros(4, 6, device="cuda", dtype=torch.float16))
    with pytest.raises(TypeError, match=r"parameter 0 of the group \(shape \(4, 6\)\) is torch.float16"):
        opt.step()
    opt, p = one(torch.zeros(4, 6, device="cuda"), torch.zeros(6, 4, device="cuda").t())
    with pytest.raises(ValueError, match=r"the gradient of parameter 0 .* is not contiguous"):
        opt.step()
    opt, p = one(torch.zeros(4, 6, device="cuda"), torch.zeros(4, 6, device="cuda").to_sparse())
    with pytest.raises(TypeError, match=r"the gradient of parameter 0 .* is torch.sparse_coo"):
        opt.step()
    opt, p = one(torch.zeros(6, 4, device="cuda").t(), torch.zeros(4, 6, device="cuda"))
    with pytest.raises(ValueError, match=r"parameter 0 .* is not contiguous"):
        opt.step()
    torch.cuda.synchronize()
    assert not p.detach().any() and len(opt.state[p]) == 0


# ------------------------------------------------------------------ 7. state dicts move between the two optimizers
@pytest.mark.parametrize("first,second", [(torch.optim.Adam, optim.Adam), (optim.Adam, torch.optim.Adam)])
def test_state_dict_interchange_mid_run(first, second):
    name, k = "betas_0_0.5", 5
    c = R.CASES[name]
    assert c["steps"] >= 2 * k
    ps = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in R.params(name)]

    def run(opt, steps):
        for s in steps:
            for p, g in zip(ps, R.grads(name, s)):
                p.grad = torch.from_numpy(g).cuda()
            opt.step()

    a = first(ps, lr=c["lr"], betas=c["betas"], eps=c["eps"])
    run(a, range(1, k + 1))
    sd = a.state_dict()
    b = second(ps, lr=1.0, betas=(0.5, 0.5), eps=1.0)                    # everything comes from the state dict
    b.load_state_dict(sd)
    run(b, range(k + 1, 2 * k + 1))
    torch.cuda.synchronize()
    assert [float(b.state[p]["step"]) for p in ps] == [2.0 * k] * len(ps)
    got = {"p": [p.detach().cpu().numpy() for p in ps], "exp_avg": [b.state[p]["exp_avg"].cpu().numpy() for p in ps],
           "exp_avg_sq": [b.state[p]["exp_avg_sq"].cpu().numpy() for p in ps]}
    ref64, ref32 = R.reference(name)
    ratio = R.judge_snapshot(name, 2 * k, got, ref64[2 * k - 1], ref32[2 * k - 1], f"{first.__module__} -> {second.__module__}")
    assert ratio <= 1.0


# ------------------------------------------------------------------ 8. one library call per step() per group
def test_one_call_per_step_per_group(monkeypatch):
    calls = []
    real = _lib.adam_step
    monkeypatch.setattr(_lib, "adam_step", lambda table, n, h, dev: (calls.append((n, h.step, h.lr)), real(table, n, h, dev))[1])
    arrays = R.params("predictors")
    ps = [torch.nn.Parameter(torch.from_numpy(a).cuda()) for a in arrays]
    opt = optim.Adam(ps, lr=R.LR)
    opt.add_param_group({"params": [torch.nn.Parameter(torch.ones(5, device="cuda"))], "lr": 1e-2})
    for step in (1, 2, 3):
        for p in ps + opt.param_groups[1]["params"]:
            p.grad = torch.ones_like(p)
        opt.step()
        assert calls[-2:] == [(24, step, R.LR), (1, step, 1e-2)] and len(calls) == 2 * step
    opt.zero_grad(set_to_none=True)
    opt.step()                                                           # no gradient anywhere: no call
    assert len(calls) == 6
