"""What holds of the optimizer step without a GPU: the numpy restatement of ``include/vqcpc.h``'s order against
``torch.optim.Adam`` in float64 (the project's judge, tests/grad_judge.py), ``optim.Adam``'s torch surface on the CPU,
``optim.WarmupScheduler`` against the learning rates recorded from the reference's scheduler (tests/golden/warmup_lrs.json,
tools/gen_sched_golden.py), and the host half of ``vqcpc_adam_step`` -- its argument validation runs
before any HIP call, so every ``VQCPC_ERR_INVALID`` the host can see is returned here as well.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import adam_ref as R
from vectorquantizedcpc_amd import _lib, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement, judged
@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_within_the_judge_of_float64_adam(name):
    ref64, ref32 = R.reference(name)
    mine = R.restated(name)
    worst = 0.0
    for k, (got, r64, r32) in enumerate(zip(mine, ref64, ref32), 1):
        worst = max(worst, R.judge_snapshot(name, k, got, r64, r32, "restatement"))
    print(f"{name}: largest err / bound over {len(mine)} updates = {worst:.3f}")


def test_cases_cover_what_the_kernel_can_get_wrong():
    sizes = {n for c in R.CASES.values() for n in c["numels"]}
    assert {1, 3, 4, 5, R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK + 3, 0} <= sizes
    assert any(len(c["numels"]) == R.TABLE + 1 for c in R.CASES.values())
    assert R.CASES["predictors"]["numels"] == [64 * 256, 64] * 12
    assert {c["scale"] for c in R.CASES.values()} >= {1e-6, 1e-3, 1.0, 1e3}
    assert {c["steps"] for c in R.CASES.values()} >= {1, 3, 20}
    assert any(c["first"] == 10000 for c in R.CASES.values()) and any(c["lr"] == 0.0 for c in R.CASES.values())
    assert {c["betas"] for c in R.CASES.values()} == {R.REF_BETAS, (0.0, 0.5)}
    kinds = {k for c in R.CASES.values() for k in c["kinds"].values()}
    assert kinds == {"half", "zero"}
    header = open(os.path.join(ROOT, "include", "vqcpc.h")).read()
    assert int(re.search(r"#define VQCPC_ADAM_CHUNK (\d+)", header).group(1)) == R.CHUNK
    assert int(re.search(r"#define VQCPC_ADAM_TABLE (\d+)", header).group(1)) == R.TABLE
    for name, c in R.CASES.items():                      # g * g stays a normal fp32 number, or g is exactly 0
        for k in range(1, c["steps"] + 1):
            for g in R.grads(name, k):
                nz = g[g != 0]
                assert nz.size == 0 or np.abs(nz).min() >= 1e-15
            if c["kinds"].get(k) == "half":
                assert all((g[::2] == 0).all() and (g[1::2] != 0).all() for g in R.grads(name, k))
            if c["kinds"].get(k) == "zero":
                assert k > 1 and not any(g.any() for g in R.grads(name, k))


# ------------------------------------------------------------------------------------------------ optim.Adam on the CPU
def _params():
    torch.manual_seed(3)
    return [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]


def test_adam_surface_is_torchs():
    ours, theirs = optim.Adam(_params(), lr=4e-4), torch.optim.Adam(_params(), lr=4e-4)
    assert isinstance(ours, torch.optim.Adam)
    assert list(ours.param_groups[0].keys()) == list(theirs.param_groups[0].keys())
    assert {k: v for k, v in ours.param_groups[0].items() if k != "params"} == {k: v for k, v in theirs.param_groups[0].items() if k != "params"}
    assert ours.state_dict().keys() == theirs.state_dict().keys()
    assert [n for n in vars(optim.Adam) if not n.startswith("_")] == ["step"]        # step() is the one public override


def test_state_dict_loads_both_ways_on_the_cpu():
    ps = _params()
    theirs = torch.optim.Adam(ps, lr=1e-3, betas=(0.8, 0.99), eps=1e-6)
    for p in ps:
        p.grad = torch.ones_like(p)
    theirs.step()
    theirs.step()
    sd = theirs.state_dict()
    ours = optim.Adam(_params(), lr=4e-4)
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert back["state"].keys() == sd["state"].keys()
    for i in sd["state"]:
        assert back["state"][i].keys() == sd["state"][i].keys() == {"step", "exp_avg", "exp_avg_sq"}
        for k in sd["state"][i]:
            assert torch.equal(back["state"][i][k], sd["state"][i][k]) and back["state"][i][k].dtype == sd["state"][i][k].dtype
    again = torch.optim.Adam(_params(), lr=1.0)
    again.load_state_dict(back)
    assert float(again.state[again.param_groups[0]["params"][1]]["step"]) == 2.0 and again.param_groups[0]["betas"] == (0.8, 0.99)


@pytest.mark.parametrize("kw", [{"weight_decay": 1e-2}, {"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}])
def test_rejected_options_raise(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        optim.Adam(_params(), lr=4e-4, **kw)


def test_rejected_options_raise_at_step_when_a_group_brings_them():
    ours = optim.Adam(_params(), lr=4e-4)
    ours.param_groups[0]["weight_decay"] = 0.1
    with pytest.raises(ValueError, match="weight_decay"):
        ours.step()


def test_step_on_cpu_parameters_has_no_fallback():
    ps = _params()
    ours = optim.Adam(ps, lr=4e-4)
    before = [p.detach().clone() for p in ps]
    ours.step()                                          # no gradient anywhere: nothing to do, nothing raised
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ours.step()
    assert all(torch.equal(p, b) for p, b in zip(ps, before))


# ------------------------------------------------------------------------------------------------ the schedule
def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "warmup_lrs.json")) as f:
        return json.load(f)["cases"]


def _scheduler_scalars(sched):
    sd = sched.state_dict()
    return {"last_epoch": sd["last_epoch"], "_step_count": sd["_step_count"], "_last_lr": list(sd["_last_lr"]), "base_lrs": list(sd["base_lrs"]),
            "warmup_epochs": sd["warmup_epochs"], "gamma": sd["gamma"], "milestones": {str(k): v for k, v in sorted(sd["milestones"].items())}}


def _same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), (a, b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, float):
        assert abs(a - b) <= 1e-15 * abs(b), (a, b)
    else:
        assert a == b, (a, b)


@pytest.mark.parametrize("name", ["example", "config", "repeated_milestone", "resume"])
def test_warmup_scheduler_gives_the_recorded_learning_rates(name):
    case = _golden()[name]
    args = case["args"]

    def make():
        opt = optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=args[1])
        return opt, optim.WarmupScheduler(opt, *args)

    opt, sched = make()
    lrs = []
    for e in range(case["n_epochs"]):
        if case["resume_after"] is not None and e == case["resume_after"]:
            _same(_scheduler_scalars(sched), case["state_at_resume"])
            saved = {"optimizer": opt.state_dict(), "scheduler": sched.state_dict()}
            opt, sched = make()
            opt.load_state_dict(saved["optimizer"])
            sched.load_state_dict(saved["scheduler"])
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()                                       # no gradient: the order torch asks for, nothing to compute
        sched.step()
    assert len(case["epochs"]) == len(case["lrs"]) >= min(case["n_epochs"], 160)
    for e, want in zip(case["epochs"], case["lrs"]):
        assert abs(lrs[e] - want) <= 1e-15 * want, (name, e, lrs[e], want)
    _same(_scheduler_scalars(sched), case["state_at_end"])


def test_warmup_scheduler_example_by_hand():
    lrs = dict(zip(_golden()["example"]["epochs"], _golden()["example"]["lrs"]))
    assert lrs[0] == 1e-6 and abs(lrs[1] - 8.08e-5) < 1e-18 and [lrs[e] for e in (5, 6, 7)] == [4e-4] * 3
    assert [lrs[e] for e in (8, 9, 10, 11)] == [1e-4] * 4 and lrs[12] == 2.5e-5


def test_warmup_scheduler_state_dict_round_trips_and_bad_arguments_raise():
    opt = optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=1e-6)
    sched = optim.WarmupScheduler(opt, 5, 1e-6, 4e-4, [8, 12], 0.25)
    for _ in range(9):
        opt.step()
        sched.step()
    sd = sched.state_dict()
    assert "optimizer" not in sd
    opt2 = optim.Adam([torch.nn.Parameter(torch.zeros(2))], lr=1e-6)
    sched2 = optim.WarmupScheduler(opt2, 1, 0.5, 0.7, [3])          # the checkpoint's order: both made, then both loaded
    opt2.load_state_dict(opt.state_dict())
    sched2.load_state_dict(sd)
    assert sched2.state_dict() == sd and opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == 1e-4
    with pytest.raises(ValueError):
        optim.WarmupScheduler(opt, 8, 1e-6, 4e-4, [8, 12])
    with pytest.raises(ValueError):
        optim.WarmupScheduler(opt, 5, [1e-6, 1e-6], 4e-4, [8, 12])


# ------------------------------------------------------------------------------------------------ the library
def test_invalid_arguments_are_refused_before_any_hip_call():
    """The validation of ``vqcpc_adam_step`` is host arithmetic that runs first: with made-up (never read) addresses every
    ``VQCPC_ERR_INVALID`` the host can see comes back on a machine without a GPU too."""
    lib = _lib.load()
    good = dict(lr=4e-4, beta1=0.9, beta2=0.999, eps=1e-8, step=1)

    def call(rows, n=None, tensors_null=False, hyper_null=False, **h):
        table = (_lib.AdamTensor * max(len(rows), 1))(*[_lib.AdamTensor(*r) for r in rows])
        hy = _lib.AdamHyper(**{**good, **h})
        return lib.vqcpc_adam_step(None if tensors_null else table, len(rows) if n is None else n, None if hyper_null else C.byref(hy), None)

    row = (0x10000, 0x20000, 0x30000, 0x40000, 8)
    bad = [call([row], tensors_null=True), call([row], hyper_null=True), call([row], n=0), call([row], n=-1),
           call([row], step=0), call([row], step=-5), call([row], lr=-1.0), call([row], lr=float("nan")), call([row], lr=float("inf")),
           call([row], eps=-1.0), call([row], eps=float("nan")), call([row], eps=float("inf")),
           call([row], beta1=1.0), call([row], beta1=-0.1), call([row], beta1=float("nan")),
           call([row], beta2=1.0), call([row], beta2=-0.1), call([row], beta2=float("nan"))]
    for member in range(4):
        for value in (None, row[member] + 4, row[member] + 8):
            r = list(row)
            r[member] = value
            bad.append(call([tuple(r)]))
            bad.append(call([(0, 0, 0, 0, 0), tuple(r)]))            # behind an empty tensor
    assert bad == [-1] * len(bad), bad
    assert b"vqcpc_adam_step" in lib.vqcpc_last_error()
