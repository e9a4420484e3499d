"""What holds of the ``WIDE`` cases of tests/adam_ref.py without a GPU: the numpy restatement of ``include/vqcpc.h``'s order is
within the project's judge of ``torch.optim.Adam`` in float64 on every one of them (the ladders per tensor), and the cases hold
what they were written to hold -- a full table of mixed sizes, a second launch behind empty tensors with a tensor of several
chunks in it, every loop count and tail length of a last chunk, gradients from the contract's floor to the largest whose square is
finite, both signs of zero.
"""
import numpy as np
import pytest

import adam_ref as R


@pytest.mark.parametrize("name", list(R.WIDE))
def test_restatement_within_the_judge_of_float64_adam(name):
    ref64, ref32 = R.reference(name)
    mine = R.restated(name)
    assert len(mine) == R.WIDE[name]["steps"]
    worst = 0.0
    for k, (got, r64, r32) in enumerate(zip(mine, ref64, ref32), 1):
        worst = max(worst, R.judge_snapshot(name, k, got, r64, r32, "restatement"))
    print(f"{name}: largest err / bound over {len(mine)} updates = {worst:.3f}")
    assert worst <= 1.0


def chunks(n):
    return -(-n // R.CHUNK)


def test_wide_cases_hold_what_they_are_meant_to_hold():
    C, T, W = R.CHUNK, R.TABLE, R.WIDE
    assert set(W) == {"full_table_mixed", "two_launches_mixed", "tails", "eps_1e-3", "eps_0", "beta2_0", "betas_near_1", "lr_1", "negzero",
                      "ladder_cold", "ladder_loaded"} and not set(W) & set(R.CASES)
    # a full table: a tensor with elements at every index 0..T-1, one launch, an irregular chunk prefix
    mixed = W["full_table_mixed"]["numels"]
    assert len(mixed) == T and all(mixed) and sum(mixed) == 166041 and R.launches(mixed) == [mixed]
    assert {chunks(n) for n in mixed} == {1, 2, 3} and [chunks(n) for n in mixed[:8]] == [1, 1, 2, 1, 3, 1, 1, 1]
    # two launches: the second one starts behind an empty tensor and holds a tensor with several chunks
    two = W["two_launches_mixed"]["numels"]
    split = R.launches(two)
    assert len(split) == 2 and split[0] == mixed and len(split[1]) >= 1 and max(chunks(n) for n in split[1]) > 1
    at = [i for i, n in enumerate(two) if n][T]                      # the list index of the second launch's first tensor
    assert two[0] == 0 and two[at - 1] == 0 and two[-1] == 0 and two.count(0) == 5
    # the last chunk of a tensor: every loop count around the 256 threads, with every tail length
    last = [n % C for n in W["tails"]["numels"]]
    assert all(n < C for n in W["tails"]["numels"])
    assert {n // 4 for n in last} >= {0, 1, 255, 256, 257, 512, 1022, 1023} and {n % 4 for n in last} == {0, 1, 2, 3}
    assert {(n // 4, n % 4) for n in last} >= {(0, 2), (256, 1), (256, 2), (256, 3), (257, 1), (512, 2)}
    # hyper-parameters at their edges
    assert W["eps_0"]["eps"] == 0.0 and not W["eps_0"]["kinds"] and W["eps_1e-3"]["eps"] == 1e-3
    assert W["beta2_0"]["betas"] == (0.9, 0.0) and W["betas_near_1"]["betas"] == (0.999, 0.999999) and W["lr_1"]["lr"] == 1.0
    # the ladder: the contract's floor at the bottom, the largest finite square at the top, a warm state of each rung's own scale
    for name in ("ladder_cold", "ladder_loaded"):
        c = W[name]
        assert c["numels"] == [1029] * 34 and c["per_tensor"] and c["scale"][0] == 2e-14
        assert all(abs(s / 10.0 ** e - 1.0) < 1e-12 for s, e in zip(c["scale"][1:], range(-13, 20)))
    assert W["ladder_cold"]["first"] == 1 and W["ladder_loaded"]["first"] == 50000
    m, v = R.start_state("ladder_loaded")
    for i, s in enumerate(W["ladder_loaded"]["scale"]):
        assert 0.01 * s <= np.abs(m[i]).max() <= 0.1 * s and 0.015 * s * s * 0.999 <= v[i].min() and v[i].max() <= 0.3 * s * s * 1.001
    # the contract over every gradient of every case: |g| >= 1e-15 or exactly 0, g * g finite in fp32
    low, top = np.inf, 0.0
    for name, c in W.items():
        for k in range(1, c["steps"] + 1):
            for g in R.grads(name, k):
                assert g.dtype == np.float32
                nz = g[g != 0]
                if nz.size:
                    low = min(low, float(np.abs(nz).min()))
                    top = max(top, float((nz * nz).max()))               # an fp32 product: inf where it overflows
                if c["kinds"].get(k) is None:
                    assert nz.size == g.size
    print(f"min |g| = {low:.3g}, max g * g = {top:.3g} over every gradient of WIDE")
    assert low >= 1e-15 and np.isfinite(top) and low < 1e-14 and top > 1e37
    # both signs of zero, at the places "negzero" names
    assert W["negzero"]["kinds"] == {1: "negzero", 3: "negzero"}
    for k in (1, 3):
        for g in R.grads("negzero", k):
            zero = g == 0
            assert zero[::2].all() and not zero[1::2].any()
            assert (np.signbit(g[zero]) == (np.flatnonzero(zero) % 4 == 2)).all() and np.signbit(g[zero]).any() and not np.signbit(g[zero]).all()
    assert all(g.all() for g in R.grads("negzero", 2))
