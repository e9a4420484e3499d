"""CPU checks of tests/vocoder_size_cases.py: the judge that tests/test_gpu_vocoder_sizes.py applies to the GPU rests on nothing the
GPU does.  Per case (model size):

1. The table covers every size vqcpc_vocoder_create accepts; teacher-forced inputs of the 9 / 10 bit cases use the upper classes.
2. The fp32 yardstick passes the judge against float64: conditioning, teacher-forced logits, and its own free-running draws on
   every input set the GPU test decodes (none outside W, at least 99 % exact).
3. A ragged batch equals its utterances run alone (float64, 1e-12).
4. Seeded faults, built on the yardstick, are rejected: the conditioning frame taken as t // 160; the sample index masked to
   8 bits before the embedding lookup (9 / 10 bit); fc2 summed over its first 512 inputs only (size_h_fc > 512); the backward
   prenet GRU started at the padded end of a ragged row.
"""
import copy

import numpy as np
import pytest
import torch

import nll_ref
import vocoder_size_cases as S


def test_table_covers_every_accepted_size():
    seen = {k: {S.CASES[n][k] for n in S.NAMES} for k in ("bits", "h_fc", "h_rnn", "hp")}
    assert seen["bits"] == {8, 9, 10} and seen["h_fc"] == {256, 512, 768, 1024}
    assert seen["h_rnn"] == {512, 896, 1024} and seen["hp"] == {64, 128, 256, 512}
    for n in S.NAMES:
        c = S.CASES[n]
        assert c["embed_ar"] % 32 == 0 and (c["dz"] + c["ds"]) % 32 == 0 and c["up"] > 0
    assert {S.CASES[n]["embed_ar"] for n in S.NAMES} >= {32, 96, 512} and {S.CASES[n]["dz"] + S.CASES[n]["ds"] for n in S.NAMES} >= {32, 96, 256}
    assert len({S.CASES[n]["up"] for n in S.NAMES}) == len(S.NAMES)          # no two cases share a hop length
    for n in S.RESIDENT:
        assert (S.CASES[n]["h_rnn"], S.CASES[n]["h_fc"], S.CASES[n]["bits"]) == (896, 256, 8)


@pytest.mark.parametrize("name", S.NAMES)
def test_yardstick_passes_conditioning_and_logits(name):
    want = S.cond_reference(name)
    got = S.cond_reference(name, S.f32(name))
    for Tc in S.COND_TC:
        assert S.judge_cond(name, got[Tc], want[Tc], "yardstick Tc %d" % Tc)[0]
    for which in ("b2", "b17"):
        x = S.tf_inputs(name, which)[2]
        if S.CASES[name]["bits"] > 8:
            assert int((x >= S.n_cls(name) // 2).sum()) > x.numel() // 4          # the upper classes are fed in
        assert S.judge_logits(name, S.tf_reference(name, which, S.f32(name)), S.tf_reference(name, which), what="yardstick " + which)[0]
    e32, tol, m = S.tolerances(name)["logit"]
    assert tol == 10.0 * max(e32, S.ULP1 * m) and 0.0 < tol < 1e-4


def _draw_sets(name):
    """The free runs of tests/test_gpu_vocoder_sizes.py: (utterances, rows checked)."""
    sizes = [3, 20] + ([80] if name in S.BIG else []) + ([5, 12, 32, 19] if name in S.RESIDENT else [])
    return [(B, S.draw_rows(B)) for B in sizes]


@pytest.mark.parametrize("name", S.NAMES)
def test_yardstick_draws_meet_the_share(name):
    """The 99 % share of exact draws is a condition on the inputs, met by fp32 on the CPU before any GPU draw is looked at."""
    y = S.f32(name)
    for B, rows in _draw_sets(name):
        z, spk, n_codes, ids = S.draw_inputs(name, B)
        cond = y.condition(z[rows], spk[rows], [n_codes[b] for b in rows])
        mu = np.zeros((B, 2 * S.CASES[name]["up"] * max(n_codes)), np.int64)
        s, _ = y.generate(cond, S.SEED, [ids[b] for b in rows])
        mu[rows, : s.shape[1]] = s.numpy()
        ok, exact, gap, bad, n = S.judge_draws(name, mu, z, spk, n_codes, ids, rows=rows, what="yardstick B %d" % B)
        assert ok, (B, exact, bad)
        if S.CASES[name]["bits"] > 8:
            assert int((mu[rows] >= S.n_cls(name) // 2).sum()) > 0


@pytest.mark.parametrize("name", S.NAMES)
def test_ragged_batch_equals_utterances_alone(name):
    f, up = S.f64(name), S.CASES[name]["up"]
    z, spk, n_codes, _ = S.draw_inputs(name, 3)
    cond = f.condition(z, spk, n_codes)
    lens = [2 * up * n for n in n_codes]
    x = S.tf_inputs(name, "b17")[2][:3, : max(lens)]
    if x.shape[1] < max(lens):
        x = torch.cat([x] * (max(lens) // x.shape[1] + 1), dim=1)[:, : max(lens)]
    lg = f.logits(x, cond, lens).numpy()
    for b in range(3):
        one = f.condition(z[b:b + 1, : n_codes[b]], spk[b:b + 1])[0]
        assert one.shape == cond[b].shape and float((one - cond[b]).abs().max()) <= 1e-12
        lg1 = f.logits(x[b:b + 1, : lens[b]], [one]).numpy()
        assert float(np.abs(lg1[0] - lg[b, : lens[b]]).max()) <= 1e-12 and not lg[b, lens[b]:].any()


# ---------------------------------------------------------------------- seeded faults
@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n]["up"] != 160])
def test_fault_frame_taken_as_t_over_160(name):
    y = S.f32(name)
    z, spk, x = S.tf_inputs(name, "b2")
    cond = y.condition(z, spk)
    need = (x.shape[1] + 159) // 160
    padded = [torch.cat([c, c[-1:].expand(max(need - c.shape[0], 0), -1)]) for c in cond]      # a hop of 160 runs past the frames
    wrong = copy.copy(y)
    wrong.up = 160
    ok, err = S.judge_logits(name, wrong.logits(x, padded).numpy(), S.tf_reference(name, "b2"), what="fault t // 160")
    assert not ok


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n]["bits"] > 8])
def test_fault_sample_index_masked_to_8_bits(name):
    y = S.f32(name)
    z, spk, x = S.tf_inputs(name, "b2")
    ok, err = S.judge_logits(name, y.logits(x & 255, y.condition(z, spk)).numpy(), S.tf_reference(name, "b2"), what="fault x & 255")
    assert not ok


@pytest.mark.parametrize("name", [n for n in S.NAMES if S.CASES[n]["h_fc"] > 512])
def test_fault_fc2_over_the_first_512_inputs(name):
    y = S.f32(name)
    wrong = copy.copy(y)
    wrong.fc2_w = y.fc2_w.clone()
    wrong.fc2_w[:, 512:] = 0.0
    z, spk, x = S.tf_inputs(name, "b2")
    ok, err = S.judge_logits(name, wrong.logits(x, y.condition(z, spk)).numpy(), S.tf_reference(name, "b2"), what="fault fc2[:512]")
    assert not ok


@pytest.mark.parametrize("name", S.NAMES)
def test_fault_backward_gru_from_the_padded_end(name):
    y, f = S.f32(name), S.f64(name)
    z, spk, n_codes, _ = S.draw_inputs(name, 3)
    b = min(range(3), key=lambda i: n_codes[i])
    assert n_codes[b] < z.shape[1]
    want = f.condition(z, spk, n_codes)[b].numpy()
    padded = y.condition(z, spk)[b][: 2 * n_codes[b]].numpy()
    assert not S.judge_cond(name, padded, want, "fault padded end")[0]
    assert S.judge_cond(name, y.condition(z, spk, n_codes)[b].numpy(), want, "ragged row, proper")[0]


# ---------------------------------------------------------------------- the scoring reference at other sizes
@pytest.mark.parametrize("name", ["hr1024", "hr512_refhead"])
def test_nll_reference_takes_a_state_dict(name):
    """nll_ref.Ref on a state dict and upsample: equal to log_softmax of the case's own float64 logits, and at the reference's
    sizes equal to the named weight set's Ref."""
    c = S.nll_inputs(name)
    tol = S.tolerances(name)["logit"][1]
    ref = nll_ref.Ref(name, c["audio"], c["z"], c["spk"], c["n_codes"], c["lengths"], sd=S.sd(name), upsample=S.CASES[name]["up"], tol=tol)
    assert ref.ambiguous_fraction() <= nll_ref.AMBIGUOUS_CAP
    f = S.f64(name)
    n = [m - 1 for m in c["lengths"]]
    lg = f.logits(c["audio"][:, :-1], f.condition(c["z"], c["spk"], c["n_codes"]), n)
    want = -torch.log_softmax(lg, dim=-1).gather(-1, c["audio"][:, 1:, None])[..., 0].numpy()
    assert float(np.abs(np.where(ref.mask, want, 0.0) - ref.nll).max()) <= 1e-12
    assert (ref.bound[ref.mask] >= 2.0 * tol).all() and not ref.bound[~ref.mask].any()
    d = nll_ref.case_ragged()
    a = nll_ref.reference("default", "ragged")
    b = nll_ref.Ref("default", d["audio"], d["z"], d["spk"], d["n_codes"], d["lengths"], sd=nll_ref.state_dict("default"),
                    upsample=160, tol=nll_ref.LOGIT_TOL["default"])
    assert np.array_equal(a.nll, b.nll) and np.array_equal(a.bound, b.bound)
