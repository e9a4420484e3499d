"""The judge of tests/grad_judge.py on synthetic arrays and a hand-made pins dictionary: what it lets pass and what it refuses, at the
bound itself and one fp32 rounding past it."""
import numpy as np
import pytest

import grad_judge

f32 = np.float32
REF = {"g": np.array([[1.0, 0.5], [-0.25, 0.125]]), "zero": np.zeros((2, 3))}       # every value an fp32 number: the errors below are exact
ULP = 2.0 ** -23                                                                     # of fp32 at 1.0, the largest element of g


def pins(e_ref):
    return {"case_g_e_ref": np.float64(e_ref), "case_g_max": np.float64(1.0), "case_zero_e_ref": np.float64(0.0), "case_zero_max": np.float64(0.0)}


def off_by(err):
    """g as fp32 with its largest element wrong by exactly ``err``."""
    a = REF["g"].astype(f32)
    a[0, 0] = f32(1.0 + err)
    assert float(a[0, 0]) - 1.0 == err
    return a


def judge(got, e_ref=2.0 ** -20):
    grad_judge.judge(REF, pins(e_ref), "case", got, "synthetic", ["g", "zero"])


def refused(got, e_ref=2.0 ** -20):
    with pytest.raises(AssertionError):
        judge(got, e_ref)


def test_a_result_within_the_bound_passes_and_one_ulp_past_it_fails():
    assert grad_judge.bound(pins(2.0 ** -20), "case", "g") == 2.0 ** -18             # 4 e_ref
    judge({"g": off_by(2.0 ** -19)})
    judge({"g": off_by(2.0 ** -18)})                                                  # at the bound
    refused({"g": off_by(2.0 ** -18 + ULP)})


def test_tensors_not_asked_for_are_skipped():
    judge({"g": None, "zero": None})
    judge({})
    judge({"g": off_by(0.0)})


def test_a_nan_an_inf_and_a_wrong_shape_fail():
    for v in (np.nan, np.inf):
        a = REF["g"].astype(f32)
        a[1, 1] = v
        refused({"g": a})
    refused({"g": REF["g"].astype(f32).reshape(4)})
    refused({"g": REF["g"].astype(f32)[:1]})


def test_the_floor_holds_where_the_reference_error_is_zero():
    assert grad_judge.bound(pins(0.0), "case", "g") == 4 * grad_judge.U32 == 2.0 ** -22      # 4 * 2^-24 * max |G64|
    judge({"g": off_by(2.0 ** -22 - ULP)}, e_ref=0.0)
    judge({"g": off_by(2.0 ** -22)}, e_ref=0.0)
    refused({"g": off_by(2.0 ** -22 + ULP)}, e_ref=0.0)


def test_an_identically_zero_reference_wants_fp32_plus_zero_bits():
    judge({"zero": np.zeros((2, 3), f32)})
    for bad in (f32(-0.0), np.finfo(f32).smallest_subnormal):
        a = np.zeros((2, 3), f32)
        a[1, 2] = bad
        assert a.view(np.uint32)[1, 2] != 0
        refused({"zero": a})
    refused({"zero": np.zeros((2, 3), np.float64)})
    refused({"zero": np.zeros((3, 2), f32)})
