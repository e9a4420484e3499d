"""-m gpu: CPC scoring (``csrc/cpc.hip``) against float64 past the four fixture shapes -- both ends of the MFMA loop (c_dim 64 and
512), 1 and 64 negatives, 16 prediction steps, a finish kernel with two to three partials per thread, scores to +-130, L = 2,
a last tile with 15 live anchors, explicit indices at the corners, and a workspace that is grown and then used short.

Cases, reference, bounds and their derivations: tests/cpc_cases.py (``check_result`` prints every figure and then asserts);
tests/test_cpc_f64_cpu.py holds the reference alone to the same bounds on the CPU.  Nothing here is measured on the code under test.
"""
import pytest
import torch

import cpc_cases
import vectorquantizedcpc_amd as V

pytestmark = pytest.mark.gpu


def module_for(ref):
    cpc = V.CPCLoss(V.ConfCPC(ref["n_pred"], ref["Spk"], ref["Utt"], ref["Neg"], 64, ref["c_dim"]))
    cpc.load_state_dict(ref["sd"])
    return cpc.cuda().eval()


def bits(t):
    return t.reshape(-1).view(torch.uint8)


def same_bits(a, b, keys):
    for key in keys:
        assert torch.equal(bits(a[key]), bits(b[key])), key


ALL_KEYS = ("loss", "step_loss", "accuracy", "correct", "scores")


def detailed(cpc, ref, **kw):
    return cpc.forward_detailed(ref["z"].cuda(), ref["c"].cuda(), want_correct=True, want_scores=True, **kw)


@pytest.mark.parametrize("name", list(cpc_cases.CASES))
def test_against_float64(name):
    ref = cpc_cases.reference(name)
    cpc = module_for(ref)
    r = detailed(cpc, ref, negatives=(ref["utt"], ref["seq"]))
    cpc_cases.check_result(ref, r, name)
    # a second identical call repeats all bits; a call without the optional outputs returns the same losses and accuracies
    same_bits(detailed(cpc, ref, negatives=(ref["utt"], ref["seq"])), r, ALL_KEYS)
    plain = cpc.forward_detailed(ref["z"].cuda(), ref["c"].cuda(), negatives=(ref["utt"], ref["seq"]))
    assert plain["scores"] is None and plain["correct"] is None
    same_bits(plain, r, ("loss", "step_loss", "accuracy"))


@pytest.mark.parametrize("name,seed,stream", [("c64_min", (9 << 32) | 13, 0), ("c512_neg64", 13, 0), ("steps16", (7 << 32) | 5, 3),
                                              ("partials", 1, 1)])
def test_protocol_mode_equals_explicit_indices_bit_for_bit(name, seed, stream):
    ref = cpc_cases.reference(name)
    cpc = module_for(ref)
    a = detailed(cpc, ref, seed=seed, stream_id=stream)
    b = detailed(cpc, ref, negatives=cpc_cases.negatives(ref, seed, stream))
    same_bits(a, b, ALL_KEYS)
    if (seed, stream) == (13, 0):                          # the draws of the float64 reference itself
        cpc_cases.check_result(ref, a, f"{name}, protocol mode")


def test_workspace_grown_then_used_short():
    """One ``CPCLoss`` of the ``partials`` configuration: T = 3 (70 partials), T = 260 (595), T = 3 again on the grown workspace."""
    short, full = cpc_cases.reference("partials", cpc_cases.SHRINK_T), cpc_cases.reference("partials")
    assert torch.equal(short["z"], full["z"][:, :cpc_cases.SHRINK_T]) and short["z"].is_contiguous() and short["c"].is_contiguous()
    cpc = module_for(full)
    first = detailed(cpc, short, negatives=(short["utt"], short["seq"]))
    grown = detailed(cpc, full, negatives=(full["utt"], full["seq"]))
    third = detailed(cpc, short, negatives=(short["utt"], short["seq"]))
    same_bits(first, third, ALL_KEYS)
    cpc_cases.check_result(short, first, "partials at T = 3, fresh workspace")
    cpc_cases.check_result(full, grown, "partials at T = 260, grown workspace")
    cpc_cases.check_result(short, third, "partials at T = 3, after T = 260")
