"""CPU checks of the codebook-update contract: the fp32 restatement ``ema_ref.step_f32`` -- the order the HIP kernels
keep bit for bit (tests/test_gpu_ema.py) -- against what the REFERENCE's own ``VQEmbeddingEMA`` in ``.train()`` left in its buffers
(tests/golden/ema_*.npz, tools/gen_ema_golden.py) and against float64.

Bound, for every fixture and each of the three buffers: max(4 x the reference's own recorded error against float64, 2 fp32 ulp),
errors scaled as ``ema_ref.scaled_errors`` scales them.  It is measured from the reference, never from the code under test.
Recorded reference errors (count, weight, embedding) and the restatement's own against float64:

  ======================  ===========================  ===========================
  fixture                 reference vs float64         step_f32 vs float64
  ======================  ===========================  ===========================
  m64_n160_warm           9.67e-8  9.19e-8  1.79e-7    9.67e-8  9.19e-8  1.79e-7
  m64_n4096_onecode       6.71e-8  7.54e-8  1.95e-7    8.13e-8  5.35e-8  1.95e-7
  m512_n4096_every_zero   0        8.08e-8  1.21e-7    0        8.08e-8  1.21e-7
  m512_n4096_warm         1.30e-7  1.05e-7  2.89e-7    1.30e-7  1.05e-7  2.89e-7
  m1024_n4113_skewed      1.51e-7  1.06e-7  2.71e-7    1.51e-7  1.06e-7  2.71e-7
  ======================  ===========================  ===========================

The per-code row sums alone are held to the same kind of bound past the fixtures' sizes, at 33 280 rows (one code owning 11 791
of them) and at 4 096 rows on one code: at most max(4 x the error of the reference's own ``encodings.t() @ x_flat`` on the same rows,
2 fp32 ulp), per code and scaled by the code's largest |value|.
"""
import math
import os
import struct

import numpy as np
import pytest

import ema_ref
import vectorquantizedcpc_amd as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", params=list(ema_ref.FIXTURE_CASES))
def fixture_case(request):
    name = request.param
    gold = np.load(os.path.join(GOLDEN, f"ema_{name}.npz"))
    case = ema_ref.make_case(name, *ema_ref.FIXTURE_CASES[name])
    idx = gold["indices"].astype(np.int64)
    got = ema_ref.step_f32(case["x"], idx, case["ema_count"], case["ema_weight"], float(gold["decay"]), float(gold["epsilon"]))
    return name, gold, case, idx, got


def against_fixture(got, gold):
    """Errors of (count, weight, embedding) against the reference's recorded values, scaled like ``ema_ref.scaled_errors``."""
    every = int(gold["every"])
    return ema_ref.scaled_errors((got[0], got[1][::every], got[2][::every]),
                                 tuple(gold[k].astype(np.float64) for k in ("ema_count", "ema_weight", "embedding")))


def test_fixtures_are_the_declared_cases(fixture_case):
    name, gold, case, idx, _ = fixture_case
    n_emb, n_rows, usage, start = ema_ref.FIXTURE_CASES[name]
    assert tuple(gold["case"]) == (n_emb, n_rows) and str(gold["usage"]) == usage and str(gold["start"]) == start
    assert np.array_equal(idx, case["code"])                       # rebuilt from the seed, the rows still take the recorded codes
    assert gold["ema_count"].shape == (n_emb,)
    assert gold["embedding"].shape == (n_emb // int(gold["every"]), 64) == gold["ema_weight"].shape
    assert int(gold["every"]) == (1 if n_emb == 64 else 8)
    assert os.path.getsize(os.path.join(GOLDEN, f"ema_{name}.npz")) < 126 * 1024


def test_step_f32_within_the_reference_bound(fixture_case):
    name, gold, _, _, got = fixture_case
    err = against_fixture(got, gold)
    bounds = [ema_ref.bound(e) for e in gold["ref_err"]]
    print(f"{name}: step_f32 vs reference {err[0]:.3g} {err[1]:.3g} {err[2]:.3g} | bounds {bounds[0]:.3g} {bounds[1]:.3g} {bounds[2]:.3g}")
    for what, e, b in zip(("ema_count", "ema_weight", "embedding"), err, bounds):
        assert e <= b, (name, what, e, b)


def test_step_f32_against_float64_no_worse_than_the_bound(fixture_case):
    name, gold, case, idx, got = fixture_case
    want = ema_ref.step_f64(case["x"], idx, case["ema_count"], case["ema_weight"], float(gold["decay"]), float(gold["epsilon"]))
    for what, e, r in zip(("ema_count", "ema_weight", "embedding"), ema_ref.scaled_errors(got, want), gold["ref_err"]):
        assert e <= ema_ref.bound(r), (name, what, e, r)


def test_recorded_reference_error_is_reproducible_from_the_fixture(fixture_case):
    """``ref_err`` is the reference's error against ``step_f64``: recomputed here from the recorded buffers."""
    name, gold, case, idx, _ = fixture_case
    want = ema_ref.step_f64(case["x"], idx, case["ema_count"], case["ema_weight"], float(gold["decay"]), float(gold["epsilon"]))
    every = int(gold["every"])
    sub = ema_ref.scaled_errors((gold["ema_count"], gold["ema_weight"], gold["embedding"]), (want[0], want[1][::every], want[2][::every]))
    for s, r in zip(sub, gold["ref_err"]):
        assert s <= r * (1 + 1e-12) + 1e-300                       # the recorded figure is over every code, this over the kept ones
    assert sub[0] == pytest.approx(float(gold["ref_err"][0]), rel=1e-9, abs=1e-300)       # ema_count is kept in full


def test_omd_is_pinned_by_its_bits():
    dec, omd, eps, meps = ema_ref.constants(0.999, 1e-5, 512)
    bits = lambda v: struct.unpack("<I", struct.pack("<f", float(v)))[0]
    assert bits(omd) == 0x3A83126F == bits(np.float32(1.0 - 0.999))
    assert bits(np.float32(1.0) - np.float32(0.999)) == 0x3A831200                       # the trap: 1.3e-5 away
    assert bits(dec) == 0x3F7FBE77 and bits(eps) == 0x3727C5AC
    assert bits(meps) == bits(np.float32(512 * 1e-5)) == 0x3BA7C5AC


def test_tree_sum_is_the_binary_counter():
    """The kernel realises the adjacent-pair tree as a binary-counter merge: both orders written out on exact integers' worth
    of structure (string concatenation shows the bracketing)."""
    for n in list(range(1, 20)) + [64, 65, 519, 520]:
        leaves = [str(i) for i in range(n)]
        want = ema_ref.tree_sum([_Bracket(s) for s in leaves]).s
        st, got = {}, None
        for c, leaf in enumerate(leaves):
            acc, l = _Bracket(leaf), 0
            while (c >> l) & 1:
                acc = st.pop(l) + acc
                l += 1
            st[l] = acc
        for l in sorted(st):
            got = st[l] if got is None else st[l] + got
        assert got.s == want, n


class _Bracket:
    """A partial sum that shows its bracketing; ``None`` is an exact zero: adding it changes no value."""
    def __init__(self, s):
        self.s = s

    def __add__(self, other):
        if self.s is None or other.s is None:
            return _Bracket(other.s if self.s is None else self.s)
        return _Bracket(f"({self.s}+{other.s})")


def _counter(leaves):
    st, got = {}, _Bracket(None)
    for c, leaf in enumerate(leaves):
        acc, l = leaf, 0
        while (c >> l) & 1:
            acc = st.pop(l) + acc
            l += 1
        st[l] = acc
    for i, l in enumerate(sorted(st)):
        got = st[l] if i == 0 else st[l] + got
    return got


def test_eight_wave_split_is_the_same_tree():
    """``ema_update_kernel`` gives wave w the aligned block of S chunks from w * S (S a power of two, 8 S >= chunks), each summed
    by its own counter, and adds ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)): value for value the adjacent-pair tree, an absent block being an exact zero."""
    for n in list(range(1, 40)) + [64, 65, 129, 519, 520, 521, 1 << 10, (1 << 10) + 1]:
        leaves = [_Bracket(str(i)) for i in range(n)]
        S = 1
        while 8 * S < n:
            S *= 2
        w = [_counter(leaves[k * S:(k + 1) * S]) for k in range(8)]
        assert (((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]))).s == ema_ref.tree_sum(leaves).s, n


@pytest.mark.parametrize("n_rows,usage,largest", [(33280, "skewed", 11791), (4096, "one", 4096)])
def test_row_sums_within_the_bound_of_the_reference_matmul(n_rows, usage, largest):
    """The accuracy the summation order was chosen for, past the fixtures' sizes: per code, scaled by the code's largest |value|,
    the chunk-tree sum's error against float64 is at most max(4 x the error of the reference's own ``encodings.t() @ x_flat``
    (``model.py:132, :142``, run here with torch on the CPU on the same rows), 2 fp32 ulp).  Measured: 1.35e-7 against 4 x 1.52e-7 at
    33 280 rows (64-row chunks combined sequentially: 7.9e-7, a plain ascending sum: 2.5e-6), 8.3e-8 against 4 x 2.28e-7 at
    4 096 rows on one code (2.3e-7, 2.8e-6).  The a-priori bound of the order, gamma_k * sum|x| with k = 63 + ceil(log2(chunks))
    additions on any path, is kept beside it as a check of the restatement itself."""
    import torch
    import torch.nn.functional as F
    case = ema_ref.make_case(f"cpu_sum_{n_rows}", 64, n_rows, usage, "warm")
    idx, x = case["code"], case["x"]
    assert np.bincount(idx).max() == largest
    dw = ema_ref.code_sums_f32(x, idx, 64).astype(np.float64)
    ref = torch.matmul(F.one_hot(torch.from_numpy(idx), 64).float().t(), torch.from_numpy(x)).numpy().astype(np.float64)
    want, mag = np.zeros((64, 64)), np.zeros((64, 64))
    np.add.at(want, idx, x.astype(np.float64))
    np.add.at(mag, idx, np.abs(x).astype(np.float64))
    scale = np.abs(want).max(axis=1, keepdims=True)
    scale[scale == 0] = 1.0
    err, ref_err = float((np.abs(dw - want) / scale).max()), float((np.abs(ref - want) / scale).max())
    print(f"{n_rows} rows {usage}: tree-sum error {err:.3g}, reference matmul {ref_err:.3g}, bound {ema_ref.bound(ref_err):.3g}")
    assert err <= ema_ref.bound(ref_err), (err, ref_err)
    k = 63 + math.ceil(math.log2(max(2, -(-n_rows // 64))))
    u = 2.0 ** -24
    assert np.all(np.abs(dw - want) <= k * u / (1 - k * u) * mag)


def test_training_forward_no_longer_refuses_on_principle():
    """Without the feature ``VQEmbeddingEMA.forward`` in training mode raised ``NotImplementedError`` before looking at its input;
    now a CPU tensor gets the no-CPU-fallback error of every other entry point, and only a gradient request is refused."""
    import torch
    enc = V.Encoder(V.ConfEncoder(80, 512, 512, 64, 256)).train()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.codebook(torch.zeros(1, 4, 64))
    with pytest.raises(NotImplementedError, match="straight-through"):
        enc.codebook(torch.zeros(1, 4, 64, requires_grad=True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc.adapt_codebook(torch.zeros(1, 80, 32))
    assert "vqcpc_encoder_vq_adapt" in V._lib.SYMBOLS
