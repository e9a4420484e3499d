"""-m gpu: the tails around the a_t hand-off of the per-XCD resident decoders -- fc1's four accumulators combined, biased, rectified
and stored together (fc1_finish4, csrc/ar_chain.h; xd_put4) and the draw's first argmax taken in lanes (first_max_8lanes,
csrc/ar_shared.h) -- in every form that shares them: one, two and four slots per XCD, partially filled four-slot XCDs where `j < bx`
masks fc1's stores, ragged lengths, more utterances than slots, the resume kernels, agent-scope stores.  Every case is 2 code frames
cut at 320 samples on the resident decoders (``xcd`` 1, last_path() == 2) against the launch-per-step kernels (``xcd`` 0), whose
epilogues and draw are the plain expressions: waveforms and mu-law classes must be EQUAL and check() clean.  The ragged cases run
their frames out: 320 next to 640 samples.  The probe at the end compares the draw helper alone with a Python loop of first_max.
(a_t in fc2's operand order, planned with these two, measured slower and is not in the tree -- DESIGN 4, item 15, round 13 -- so
there is no layout test.)"""
import numpy as np
import pytest
import torch

import decode_harness as H
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu
TC, STEPS, SEED, UTT_BASE = 2, 320, 31, 5
CASES = H.CutCases(H.Handles(), "ah/?{B}", TC, STEPS, SEED, UTT_BASE)


@pytest.mark.parametrize("B,ragged", [(1, False), (8, False), (9, False), (16, True), (17, False), (25, False), (31, False), (32, False)])
def test_every_form_of_the_draw(B, ragged):
    """One slot per XCD (1, 8), two slots (9, 16 ragged), four slots with XCDs that run two or three of them (17, 25, 31), and all of
    them (32): a draw on one, two or four chain waves of a workgroup, fc1's joint stores with one to four live slots."""
    CASES.assert_equal(CASES.resident(B, ragged), B, ragged)


def test_32_ragged():
    CASES.assert_equal(CASES.resident(32, True), 32, True)


def test_40_utterances_through_32_slots():
    CASES.assert_equal(CASES.resident(40, True, xcd_slots=32), 40, True)


def test_stream_of_two_chunks_equals_one_shot():
    """The resume kernels share fc1's epilogue and fc2_and_draw: one code frame in two chunks of 160 samples equals the one-shot call."""
    CASES.assert_stream_equals_one_shot(32, chunk=160)


def test_agent_scope_stores_same_bits():
    CASES.assert_equal(CASES.resident(32, False, xcd_agent_stores=1), 32, False)


# ---- the draw helper alone

def _first_max(row):
    """csrc/ar_shared.h first_max over classes 0..7, in fp32: a later class wins only if strictly greater."""
    best, k = row[0], 0
    for c in range(1, 8):
        if row[c] > best:
            best, k = row[c], c
    return k, best


def _draw_cases():
    rng = np.random.default_rng(20260131)
    f32 = np.float32
    cases = [rng.standard_normal((2048, 8)).astype(f32) * f32(8.0),                       # seeded random scores
             (rng.standard_normal((512, 8)) * 1e-3).astype(f32)]                          # close together, both signs
    base = rng.standard_normal((64, 8)).astype(f32)
    ties = []
    for a in range(8):                                                                      # every pair tied at the maximum
        for b in range(a + 1, 8):
            for row in base[:4]:
                r = row.copy()
                r[a] = r[b] = f32(9.5)
                ties.append(r)
    cases.append(np.array(ties, f32))
    cases.append(np.array([[v] * 8 for v in (0.0, -0.0, 1.5, -3.25, np.inf, -np.inf, 1e-45, -1e-45)], f32))      # all equal
    asc = np.arange(8, dtype=f32)
    cases.append(np.array([asc, asc[::-1], -asc, -asc[::-1], asc * f32(1e-41), asc[::-1] * f32(1e-41)], f32))    # ascending, descending
    zeros = np.array([[(-0.0 if (m >> c) & 1 else 0.0) for c in range(8)] for m in range(256)], f32)             # every +-0 mix
    cases.append(zeros)
    cases.append(np.where(rng.random((256, 8)) < 0.5, zeros, f32(-1.0)).astype(f32))                             # +-0 above negatives
    inf = base.copy()
    inf[rng.random(inf.shape) < 0.3] = -np.inf
    cases.append(inf)
    inf = base.copy()
    inf[rng.random(inf.shape) < 0.2] = np.inf
    inf[rng.random(inf.shape) < 0.2] = -np.inf
    cases.append(inf)
    den = (rng.integers(-40, 41, (256, 8)) * 1e-45).astype(f32)                                                  # denormals, +-0 among them
    cases.append(den)
    cases.append(np.where(rng.random((128, 8)) < 0.5, den[:128], f32(1.17549435e-38)).astype(f32))               # next to the smallest normal
    return np.concatenate(cases)


def test_draw_helper_equals_first_max():
    sc = _draw_cases()
    assert 3000 < len(sc) < 8000 and not np.isnan(sc).any()
    lib = _lib.load()
    d_sc = torch.from_numpy(sc).cuda()
    d_cls = torch.full((len(sc),), -1, dtype=torch.int32, device="cuda")
    d_bits = torch.zeros(len(sc), dtype=torch.int32, device="cuda")
    _lib.check(lib.vqcpc_probe_draw(d_sc.data_ptr(), len(sc), d_cls.data_ptr(), d_bits.data_ptr(), _lib.current_stream()))
    torch.cuda.synchronize()
    got_k, got_bits = d_cls.cpu().numpy(), d_bits.cpu().numpy().view(np.uint32)
    want = [_first_max(row) for row in sc]
    want_k = np.array([w[0] for w in want], np.int32)
    want_bits = np.array([w[1] for w in want], np.float32).view(np.uint32)
    bad = np.nonzero((got_k != want_k) | (got_bits != want_bits))[0]
    assert len(bad) == 0, (len(bad), sc[bad[0]], int(got_k[bad[0]]), int(want_k[bad[0]]), hex(got_bits[bad[0]]), hex(want_bits[bad[0]]))
