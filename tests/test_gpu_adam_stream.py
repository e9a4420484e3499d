"""-m gpu: ``vqcpc_adam_step`` on a caller's stream -- the stream contract of ``include/vqcpc.h`` (*all work is enqueued on `stream`;
no call synchronises*), held with tests/stream_harness.py exactly as tests/test_gpu_stream_contract.py holds the other entries.
That file keeps the one table of entries against the header; its row names the test here.

Does not synchronise (``busy`` is asserted).  The parameters, the gradients and both moments of every tensor are among the
buffers written behind the delay: an update enqueued anywhere but on the caller's stream reads the decoy, and one still running
when the call returns is overtaken by the harness's clones.  The list is longer than one launch's table, so the second launch is
held too.
"""
import numpy as np
import pytest
import torch

import adam_ref as R
import stream_harness as H
from vectorquantizedcpc_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [R.CHUNK + 1, 5, 2 * R.CHUNK + 3] + [3 + i % 4 for i in range(R.TABLE)]       # TABLE + 3 tensors: two launches


@pytest.fixture(scope="module", autouse=True)
def release_what_this_file_holds():
    """The device buffers of this file are released when it is done, and the stream harness's session-wide delay chain and report
    are left as they were found (``stream_harness.release_after`` says why)."""
    yield from H.release_after()


def _buffers(tag, v_floor):
    """p, g, m, v of every tensor, seeded: finite, v positive."""
    out = []
    for i, n in enumerate(SIZES):
        u = [R.synth.uniform01(f"adam/stream/{tag}/{k}{i}", n) for k in "pgmv"]
        out += [torch.from_numpy(((u[0] * 2 - 1)).astype(np.float32)), torch.from_numpy(((u[1] * 2 - 1) * 0.1 + 0.2).astype(np.float32)),
                torch.from_numpy(((u[2] * 2 - 1) * 0.05).astype(np.float32)), torch.from_numpy((v_floor + u[3] * 0.01).astype(np.float32))]
    return [t.cuda() for t in out]


def test_adam_step_on_a_callers_stream():
    true, decoy = _buffers("true", 1e-3), _buffers("decoy", 2e-3)
    n = len(SIZES)
    hyper = _lib.AdamHyper(R.LR, 0.9, 0.999, R.EPS, 7)
    dev = true[0].device

    def entry(*bufs):
        table = (_lib.AdamTensor * n)(*[_lib.AdamTensor(*(b.data_ptr() for b in bufs[4 * i:4 * i + 4]), SIZES[i]) for i in range(n)])
        _lib.adam_step(table, n, hyper, dev)
        return list(bufs)                                  # p, m, v as updated; g as it was

    res = H.hold(entry, true, decoy, label=f"adam_step, {n} tensors")
    # and the values are the update's: the restatement on the true inputs
    k = R.scalars(R.LR, 0.9, 0.999, R.EPS, 7)
    for i in (0, 1, 2, n - 1):
        p, g, m, v = (t.cpu().numpy().copy() for t in true[4 * i:4 * i + 4])
        R.update(p, g, m, v, k)
        for j, want in enumerate((p, g, m, v)):
            assert np.array_equal(res[str(4 * i + j)].cpu().numpy().view(np.uint32), want.view(np.uint32)), (i, j)
