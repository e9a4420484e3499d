#!/usr/bin/env python3
"""Generate tests/golden/ema_*.npz from the REFERENCE itself (runs in the build container only).

Imports the reference's ``model.py`` as ``tools/gen_golden.py`` does, puts its own ``VQEmbeddingEMA`` in ``.train()`` and
records what one ``forward`` (``model.py:117-155``, the EMA update of ``:136-145``) leaves in the three buffers, on inputs
rebuilt from a seed (``tests/ema_ref.make_case``: x = codebook[code] + noise).  Fixtures are DATA only: the indices, ``ema_count``
in full, ``ema_weight`` / ``embedding`` in full for 64 codes and for every 8th code otherwise, the returned loss / perplexity, and
the reference's own three errors against the float64 restatement (``ema_ref.step_f64`` on the reference's indices) -- the yardstick
of the bounds in ``tests/test_ema_cpu.py`` and ``tests/test_gpu_ema.py``.

Usage:  python tools/gen_ema_golden.py            (writes tests/golden/ema_<case>.npz)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ema_ref  # noqa: E402
from gen_golden import import_reference  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def main():
    model = import_reference()
    print("reference imported from", model.__file__, "| torch", torch.__version__, "| threads", torch.get_num_threads())
    for name, (n_emb, n_rows, usage, start) in ema_ref.FIXTURE_CASES.items():
        case = ema_ref.make_case(name, n_emb, n_rows, usage, start)
        vq = model.VQEmbeddingEMA(n_emb, 64)
        vq.embedding.copy_(torch.from_numpy(case["embedding"]))
        vq.ema_count.copy_(torch.from_numpy(case["ema_count"]))
        vq.ema_weight.copy_(torch.from_numpy(case["ema_weight"]))
        vq.train()
        x = torch.from_numpy(case["x"])[None]
        with torch.no_grad():
            _, idx = vq.encode(x)                           # the indices forward() is about to compute, from the old codebook
            _, loss, ppl = vq(x)
        idx = idx.reshape(-1).numpy()
        assert np.array_equal(idx, case["code"]), "a row left its code: the case is not tie-free"
        got = (vq.ema_count.numpy(), vq.ema_weight.numpy(), vq.embedding.numpy())
        want = ema_ref.step_f64(case["x"], idx, case["ema_count"], case["ema_weight"], vq.decay, vq.epsilon)
        err = ema_ref.scaled_errors(got, want)
        own = ema_ref.scaled_errors(ema_ref.step_f32(case["x"], idx, case["ema_count"], case["ema_weight"]), want)
        every = 1 if n_emb == 64 else 8
        np.savez_compressed(os.path.join(GOLD, f"ema_{name}.npz"), case=np.array([n_emb, n_rows]), usage=np.array(usage),
                            start=np.array(start), decay=np.array(vq.decay), epsilon=np.array(vq.epsilon),
                            indices=idx.astype(np.int16), ema_count=got[0], every=np.array(every),
                            ema_weight=got[1][::every].copy(), embedding=got[2][::every].copy(),
                            loss=np.array(loss.item(), np.float32), perplexity=np.array(ppl.item(), np.float32),
                            ref_err=np.array(err, np.float64),
                            source=np.array("reference model.py VQEmbeddingEMA.forward in .train(), PyTorch CPU"))
        print(f"{name}: codes in use {np.unique(idx).size}/{n_emb}, largest code {np.bincount(idx).max()} rows | reference vs f64 "
              f"count {err[0]:.3g} weight {err[1]:.3g} embedding {err[2]:.3g} | step_f32 vs f64 {own[0]:.3g} {own[1]:.3g} {own[2]:.3g}")


if __name__ == "__main__":
    main()
