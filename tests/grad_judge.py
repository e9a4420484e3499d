"""Shared by the gradient tests (plain module, not a conftest): the one judge of a result against a float64 reference, the pins
that hold that reference, and the seeded inputs.  tests/cpc_grad_ref.py, ctx_grad_ref.py and front_grad_ref.py supply the cases
and the references and call in here; tools/gen_*_grad_golden.py write the pins with ``pin_entries``.

Pins, per case and tensor, in an ``.npz`` under tests/golden: ``<case>_<tensor>_samples`` (the float64 reference at ``N_SAMPLES``
seeded positions), ``_sums`` (its sum and sum of squares), ``_max`` (``max |G64|``) and ``_e_ref`` (``max |G_ref32 - G_ref64|``,
the error of the reference's own fp32 run on the CPU).  ``check_pins`` holds a float64 reference to them within 1e-12 relative.

Judge, per tensor, the same for every case: ``max |G - G64| <= 4 max(e_ref, 2^-24 max |G64|)``.  The factor 4 is the project's
rule for a fixed fp32 summation order against the reference's own error; the floor covers a tensor whose reference
error happens to fall below one rounding of its largest element.  Where ``G64`` is identically zero the result must be fp32 and
exact ``+0``.  Nothing in it is measured on the code under test.

Per row (``judge_rows``, for the tensors whose rows are outputs of their own: a table's gradient per code, ``grad_cond`` per frame):
the same rule with ``e_ref`` and ``max |G64|`` taken over one row, so that a row many orders of magnitude below the tensor's
largest element is held to its own size.  Its pins are ``<case>_<tensor>_row_max`` and ``_row_e_ref`` over the rows
``_row_idx`` lists (``row_pin_entries``); every other row is zero in float64 and must come back ``+0``.
"""
import contextlib
import functools
import os
import zipfile

import numpy as np
import torch

from vectorquantizedcpc_amd import synth

U32 = 2.0 ** -24
N_SAMPLES = 64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@contextlib.contextmanager
def one_thread():
    """torch on one thread inside the block: the summation order the generators record ``e_ref`` with, and the way a CPU reference
    of many small products is quickest (a thread pool only gets in their way)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def uniform(seed, shape, bound):
    """fp32 torch tensor of ``shape``, U(+-bound) from the stream ``seed`` names."""
    n = int(np.prod(shape))
    return torch.from_numpy(((synth.uniform01(seed, n) * 2.0 - 1.0) * bound).astype(np.float32).reshape(shape))


@functools.lru_cache(maxsize=None)
def load_pins(*paths):
    """The pins of ``paths`` as one dict (keys start with the case's name: the files of one family share none).  Read at the first
    call and shared (treat as read-only)."""
    return {k: v for path in paths for k, v in np.load(path).items()}


def sample_positions(seed, numel):
    """The ``N_SAMPLES`` flat element positions, drawn from the stream ``seed`` names, whose reference values the pins hold."""
    return synth.randint(seed, (N_SAMPLES,), numel).numpy()


def bound(pins, name, tensor):
    """The judge's right-hand side for one tensor of one case."""
    return 4.0 * max(float(pins[f"{name}_{tensor}_e_ref"]), U32 * float(pins[f"{name}_{tensor}_max"]))


def judge(ref, pins, name, got, what, keys):
    """Every tensor ``keys`` names of ``got`` (dict of arrays; missing or None = not asked for) against the float64 ``ref``: prints
    each figure, then asserts."""
    bad = []
    for k in keys:
        if got.get(k) is None:
            continue
        a = np.asarray(got[k])
        assert a.shape == ref[k].shape, (k, a.shape, ref[k].shape)
        if not ref[k].any():                                         # identically zero: exact +0, bit for bit
            ok = a.dtype == np.float32 and not a.view(np.uint32).any()
            print(f"{what} {name} {k}: reference identically zero, result all +0: {ok}")
            if not ok:
                bad.append((k, "not +0"))
            continue
        a = a.astype(np.float64)
        err, e_ref, limit = float(np.abs(a - ref[k]).max()), float(pins[f"{name}_{k}_e_ref"]), bound(pins, name, k)
        print(f"{what} {name} {k}: max|G - G64| = {err:.3g}, e_ref = {e_ref:.3g}, err / bound {err / limit:.3f}, bound {limit:.3g}, "
              f"max|G64| = {np.abs(ref[k]).max():.3g}")
        if not (np.isfinite(a).all() and err <= limit):
            bad.append((k, err, limit))
    assert not bad, bad


def check_pins(ref, pins, name, keys, positions):
    """The float64 reference ``ref`` reproduces the pins of case ``name``, each figure within 1e-12 relative.  ``positions``: the
    seed of ``sample_positions`` with ``{name}`` and ``{tensor}`` left to fill in."""
    for k in keys:
        G, top = ref[k], float(pins[f"{name}_{k}_max"])
        assert abs(np.abs(G).max() - top) <= 1e-12 * top, k
        samples = G.reshape(-1)[sample_positions(positions.format(name=name, tensor=k), G.size)]
        assert np.abs(samples - pins[f"{name}_{k}_samples"]).max() <= 1e-12 * top, k
        s, ss = pins[f"{name}_{k}_sums"]
        assert abs(G.sum() - s) <= 1e-12 * np.abs(G).sum() and abs((G ** 2).sum() - ss) <= 1e-12 * ss, k


def pin_entries(name, ref64, ref32, positions, keys=None):
    """What a generator records of case ``name``: for every tensor of ``keys`` (default: all of ``ref64``) the ``_samples``,
    ``_sums``, ``_max`` and ``_e_ref`` entries, from the float64 reference and the same reference run in fp32.  ``positions``: as
    for ``check_pins``."""
    out = {}
    for k in (ref64 if keys is None else keys):
        G = ref64[k]
        out[f"{name}_{k}_samples"] = G.reshape(-1)[sample_positions(positions.format(name=name, tensor=k), G.size)]
        out[f"{name}_{k}_sums"] = np.array([G.sum(), (G ** 2).sum()])
        out[f"{name}_{k}_max"] = np.float64(np.abs(G).max())
        out[f"{name}_{k}_e_ref"] = np.float64(np.abs(ref32[k] - G).max())
    return out


def rows_of(a):
    """``a`` (2-D or 3-D) as (rows, last dimension): a row is the leading index, or the leading two flattened."""
    a = np.asarray(a)
    assert a.ndim in (2, 3), a.shape
    return a.reshape(-1, a.shape[-1])


def row_pin_entries(name, ref64, refs32, keys):
    """The row pins of case ``name`` for the tensors of ``keys``: ``_row_idx`` (the rows that are not identically zero in float64,
    int32, ascending), and over those rows ``_row_max`` (``max |G64[row]|``) and ``_row_e_ref`` (``max |G_ref32[row] - G64[row]|``,
    the largest over the fp32 CPU yardsticks ``refs32``, a list of runs that may sum in different orders).  Rows that are not
    listed are zero in float64; only the others cost bytes."""
    out = {}
    for k in keys:
        G = rows_of(ref64[k])
        idx = np.flatnonzero(np.abs(G).max(axis=1) > 0.0).astype(np.int32)
        e = np.max([np.abs(rows_of(low[k]) - G).max(axis=1) for low in refs32], axis=0)
        out[f"{name}_{k}_row_idx"] = idx
        out[f"{name}_{k}_row_max"] = np.abs(G).max(axis=1)[idx]
        out[f"{name}_{k}_row_e_ref"] = e[idx]
    return out


def row_pins(pins, name, tensor, n_rows):
    """``(top, e_ref)`` per row of one tensor of one case, each of length ``n_rows``: zero where the pins list no row."""
    idx = pins[f"{name}_{tensor}_row_idx"]
    top, e_ref = np.zeros(n_rows), np.zeros(n_rows)
    top[idx], e_ref[idx] = pins[f"{name}_{tensor}_row_max"], pins[f"{name}_{tensor}_row_e_ref"]
    return top, e_ref


def check_row_pins(ref, pins, name, keys):
    """The float64 reference ``ref`` reproduces the row pins of case ``name``: the same rows are non-zero, and each row's largest
    magnitude is the pinned one within 1e-12 relative."""
    for k in keys:
        G = rows_of(ref[k])
        top, _ = row_pins(pins, name, k, G.shape[0])
        mine = np.abs(G).max(axis=1)
        assert np.array_equal(mine > 0.0, top > 0.0), k
        assert (np.abs(mine - top) <= 1e-12 * top).all(), k


def judge_rows(ref, pins, name, got, what, keys):
    """The judge's rule per row of the 2-D or 3-D tensors ``keys`` names of ``got`` (a row: ``rows_of``), no row left out:
    ``max |G[row] - G64[row]| <= 4 max(e_ref[row], 2^-24 max |G64[row]|)``, and a row that is identically zero in float64 must be
    exact ``+0``, bit for bit.  Prints the worst ratio to the bound with its row and the smallest row magnitude held, then asserts.
    -> {tensor: (worst ratio, its row as an index tuple, smallest non-zero ``max |G64[row]|``)}."""
    bad, seen = [], {}
    for k in keys:
        if got.get(k) is None:
            continue
        a = np.asarray(got[k])
        assert a.shape == ref[k].shape and a.dtype == np.float32, (k, a.shape, a.dtype, ref[k].shape)
        A, G = rows_of(a), rows_of(ref[k])
        top, e_ref = row_pins(pins, name, k, G.shape[0])
        assert np.array_equal(top > 0.0, np.abs(G).max(axis=1) > 0.0), (k, "row pins are not this reference's")
        zero = top == 0.0
        limit = 4.0 * np.maximum(e_ref, U32 * top)
        with np.errstate(invalid="ignore"):
            err = np.where(np.isfinite(A).all(axis=1), np.abs(A.astype(np.float64) - G).max(axis=1), np.inf)
        plus0 = ~np.ascontiguousarray(A).view(np.uint32).any(axis=1)
        ratio = np.where(zero, np.where(plus0, 0.0, np.inf), err / np.where(zero, 1.0, limit))
        r = int(ratio.argmax())
        at = tuple(int(i) for i in np.unravel_index(r, a.shape[:-1]))
        low = float(top[~zero].min()) if (~zero).any() else 0.0
        print(f"{what} {name} {k} per row: worst err / bound = {ratio[r]:.3f} at row {at} (err {err[r]:.3g}, e_ref[row] {e_ref[r]:.3g}, "
              f"max|G64[row]| = {top[r]:.3g}); max|G64[row]| spans {low:.3g} .. {top.max():.3g} over {int((~zero).sum())} rows; "
              f"{int(zero.sum())} zero rows, all +0: {bool(plus0[zero].all())}")
        seen[k] = (float(ratio[r]), at, low)
        if not ratio[r] <= 1.0:
            bad.append((k, at, float(err[r]), float(limit[r])))
    assert not bad, bad
    return seen


def write_npz(path, arrays):
    """An uncompressed .npz as ``np.load`` reads it, with the archive's dates fixed (``np.savez`` stamps the time of writing)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for key, value in arrays.items():
            with zf.open(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), "w") as f:
                np.lib.format.write_array(f, np.asanyarray(value), allow_pickle=False)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
