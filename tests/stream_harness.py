"""Shared by tests/test_gpu_stream_contract.py (plain module, not a conftest): the procedure that holds one entry point to the
stream contract of ``include/vqcpc.h`` -- *all work is enqueued on `stream`; no call synchronises except where stated* -- on a
caller's stream.

``run(entry, inputs, decoy)`` does, in this order:

1. Reference.  ``entry(*clones of inputs)`` twice on the default stream, a device synchronisation after each.  The first run
   builds whatever the call builds once (work space, captured graphs, the staging arena); the second is timed on the host
   (``time.perf_counter`` around the enqueue only: ``t_host``) and gives the reference bits.
2. Live buffers filled with the DECOY: valid inputs of the same shapes and dtypes (finite floats, in-range indices -- a stale read
   gives wrong values, never a bad address).  A fresh ``torch.cuda.Stream`` ``s``.  Device synchronisation.
3. Under ``torch.cuda.stream(s)``: (a) a delay, a chain of fp32 ``torch.mm``; (b) the true inputs copied into the live buffers;
   (b') blocks shaped like the reference's outputs filled with a finite pattern and handed back to the allocator, so that the
   outputs the entry is about to allocate on ``s`` are dirty until ITS work clears them, and an event recorded behind all of this;
   (c) the entry on the live buffers; (d) ``busy = not s.query()`` and that event not yet reached; (e) every output cloned on
   ``s``; (f) the live buffers overwritten with the decoy again.  No host synchronisation anywhere in between.
   (``s.query()`` alone does not do for (d): an entry that synchronises FIRST and enqueues afterwards returns with its own work
   still in flight.  The harness's self-test showed that on the first MI355X run; the event behind the delay settles it.)
4. ``s.synchronize()``, ``torch.cuda.synchronize()``: the device is quiet whatever happened.  Then every clone is compared with
   its reference, bit for bit.
5. ``busy`` must be true unless the entry is one the header says synchronises.

Steps 2 - 4 run TWICE, on two streams created one after the other.  The runtime spreads its streams over a few hardware queues
(four here), and work that a faulty entry puts on the default stream is, by accident, in order with a caller's stream that shares
the default stream's queue: measured on an MI355X with a pure-torch entry that works on the default stream, rounds 6 and 10 of
12 fresh streams (every fourth) gave the right bits.  Two streams in a row never both share it.

What each step catches: work that is not ordered behind ``s`` (a launch, memset or copy on another stream) runs during the delay
and reads the decoy, or clears an output before (b') dirties it; work still running on an internal stream when the call returns
is overtaken by (e) or reads what (f) wrote; a hidden synchronisation drains the delay before (d).

The delay is as long as ``max(20 ms, 10 x the largest t_host seen so far)``: one ``torch.mm`` of the chain is timed once per session
with HIP events, and the chain is as many of them as that takes.  The factor 10 keeps host jitter from draining the queue before
(d); the floor keeps millisecond decodes behind it.

An entry is a callable on device tensors that returns a tensor, or a list / tuple / dict of them (None entries are skipped).  An entry
made of several library calls, of which only the first can be held to (d) (a later one may wait for the staging arena), returns
``Early(outputs, probe())`` with ``probe()`` taken right after its first call.
"""
import math
import os
import re
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DELAY_FLOOR_MS = 20.0
HOST_FACTOR = 10.0
MM_N = 2048
N_STREAMS = 2                     # rounds of steps 2 - 4, each on a fresh stream (why: the module docstring)


class ContractBreach(AssertionError):
    """``kind``: "values" (an output differs from the default-stream run) or "sync" (the delay ahead of the entry had drained when it returned)."""

    def __init__(self, kind, message):
        super().__init__(message)
        self.kind = kind


class Early:
    """What a multi-call entry returns: its outputs and ``probe()`` as it stood after the first call."""

    def __init__(self, outputs, busy):
        self.outputs, self.busy = outputs, busy


_marker = None                    # the event behind the delay of the run in progress (None during the reference runs)


def probe():
    """Is the delay of the run in progress still ahead of the entry's work?  (The reference runs have none: True.)"""
    return True if _marker is None else not _marker.query()


class Delay:
    """The matmul chain.  ``ms_per_mm`` is measured once; ``enqueue(ms)`` puts at least ``ms`` of it on the current stream."""

    def __init__(self):
        self.a = torch.full((MM_N, MM_N), 1.0 / MM_N, device="cuda")          # row sums 1: the chain stays finite
        self.x = [torch.ones(MM_N, MM_N, device="cuda"), torch.empty(MM_N, MM_N, device="cuda")]
        for _ in range(8):                                                     # load the kernel, settle the clocks
            self._chain(8)
        torch.cuda.synchronize()
        n = 64
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._chain(n)
        e1.record()
        torch.cuda.synchronize()
        self.ms_per_mm = e0.elapsed_time(e1) / n
        self.largest_t_host = 0.0
        self.last_ms = 0.0

    def _chain(self, n):
        for i in range(n):
            torch.mm(self.a, self.x[i & 1], out=self.x[(i + 1) & 1])

    def target_ms(self):
        return max(DELAY_FLOOR_MS, HOST_FACTOR * self.largest_t_host * 1e3)

    def enqueue(self):
        ms = self.target_ms()
        n = int(math.ceil(ms / self.ms_per_mm)) + 1
        self._chain(n)
        self.last_ms = n * self.ms_per_mm
        return self.last_ms


_delay = None
REPORT = []                       # (label, t_host, host time behind the delay, delay (ms), busy): printed by the test file


def delay():
    global _delay
    if _delay is None:
        _delay = Delay()
        print(f"\nstream harness: one {MM_N} x {MM_N} fp32 torch.mm = {_delay.ms_per_mm * 1e3:.1f} us; "
              f"delay floor {DELAY_FLOOR_MS:.0f} ms = {int(math.ceil(DELAY_FLOOR_MS / _delay.ms_per_mm)) + 1} of them")
    return _delay


def flatten(out):
    """The tensors of an entry's result, in a fixed order, with names for the messages."""
    if isinstance(out, Early):
        out = out.outputs
    if isinstance(out, torch.Tensor):
        return [("out", out)]
    if isinstance(out, dict):
        items = [(str(k), v) for k, v in out.items()]
    else:
        items = [(str(i), v) for i, v in enumerate(out)]
    flat = []
    for name, v in items:
        if v is None:
            continue
        if isinstance(v, torch.Tensor):
            flat.append((name, v))
        else:
            flat += [(f"{name}.{n}", t) for n, t in flatten(v)]
    return flat


def bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _pattern(t):
    return torch.full_like(t, 0.25 if t.is_floating_point() else 1)


def check_decoy(inputs, decoy):
    assert len(inputs) == len(decoy)
    for i, (t, d) in enumerate(zip(inputs, decoy)):
        assert t.shape == d.shape and t.dtype == d.dtype and t.device == d.device, f"decoy {i} does not match its input"
        if d.is_floating_point():
            assert torch.isfinite(d).all(), f"decoy {i} is not finite"


class Result:
    """``got[k]``: the clones of round k (``N_STREAMS`` rounds, one fresh stream each); ``result[name]`` is round 0's."""

    def __init__(self, label, names, ref, got, busy, t_host, delay_ms, expect_busy):
        self.label, self.names, self.ref, self.got = label, names, ref, got
        self.busy, self.t_host, self.delay_ms, self.expect_busy = busy, t_host, delay_ms, expect_busy

    def differing(self):
        return [f"{n} (stream {k})" for k, got in enumerate(self.got) for n, r, g in zip(self.names, self.ref, got)
                if r.shape != g.shape or r.dtype != g.dtype or not torch.equal(bits(r), bits(g))]

    def verify(self):
        bad = self.differing()
        if bad:
            raise ContractBreach("values", f"{self.label}: on a caller's stream these outputs differ from the default-stream run: {bad}")
        if self.expect_busy and not all(self.busy):
            raise ContractBreach("sync", f"{self.label}: the {self.delay_ms:.1f} ms delay ahead of the entry had drained when it returned "
                                         f"(the call takes {self.t_host * 1e3:.3f} ms of host time): it synchronised")
        return self

    def __getitem__(self, name):
        return self.got[0][self.names.index(name)]


def run(entry, inputs, decoy, *, expect_busy=True, reset=None, label="entry"):
    """Steps 1 - 4 of the module docstring; ``Result.verify()`` is step 4's comparison and step 5.  ``reset``: called before
    every run of the entry (a call that moves its handle's state starts each run from the same one); whatever it does is finished
    before the delay is enqueued."""
    global _marker
    inputs, decoy = list(inputs), list(decoy)
    check_decoy(inputs, decoy)
    d = delay()
    # 1. reference
    t_host = 0.0
    for _ in range(2):
        if reset is not None:
            reset()
        args = [t.clone() for t in inputs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = entry(*args)
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
    flat = flatten(out)
    names, ref = [n for n, _ in flat], [t.clone() for _, t in flat]
    del out, flat, args
    d.largest_t_host = max(d.largest_t_host, t_host)
    gots, busys, t_streams = [], [], []
    for _ in range(N_STREAMS):
        # 2. live buffers
        if reset is not None:
            reset()
        live = [t.clone() for t in decoy]
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        # 3. on the caller's stream
        with torch.cuda.stream(s):
            delay_ms = d.enqueue()                                     # (a)
            for buf, t in zip(live, inputs):                           # (b)
                buf.copy_(t, non_blocking=True)
            dirt = [_pattern(r) for r in ref]                          # (b')
            del dirt
            _marker = torch.cuda.Event()
            _marker.record(s)
            try:
                t0 = time.perf_counter()
                out = entry(*live)                                     # (c)
                t_streams.append(time.perf_counter() - t0)
                busy = not s.query() and probe()                       # (d)
            finally:
                _marker = None
            if isinstance(out, Early):
                busy = out.busy
            got = [t.clone() for _, t in flatten(out)]                 # (e)
            for buf, t in zip(live, decoy):                            # (f)
                buf.copy_(t, non_blocking=True)
        # 4. quiet
        s.synchronize()
        torch.cuda.synchronize()
        del out
        assert len(got) == len(ref), f"{label}: {len(got)} outputs on the stream, {len(ref)} in the reference"
        gots.append(got)
        busys.append(busy)
    t_stream = max(t_streams)
    print(f"{label}: t_host {t_host * 1e3:.3f} ms ({t_stream * 1e3:.3f} ms behind the delay), delay {delay_ms:.1f} ms, busy {busys}")
    REPORT.append((label, t_host * 1e3, t_stream * 1e3, delay_ms, all(busys)))
    return Result(label, names, ref, gots, busys, t_host, delay_ms, expect_busy)


def hold(entry, inputs, decoy, **kw):
    """``run`` and ``verify``."""
    return run(entry, inputs, decoy, **kw).verify()


# ------------------------------------------------------------------- what the file that keeps the header's table does with it
def check_entries_listed(entries, doc):
    """The entries of ``include/vqcpc.h`` that take a ``stream`` are exactly ``entries`` (name -> how), and each has its row in the
    table of ``doc``, the test file's docstring.  Returns the names found in the header."""
    text = open(os.path.join(ROOT, "include", "vqcpc.h")).read()
    found = set(re.findall(r"\bint\s+(vqcpc_\w+)\s*\([^;{]*?void\s*\*\s*stream\b[^;{]*?\)\s*;", text))
    assert found == set(entries), (sorted(found - set(entries)), sorted(set(entries) - found))
    for name, how in entries.items():
        assert re.search(r"^  %s\s+%s\W" % (name, how), doc, re.M), name
    return found


def release_after(*caches):
    """The body of a gradient file's module-wide fixture (``yield from`` it): when the file is done, the session-wide delay chain and
    report are left as they were found, ``caches`` (the dicts of cases and references the file filled) are cleared and the device
    buffers go back, so that the files that run after it find the process -- its heap, torch's caching allocator and the harness --
    as they would without it (tests/test_gpu_stream_contract.py then builds and times the delay chain itself, as it always did)."""
    global _delay
    found, reported = _delay, len(REPORT)
    yield
    import gc
    _delay = found
    del REPORT[reported:]
    for c in caches:
        c.clear()
    gc.collect()
    torch.cuda.empty_cache()
