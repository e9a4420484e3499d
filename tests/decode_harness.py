"""Shared by the decoder tests (test_gpu_xcd*.py, test_gpu_xcm.py, test_gpu_stream.py, test_gpu_vocoder.py; a plain module, not a
conftest): what all of them do around the decode loop.  Handles on the synthetic weights, options set for a scope and put back to
the library's defaults, seeded inputs and the ragged-length rules, one call on two decode paths compared bit for bit, and chunks of
generate_stream against one generate call.  The draw rule against the C oracle is oracle.judge_draws.  A new decoder test is a table
of shapes, and a docstring saying what each shape catches, over these.
"""
import contextlib

import torch

import vectorquantizedcpc_amd as V
from vectorquantizedcpc_amd import synth

FRAME = 320                       # samples per code frame

# what vqcpc_vocoder_create sets (csrc/vocoder_internal.h)
DEFAULTS = {"xcd": -1, "xcm": -1, "xcd_slots": 32, "xcm_slots": 128, "xcd_agent_stores": 0, "fuse_fc2": 1, "use_graph": 1,
            "steps_per_graph": 160, "two_groups": 1, "big_min_tiles": 5, "slots": 0, "tf_chunk_replays": 4}


def new_vocoder(conf=None, sd=None):
    """A handle of the caller's own, with the library's options, and its state dict: the default model on the synthetic weights, or
    a model of another size (``conf`` and its ``sd``)."""
    sd = sd or synth.vocoder_state_dict()
    v = V.Vocoder(conf or V.ConfVocoder())
    v.load_state_dict(sd)
    return v.to("cuda").eval(), sd


class Handles:
    """``vocoder = Handles()`` at the top of a test module: ``vocoder()`` is that module's one handle on the default model, built
    at the first call with ``options`` set on it for good; ``vocoder(fresh=True)`` or a ``conf`` gives a new_vocoder."""

    def __init__(self, **options):
        self.options, self.shared = options, None

    def __call__(self, fresh=False, conf=None, sd=None):
        if fresh or conf is not None:
            return new_vocoder(conf, sd)
        if self.shared is None:
            self.shared = new_vocoder()
            for k, val in self.options.items():
                self.shared[0].set_option(k, val)
        return self.shared


@contextlib.contextmanager
def options(voc, restore=DEFAULTS, **opts):
    """Sets ``opts``; yields ``set_option`` for more inside the scope; on exit every option set either way goes back to
    ``restore[name]``, once.  (Setting ``xcd`` re-arms a handle's fallback, so a scope makes no call of its own besides those.)"""
    touched = []

    def set_option(name, value):
        if name not in touched:
            touched.append(name)
        voc.set_option(name, value)
    try:
        for k, v in opts.items():
            set_option(k, v)
        yield set_option
    finally:
        for k in touched:
            voc.set_option(k, restore[k])


# ---- inputs

def inputs(tag, B, Tc, device="cuda"):
    """Code rows and speakers from the seeded generator; the ``?`` of ``tag`` is z for the codes and s for the speakers."""
    z = synth.randint(tag.replace("?", "z"), (B, Tc), 512)
    spk = synth.randint(tag.replace("?", "s"), (B,), 102)
    return z.to(device), spk.to(device)


def ragged_countdown(B, Tc):
    """Tc, Tc - 1, ..., 1, Tc, ...: every length, the longest first."""
    return [max(1, Tc - b % Tc) for b in range(B)]


def ragged_sevens(B, Tc):
    """1 + 7 b mod Tc: every length, neighbours differ."""
    return [1 + (7 * b) % Tc for b in range(B)]


def ragged_pairs(B):
    """1, 2, 2, 1, 2, 1, 1, 2, ...: both lengths in every XCD, in both granules of a 16-byte pair and in neighbouring pairs."""
    return [1 + ((b * 5 + b // 8) % 3 != 0) for b in range(B)]


# ---- one call, two paths

def decode(voc, z, spk, path=None, slots=None, **kw):
    """generate + check(), the path (and decode slots) asserted where stated; (wav, mu) on the CPU."""
    wav, mu = voc.generate(z, spk, return_mulaw=True, **kw)
    voc.check()
    assert path is None or voc.last_path() == path, (voc.last_path(), path)
    assert slots is None or voc.last_slots() == slots, (voc.last_slots(), slots)
    return wav.cpu(), mu.cpu()


def path_pair(voc, z, spk, resident, launch, path, slots=None, restore=DEFAULTS, **kw):
    """The same call under the options ``resident`` (which must take decode path ``path``, through ``slots`` slots if stated) and
    under ``launch`` (path 0, one launch per kernel and step), in one option scope: ((wav, mu), (wav, mu))."""
    with options(voc, restore) as set_option:
        out = []
        for opts, want_path, want_slots in ((resident, path, slots), (launch, 0, None)):
            for k, v in opts.items():
                set_option(k, v)
            out.append(decode(voc, z, spk, path=want_path, slots=want_slots, **kw))
    return out


def assert_same_bits(got, want):
    """(wav, mu) pairs: the mu-law classes, then the waveform."""
    assert got[1].shape == want[1].shape and got[0].shape == want[0].shape
    assert torch.equal(got[1].cpu(), want[1].cpu()) and torch.equal(got[0].cpu(), want[0].cpu())


def assert_live(mu, n_codes):
    """Not a decode that stopped early or wrote zeros: over 90 % of the classes of ``n_codes`` code frames are not class 0."""
    assert int((mu != 0).sum()) > 0.9 * FRAME * sum(n_codes)


def reference_bits(z, spk, **kw):
    """The bits of a handle nothing has happened to, on the plainest path: three launches per step."""
    ref, _ = new_vocoder()
    ref.set_option("xcd", 0)
    ref.set_option("fuse_fc2", 0)
    return decode(ref, z, spk, **kw)


class CutCases:
    """A family of cases on a module's shared handle: B utterances of ``Tc`` code frames from ``tag`` (``{B}`` in it is the batch),
    cut at ``steps`` samples, or, ragged, run out at the ragged_pairs lengths; the resident decoders (``xcd`` 1, path 2) against
    the launch-per-step kernels, whose bits are computed once per case."""

    def __init__(self, handles, tag, Tc, steps, seed, utt_base):
        self.handles, self.tag, self.Tc, self.steps, self.seed, self.utt_base = handles, tag, Tc, steps, seed, utt_base
        self.launch = {}

    def inputs(self, B, ragged):
        return (*inputs(self.tag.format(B=B), B, self.Tc), ragged_pairs(B) if ragged else None)

    def _decode(self, B, ragged, path, **kw):
        z, spk, n_codes = self.inputs(B, ragged)
        return decode(self.handles()[0], z, spk, path=path, n_codes=n_codes, seed=self.seed, utt_base=self.utt_base,
                      max_steps=0 if ragged else self.steps, **kw)

    def launch_bits(self, B, ragged):
        if (B, ragged) not in self.launch:
            with options(self.handles()[0], xcd=0):
                self.launch[B, ragged] = self._decode(B, ragged, 0)
        return self.launch[B, ragged]

    def resident(self, B, ragged, **opts):
        """Only enqueued, so check() is what says that no hand-off timed out."""
        with options(self.handles()[0], xcd=1, **opts):
            return self._decode(B, ragged, 2, async_=True)

    def assert_equal(self, got, B, ragged):
        """Equal to the launch path's bits, live, and nothing behind an utterance's end."""
        assert_same_bits(got, self.launch_bits(B, ragged))
        n_codes = ragged_pairs(B) if ragged else [self.steps // FRAME] * B
        assert_live(got[1], n_codes)
        for b, n in enumerate(n_codes):
            assert not got[1][b, FRAME * n:].any()

    def assert_stream_equals_one_shot(self, B, chunk):
        """The first code frame of a case: streamed in chunks on the resume kernels, in one call on the launch path."""
        voc = self.handles()[0]
        z, spk, _ = self.inputs(B, False)
        z = z[:, :1].contiguous()
        with options(voc, xcd=0) as set_option:
            want = voc.generate(z, spk, seed=self.seed, utt_base=self.utt_base, return_mulaw=True)
            set_option("xcd", 1)
            got = streamed(voc, z, spk, chunk, path=2, chunks=FRAME // chunk, seed=self.seed, utt_base=self.utt_base)
            voc.check()
        assert want[1].shape[1] == FRAME
        assert_live(want[1], [1] * B)
        assert_same_bits(got, want)


# ---- chunks of generate_stream against one generate call

def streamed(voc, z, spk, chunk, path=None, slots=None, chunks=None, **kw):
    """Every chunk of a stream, concatenated: each as wide as asked for (the last one what is left), on decode path ``path``
    through ``slots`` = (fewest, most) slots and ``chunks`` of them in all, where stated."""
    st = voc.generate_stream(z, spk, chunk_samples=chunk, return_mulaw=True, **kw)
    ws, ms = [], []
    total = st.position[1]
    for w, m in st:
        assert path is None or voc.last_path() == path
        assert slots is None or slots[0] <= voc.last_slots() <= slots[1]
        assert w.shape[1] == min(chunk, total - sum(x.shape[1] for x in ws))
        ws.append(w)
        ms.append(m)
    assert chunks is None or len(ws) == chunks
    return torch.cat(ws, 1), torch.cat(ms, 1)


def assert_same(voc, z, spk, chunk, path=None, seed=17, utt_base=5, **kw):
    """One generate call, then the same call streamed, on the handle as it stands."""
    want = voc.generate(z, spk, return_mulaw=True, seed=seed, utt_base=utt_base, **kw)
    got = streamed(voc, z, spk, chunk, path=path, seed=seed, utt_base=utt_base, **kw)
    assert_same_bits(got, want)
    assert int((got[1] != 0).sum()) > 0.9 * int((want[1] != 0).sum()) > 0
    return want
