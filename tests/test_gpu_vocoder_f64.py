"""-m gpu: the vocoder against the float64 reference (oracle/f64_ref.py) over whole utterances, on every decode form.

The other vocoder tests compare the GPU with fp32 oracles over the first few hundred samples, and otherwise path with path.
Here every conditioning frame, every teacher-forced logit up to 32 000 samples and every free-running draw of ragged
utterances (one of them 160 000 samples long) is compared with float64, on the default weights and on f64_ref.stressed()
(saturating GRU gates, peaked logits).  Each case asserts the decode path (and slot count) it ran.

Tolerances (absolute, about 10x the fp32 deviation of torch_ref from f64 on CPU, tests/test_f64_ref_cpu.py):
  conditioning 2e-6 / 2e-5, logits 1e-6 / 5e-5 (default / stressed weights);
  draws: >= 99.99 % exactly the argmax of f64 logits + the protocol's noise, every other draw within
  W = logit tolerance + 4 ulp_f32(top score) of the top (f64_ref.check_draws).
Observed maxima on MI355X (printed by each case): conditioning 6.0e-7 / 3.4e-6; logits 2.2e-7 / 1.4e-5, flat over the
1 600-sample windows up to 32 000 samples (torch_ref fp32 on CPU: 6.8e-8 / 7.5e-6); every one of the 317 760 draws checked
is exact, on every decode form and both weight sets.

Also here: the gate functions of the decode (gate_sigmoid / gate_tanh, ar_shared.h) and the libm gates of the scans, element
by element against numpy float64 (csrc/gate_probe.hip), and bad indices through forward / glue / condition.
"""
import numpy as np
import pytest
import torch

import oracle
import vectorquantizedcpc_amd as V
from oracle import f64_ref
from vectorquantizedcpc_amd import _lib, synth

pytestmark = pytest.mark.gpu

SEED = 13
LOGIT_TOL = {"default": 1e-6, "stressed": 5e-5}
COND_TOL = {"default": 2e-6, "stressed": 2e-5}
DEFAULTS = {"xcd": -1, "xcm": -1, "big_min_tiles": 5, "slots": 0}
MULAW = np.array([oracle.mulaw_decode(k) for k in range(256)], np.float32)
_cache = {}


def setup(name):
    if name not in _cache:
        sd = synth.vocoder_state_dict()
        if name == "stressed":
            sd = f64_ref.stressed(sd)
        v = V.Vocoder(V.ConfVocoder())
        v.load_state_dict(sd)
        _cache[name] = (v.to("cuda").eval(), sd, f64_ref.F64Vocoder(sd))
    return _cache[name]


# ---------------------------------------------------------------------- conditioning
@pytest.mark.parametrize("name", ["default", "stressed"])
def test_conditioning_every_frame(name):
    """Vocoder.condition at Tc in {1, 2, 3, 17, 100, 500} x B in {1, 16, 17, 33} (the scans work on tiles of 16 utterances)."""
    voc, _, f = setup(name)
    worst = 0.0
    for Tc in (1, 2, 3, 17, 100, 500):
        z = synth.randint(f"f64cond/z{Tc}", (33, Tc), 512)
        spk = synth.randint(f"f64cond/s{Tc}", (33,), 102)
        want = torch.stack(f.condition(z, spk)).numpy()
        for B in (1, 16, 17, 33):
            got = voc.condition(z[:B].cuda(), spk[:B].cuda()).cpu().numpy()
            assert got.shape == (B, 2 * Tc, 256)
            e = np.abs(got - want[:B]).max(axis=(0, 2))                     # per frame
            worst = max(worst, float(e.max()))
            assert e.max() <= COND_TOL[name], (Tc, B, int(e.argmax()), float(e.max()))
    print("%s: conditioning, max |GPU - f64| = %.3g" % (name, worst))


# ---------------------------------------------------------------------- teacher-forced logits
@pytest.mark.parametrize("name", ["default", "stressed"])
def test_teacher_forced_logits_full_length(name):
    """Vocoder.forward at Tc = 100 for Ts in {1, 161, 31999, 32000} (B = 2), and B = 17 at Tc = 8 (2 560 samples)."""
    voc, _, f = setup(name)
    z = synth.randint("f64tf/z", (2, 100), 512)
    spk = synth.randint("f64tf/s", (2,), 102)
    x = synth.randint("f64tf/x", (2, 32000), 256)
    want = f.logits(x, f.condition(z, spk)).numpy()
    for Ts in (1, 161, 31999, 32000):
        got = voc(x[:, :Ts].cuda(), z.cuda(), spk.cuda()).cpu().numpy()
        assert voc.last_path() == 0
        err, per = f64_ref.logit_error(got, want[:, :Ts])
        print("%s: logits Tc 100, Ts %d, max |GPU - f64| = %.3g, by 1600-sample window %s" % (name, Ts, err, np.array2string(per, precision=2)))
        assert err <= LOGIT_TOL[name], (Ts, err)
    z = synth.randint("f64tf/z17", (17, 8), 512)
    spk = synth.randint("f64tf/s17", (17,), 102)
    x = synth.randint("f64tf/x17", (17, 2560), 256)
    got = voc(x.cuda(), z.cuda(), spk.cuda()).cpu().numpy()
    err, per = f64_ref.logit_error(got, f.logits(x, f.condition(z, spk)).numpy())
    print("%s: logits B 17, Tc 8, max |GPU - f64| = %.3g" % (name, err))
    assert err <= LOGIT_TOL[name]


# ---------------------------------------------------------------------- free-running decode
def _free_run(name, tag, B, n_codes, opts, path, slots=None, rows=None, seed=SEED):
    """Full-length generate() under `opts` on ragged utterances; rows `rows` (default all) checked draw by draw against f64 on
    the GPU's own history; waveform = mu-law table of the draws, zeros behind each utterance."""
    voc, _, f = setup(name)
    Tc = max(n_codes)
    z = synth.randint(f"f64fr/{tag}/z", (B, Tc), 512)
    spk = synth.randint(f"f64fr/{tag}/s", (B,), 102)
    ids = [7000 + 37 * b for b in range(B)]
    try:
        for k, v in opts.items():
            voc.set_option(k, v)
        wav, mu = voc.generate(z.cuda(), spk.cuda(), n_codes=n_codes, seed=seed, utt_ids=ids, return_mulaw=True)
        got_path, got_slots = voc.last_path(), voc.last_slots()
    finally:
        for k in opts:
            voc.set_option(k, DEFAULTS[k])
    assert got_path == path, (tag, got_path)
    if slots is not None:
        assert got_slots == slots, (tag, got_slots)
    wav, mu = wav.cpu().numpy(), mu.cpu().numpy()
    lengths = [320 * n for n in n_codes]
    for b in range(B):
        L = lengths[b]
        assert np.array_equal(wav[b, :L], MULAW[mu[b, :L]]), (tag, b)
        assert not wav[b, L:].any() and not mu[b, L:].any(), (tag, b)
    rows = sorted(range(B) if rows is None else rows, key=lambda b: lengths[b])
    n_exact = n_all = 0
    worst = 0.0
    for g in range(0, len(rows), 8):                         # f64 in groups of similar length
        grp = rows[g:g + 8]
        rl = [lengths[b] for b in grp]
        n = max(rl)
        hist = np.concatenate([np.full((len(grp), 1), 128), mu[grp, : n - 1]], axis=1)
        lg = f.logits(hist, f.condition(z[grp], spk[grp], [n_codes[b] for b in grp]), rl).numpy()
        exact, gap, bad, first = f64_ref.check_draws(mu[grp, :n], lg, seed, [ids[b] for b in grp], rl, LOGIT_TOL[name])
        assert bad == 0, (tag, grp[first[0]], first[1])
        n_exact += round(exact * sum(rl))
        n_all += sum(rl)
        worst = max(worst, gap)
    print("%s %s: %d draws on %d rows, exact %.6f, worst gap %.3g, all within W" % (name, tag, n_all, len(rows), n_exact / n_all, worst))
    assert n_exact >= 0.9999 * n_all, (tag, n_exact, n_all)


def _ragged(B, Tc):
    return [Tc - (7 * b) % Tc if b else Tc for b in range(B)]


@pytest.mark.parametrize("name", ["default", "stressed"])
def test_launch_path_small_kernel(name):
    _free_run(name, "launch5", 5, _ragged(5, 10), {"xcd": 0}, path=0)


def test_launch_path_large_batch_kernel():
    """80 utterances = 5 tiles: ar_gru_big_kernel; rows spread over the tiles."""
    _free_run("default", "launch80", 80, _ragged(80, 5), {"xcd": 0, "big_min_tiles": 5}, path=0,
              rows=(0, 15, 16, 40, 63, 64, 79))


def test_xcd_one_slot():
    _free_run("default", "xcd5", 5, _ragged(5, 10), {"xcd": 1}, path=2, slots=5)


def test_xcd_two_slots():
    _free_run("default", "xcd12", 12, _ragged(12, 6), {"xcd": 1}, path=2, slots=12)


@pytest.mark.parametrize("name", ["default", "stressed"])
def test_xcd_four_slots(name):
    """32 utterances: four slots on each XCD; every row checked (covers XCDs 0 and 7, local slots 0 and 3)."""
    _free_run(name, "xcd32", 32, _ragged(32, 5), {"xcd": 1}, path=2, slots=32)


@pytest.mark.parametrize("name", ["default", "stressed"])
def test_xcm_19(name):
    _free_run(name, "xcm19", 19, _ragged(19, 5), {"xcm": 1}, path=3, slots=19)


def test_xcm_128():
    _free_run("default", "xcm128", 128, _ragged(128, 3), {"xcm": 1}, path=3, slots=128,
              rows=(0, 1, 15, 16, 63, 64, 100, 127))


def test_ten_second_utterance_alone_at_the_tail():
    """One 10 s utterance (Tc 500, 160 000 samples) among 39 short ones on the default path: 32 resident slots, the others
    run back to back in 31 of them while the long one runs on, and finishes alone."""
    n_codes = [500] + [1 + b % 4 for b in range(39)]
    _free_run("default", "long40", 40, n_codes, {}, path=2, slots=32, rows=(0, 1, 39))


# ---------------------------------------------------------------------- gate functions
ULP1 = 2.0 ** -23


def _probe(v):
    v = np.ascontiguousarray(v, dtype=np.float32)
    dv = torch.from_numpy(v).cuda()
    out = torch.empty(4, v.size, device="cuda")
    _lib.check(_lib.load().vqcpc_probe_gates(dv.data_ptr(), v.size, out.data_ptr(), _lib.current_stream()))
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


def _want(v):
    with np.errstate(over="ignore", invalid="ignore"):          # signalling-NaN bit patterns warn in the cast
        d = v.astype(np.float64)
        s = 1.0 / (1.0 + np.exp(-d))
    return s, np.tanh(d)


def _inputs():
    every256 = (np.arange(0, 2 ** 32, 256, dtype=np.uint64).astype(np.uint32)).view(np.float32)
    pos = np.arange(0, 0x3F800001, 64, dtype=np.uint32).view(np.float32)
    dense = np.concatenate([pos, -pos])
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    sub = np.array([1, 2, 0x400000, 0x7FFFFF], np.uint32).view(np.float32)
    edges = []
    for t in (9.1, -9.1, 8.0, -8.0, 16.0, 17.0, -17.0, 44.0, -44.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0):
        bits = int(np.array([t], np.float32).view(np.uint32)[0])          # 4 000 neighbours of each edge
        edges.append(np.arange(bits - 2000, bits + 2000, dtype=np.int64).astype(np.uint32).view(np.float32))
    edges = np.concatenate(edges)
    return every256, dense, np.concatenate([special, sub, -sub, edges])


def test_gate_functions_against_float64():
    """gate_sigmoid / gate_tanh (v_exp_f32 + v_rcp_f32) and sigmoidf_ / tanhf (libm) on every 256th fp32 bit pattern, every
    64th in [-1, 1], the specials and the saturation edges: range, exact ends (sigmoid 1 from 17 up and 0 from -89 down, tanh
    +-1 from |v| = 9.1), NaN propagation, monotone within an output ulp, and the absolute error against float64.
    Observed on MI355X, in units of 2^-23: gate_sigmoid 0.89 (at 3.55), gate_tanh 1.78 (at -1.78), sigmoidf_ 0.75,
    tanhf 0.68; pinned at 1, 2, 1, 1."""
    names = ("gate_sigmoid", "gate_tanh", "sigmoidf_", "tanhf")
    err = dict.fromkeys(names, 0.0)
    worst_at = dict.fromkeys(names, None)
    problems = []
    sets = _inputs()
    for si, v in enumerate(sets):
        for c0 in range(0, v.size, 1 << 22):
            vc = v[c0:c0 + (1 << 22)]
            out = _probe(vc)
            ws, wt = _want(vc)
            nan = np.isnan(vc)
            for i, nm in enumerate(names):
                o = out[i]
                if not np.isnan(o[nan]).all():
                    problems.append((nm, "NaN in, not NaN out"))
                o, ok = o[~nan], vc[~nan]
                lo = 0.0 if i % 2 == 0 else -1.0
                if not ((o >= lo) & (o <= 1.0)).all():
                    problems.append((nm, "out of range", float(ok[~((o >= lo) & (o <= 1.0))][0])))
                want = (ws if i % 2 == 0 else wt)[~nan]
                e = np.abs(o.astype(np.float64) - want)
                if e.size and e.max() > err[nm]:
                    err[nm] = float(e.max())
                    worst_at[nm] = float(ok[e.argmax()])
                if i % 2 == 0:
                    hi_end, lo_end = ok >= 17.0, ok <= -89.0
                    if not (o[hi_end] == 1.0).all() or not (o[lo_end] == 0.0).all():
                        problems.append((nm, "sigmoid end not exact"))
                else:
                    if not (o[ok >= 9.1] == 1.0).all() or not (o[ok <= -9.1] == -1.0).all():
                        problems.append((nm, "tanh end not exact"))
            if si < 2:                                           # monotone within one output ulp, in input order
                order = np.argsort(vc[~np.isnan(vc)], kind="stable")
                for i, nm in enumerate(names):
                    o = out[i][~np.isnan(vc)][order]
                    d = np.diff(o.astype(np.float64))
                    if (d < -np.spacing(np.abs(o[:-1]))).any():
                        problems.append((nm, "not monotone", int((d < -np.spacing(np.abs(o[:-1]))).sum())))
    print("gates, max |GPU - float64| (in units of 2^-23):",
          {nm: "%.3f at %r" % (err[nm] / ULP1, worst_at[nm]) for nm in names})
    assert not problems, problems[:10]
    assert err["gate_sigmoid"] <= 1.0 * ULP1 and err["gate_tanh"] <= 2.0 * ULP1
    assert err["sigmoidf_"] <= 1.0 * ULP1 and err["tanhf"] <= 1.0 * ULP1


# ---------------------------------------------------------------------- bad indices
def test_bad_index_raises_in_forward_glue_condition_and_does_not_latch():
    sd = synth.vocoder_state_dict()
    voc = V.Vocoder(V.ConfVocoder())
    voc.load_state_dict(sd)
    voc = voc.to("cuda").eval()
    z = synth.randint("bad/z", (2, 3), 512).cuda()
    spk = synth.randint("bad/s", (2,), 102).cuda()
    x = synth.randint("bad/x", (2, 100), 256).cuda()
    bad_z, bad_spk = z.clone(), spk.clone()
    bad_z[1, 2] = 512
    bad_spk[0] = 102
    for zz, ss in ((bad_z, spk), (z, bad_spk)):
        with pytest.raises(IndexError):
            voc(x, zz, ss)
        with pytest.raises(IndexError):
            voc.glue(zz, ss)
        with pytest.raises(IndexError):
            voc.condition(zz, ss)
    got = voc.generate(z, spk, seed=5, utt_base=0, return_mulaw=True)
    fresh = V.Vocoder(V.ConfVocoder())
    fresh.load_state_dict(sd)
    fresh = fresh.to("cuda").eval()
    want = fresh.generate(z, spk, seed=5, utt_base=0, return_mulaw=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
