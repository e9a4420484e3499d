"""Shared by tests/test_vocoder_sizes_cpu.py and tests/test_gpu_vocoder_sizes.py (plain module, not a conftest): the model sizes
``vqcpc_vocoder_create`` accepts, as cases; their float64 references; the fp32 yardstick; and the judge.

Cases.  Every accepted value of every dimension the kernels dispatch on appears at least once (asserted in the CPU test):
bits_mu_law 8 / 9 / 10, size_h_fc 256 / 512 / 768 / 1024, size_h_rnn 512 / 896 / 1024, dim_voc_latent / 2 of 64 / 128 / 256 / 512;
size_i_embed_ar and dim_i_embedding + dim_speaker_embedding from 32 up, multiples of 64 and not (96); upsampling_t from 6 to 200,
so that a run of a few hundred samples crosses many conditioning frames.  ``hf512`` is not in the table the work started from:
without it no case had size_h_fc 512.

Reference: ``oracle.f64_ref.F64Vocoder(sd, upsample=...)``.

Yardstick: the same class with ``dtype=torch.float32`` -- the same statements in fp32 on the CPU, on the same inputs -- and, on
row 0 of the same inputs, the C oracle (``oracle.vocoder_condition`` / ``vocoder_generate``), which sums in another order (one fma
chain per dot product).  The C oracle runs the first ORACLE_STEPS steps only (a serial chain costs ~10 ms per step at the largest
sizes); a shorter run can only make the tolerance below smaller.

Tolerance, per case and per quantity (conditioning, logits):  tol = 10 * max(e32, 2^-23 * max|ref|)  with e32 the larger of the
two yardsticks' max error against float64.  10 is the rule of tests/test_gpu_vocoder_f64.py (GPU tolerance = 10x the fp32
deviation from f64 on the CPU); the floor covers a case whose fp32 run happens to land closer to f64 than one rounding of the
largest value.  Nothing in it is measured on the GPU.

Draws: ``f64_ref.check_draws`` on the history the code under test drew itself, first input n_cls / 2: no draw outside
W = tol_logit + 4 ulp, and at least 99 % exactly the argmax of f64 logits + the protocol's noise.  The CPU test shows the
yardstick's own free run meets both on every input set the GPU test uses.
"""
import numpy as np
import torch

import oracle
import vectorquantizedcpc_amd as V
from oracle import f64_ref
from vectorquantizedcpc_amd import synth

SEED = 13
EXACT_SHARE = 0.99
ORACLE_STEPS = 96
ULP1 = 2.0 ** -23

#            bits h_rnn  h_fc   hp  embed  dz   ds  codebook speakers up
_TABLE = {
    "ref_small_glue":  (8, 896, 256, 64, 128, 32, 32, 64, 5, 40),
    "ref_wide_prenet": (8, 896, 256, 512, 512, 64, 96, 1024, 1, 200),
    "min":             (8, 512, 256, 64, 32, 16, 16, 64, 3, 6),
    "hf512":           (9, 896, 512, 256, 96, 32, 64, 100, 7, 24),
    "hf768":           (9, 512, 768, 128, 256, 64, 64, 512, 102, 16),
    "hf1024_b10":      (10, 896, 1024, 256, 64, 64, 64, 512, 102, 32),
    "hr1024":          (8, 1024, 256, 128, 256, 64, 64, 512, 102, 160),
    "max":             (10, 1024, 1024, 512, 512, 128, 128, 512, 102, 8),
    # not a size case of its own: hr1024 with size_h_rnn 512, the second model Vocoder.nll is checked on
    "hr512_refhead":   (8, 512, 256, 128, 256, 64, 64, 512, 102, 160),
}
_KEYS = ("bits", "h_rnn", "h_fc", "hp", "embed_ar", "dz", "ds", "codebook", "speakers", "up")
CASES = {name: dict(zip(_KEYS, row)) for name, row in _TABLE.items()}
NAMES = [n for n in CASES if n != "hr512_refhead"]
RESIDENT = ["ref_small_glue", "ref_wide_prenet"]          # the reference's 896 / 256 / 8 bit: the resident decoders take them
BIG = ["max", "hr1024", "min"]                            # run on the large-batch GRU kernel as well

_cache = {}


def conf(name, **override):
    c = dict(CASES[name], **override)
    cv = V.ConfVocoder()
    cv.size_i_codebook, cv.dim_i_embedding, cv.n_speakers, cv.dim_speaker_embedding = c["codebook"], c["dz"], c["speakers"], c["ds"]
    r = cv.rnnms
    r.dim_i_feature, r.dim_voc_latent, r.bits_mu_law, r.upsampling_t = c["dz"] + c["ds"], 2 * c["hp"], c["bits"], c["up"]
    r.wave_ar.size_i_embed_ar, r.wave_ar.size_h_rnn, r.wave_ar.size_h_fc = c["embed_ar"], c["h_rnn"], c["h_fc"]
    return cv


def state_dict(name, **override):
    c = dict(CASES[name], **override)
    return synth.vocoder_state_dict(size_i_codebook=c["codebook"], dim_i_embedding=c["dz"], n_speakers=c["speakers"],
                                    dim_speaker_embedding=c["ds"], dim_voc_latent=2 * c["hp"], size_i_embed_ar=c["embed_ar"],
                                    size_h_rnn=c["h_rnn"], size_h_fc=c["h_fc"], bits_mu_law=c["bits"])


def sd(name):
    if ("sd", name) not in _cache:
        _cache["sd", name] = state_dict(name)
    return _cache["sd", name]


def f64(name):
    if ("f64", name) not in _cache:
        _cache["f64", name] = f64_ref.F64Vocoder(sd(name), upsample=CASES[name]["up"])
    return _cache["f64", name]


def f32(name):
    """The yardstick."""
    if ("f32", name) not in _cache:
        _cache["f32", name] = f64_ref.F64Vocoder(sd(name), upsample=CASES[name]["up"], dtype=torch.float32)
    return _cache["f32", name]


def n_cls(name):
    return 1 << CASES[name]["bits"]


# ---------------------------------------------------------------------- inputs
def cond_inputs(name):
    """z (17, 17), spk (17): the conditioning test takes Tc in {1, 2, 17} x B in {1, 17} as z[:B, :Tc]."""
    c = CASES[name]
    return synth.randint(f"vsz/{name}/cz", (17, 17), c["codebook"]), synth.randint(f"vsz/{name}/cs", (17,), c["speakers"])


COND_TC = (1, 2, 17)


def tf_inputs(name, which):
    """Teacher-forced inputs, drawn from all n_cls classes: 'b2' B = 2, Tc = 3, the full 2 up Tc steps; 'b17' B = 17, Tc = 2."""
    c = CASES[name]
    B, Tc = (2, 3) if which == "b2" else (17, 2)
    z = synth.randint(f"vsz/{name}/tz{which}", (B, Tc), c["codebook"])
    spk = synth.randint(f"vsz/{name}/ts{which}", (B,), c["speakers"])
    x = synth.randint(f"vsz/{name}/tx{which}", (B, 2 * c["up"] * Tc), n_cls(name))
    return z, spk, x


def tf_lengths(name):
    up = CASES[name]["up"]
    return (1, up + 1, 2 * up * 3)


def draw_tc(name):
    """Codes per utterance of a free run: about 256 samples at the longest row, at least two codes so that rows can be ragged."""
    return max(2, round(128 / CASES[name]["up"]))


def ragged(B, Tc):
    return [Tc - (7 * b) % Tc if b else Tc for b in range(B)]


def draw_inputs(name, B):
    """(z, spk, n_codes, utt_ids) of the free run with B utterances; the sampling seed is SEED."""
    c = CASES[name]
    Tc = draw_tc(name)
    z = synth.randint(f"vsz/{name}/dz{B}", (B, Tc), c["codebook"])
    spk = synth.randint(f"vsz/{name}/ds{B}", (B,), c["speakers"])
    return z, spk, ragged(B, Tc), [3000 + 41 * b for b in range(B)]


ROWS80 = (0, 15, 16, 40, 63, 64, 79)                      # of the 80-utterance run: spread over its five tiles


def draw_rows(B):
    """Rows of a B-utterance free run that are checked draw by draw: all up to 8 utterances, else a subset that holds both ends
    of every 16-utterance tile in use (and so XCD 0 / 7 and local slots 0 / 3 of a 32-slot resident run)."""
    if B <= 8:
        return list(range(B))
    if B == 80:
        return list(ROWS80)
    return sorted({0, 1, 7, 15, 16, B // 2, B - 2, B - 1} & set(range(B)))


def nll_inputs(name):
    """A ragged scoring batch: B = 3, Tc = 2; row 0 full length, row 1 cut short in mid-frame, row 2 ends where its one code ends."""
    c = CASES[name]
    up2 = 2 * c["up"]
    n_codes = [2, 2, 1]
    lengths = [2 * up2, up2 + 37, up2 + 1]
    return dict(audio=synth.randint(f"vsz/{name}/na", (3, 2 * up2), n_cls(name)), z=synth.randint(f"vsz/{name}/nz", (3, 2), c["codebook"]),
                spk=synth.randint(f"vsz/{name}/ns", (3,), c["speakers"]), n_codes=n_codes, lengths=lengths)


# ---------------------------------------------------------------------- references and tolerances
def cond_reference(name, model=None):
    """{Tc: (17, 2 Tc, dl) array} of `model` (default float64) on cond_inputs."""
    key = ("cond", name) if model is None else None
    if key and key in _cache:
        return _cache[key]
    m = model or f64(name)
    z, spk = cond_inputs(name)
    out = {Tc: torch.stack(m.condition(z[:, :Tc], spk)).double().numpy() for Tc in COND_TC}
    if key:
        _cache[key] = out
    return out


def tf_reference(name, which, model=None):
    """(B, T, n_cls) logits of `model` (default float64) on tf_inputs, conditioned by the model itself."""
    key = ("tf", name, which) if model is None else None
    if key and key in _cache:
        return _cache[key]
    m = model or f64(name)
    z, spk, x = tf_inputs(name, which)
    out = m.logits(x, m.condition(z, spk)).double().numpy()
    if key:
        _cache[key] = out
    return out


def tolerances(name):
    """{'cond': (e32, tol, max|ref|), 'logit': (...)} of the case, from the yardsticks alone; computed once per process."""
    if ("tol", name) in _cache:
        return _cache["tol", name]
    c = CASES[name]
    s = sd(name)
    # conditioning
    want = cond_reference(name)
    got = cond_reference(name, f32(name))
    e_c = max(float(np.abs(got[Tc] - want[Tc]).max()) for Tc in COND_TC)
    z, spk = cond_inputs(name)
    e_c = max(e_c, float(np.abs(oracle.vocoder_condition(s, z[0].numpy(), int(spk[0]), upsample=c["up"]) - want[17][0]).max()))
    m_c = max(float(np.abs(want[Tc]).max()) for Tc in COND_TC)
    # logits
    e_l = m_l = 0.0
    for which in ("b2", "b17"):
        w = tf_reference(name, which)
        e_l = max(e_l, float(np.abs(tf_reference(name, which, f32(name)) - w).max()))
        m_l = max(m_l, float(np.abs(w).max()))
    z, spk, x = tf_inputs(name, "b2")
    n = min(ORACLE_STEPS, x.shape[1])
    r = oracle.vocoder_generate(s, z[0].numpy(), int(spk[0]), seed=0, n_steps=n, inputs=x[0].numpy(), want_logits=True,
                                upsample=c["up"], bits=c["bits"])
    e_l = max(e_l, float(np.abs(r["logits"] - tf_reference(name, "b2")[0, :n]).max()))
    out = {"cond": (e_c, 10.0 * max(e_c, ULP1 * m_c), m_c), "logit": (e_l, 10.0 * max(e_l, ULP1 * m_l), m_l)}
    _cache["tol", name] = out
    print("%s: yardstick e32 cond %.3g -> tol %.3g (max|ref| %.3g); logits %.3g -> tol %.3g (max|ref| %.3g)"
          % (name, e_c, out["cond"][1], m_c, e_l, out["logit"][1], m_l))
    return out


# ---------------------------------------------------------------------- the judge
def judge_cond(name, got, want, what=""):
    """Every frame of `got` against float64 `want` (same shapes): (ok, max error)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    tol = tolerances(name)["cond"][1]
    err = float(np.abs(got - want).max()) if got.size else 0.0
    print("%s %s: conditioning max |got - f64| = %.3g (tol %.3g)" % (name, what, err, tol))
    return bool(np.isfinite(got).all()) and err <= tol, err


def judge_logits(name, got, want, lengths=None, what=""):
    """(ok, max error) of teacher-forced logits over each row's valid steps."""
    tol = tolerances(name)["logit"][1]
    err, _ = f64_ref.logit_error(got, want, lengths, window=1 << 30)
    print("%s %s: logits max |got - f64| = %.3g (tol %.3g)" % (name, what, err, tol))
    return bool(np.isfinite(np.asarray(got)).all()) and err <= tol, err


def judge_draws(name, mu, z, spk, n_codes, ids, rows=None, seed=SEED, what=""):
    """Free-run draws `mu` (B, L) of utterances (z, spk, n_codes, ids), rows `rows` (default all) draw by draw against float64 on
    their own history: (ok, share of exact draws, worst gap, draws outside W, draws checked)."""
    c = CASES[name]
    f = f64(name)
    mu = np.asarray(mu)
    rows = list(range(mu.shape[0])) if rows is None else list(rows)
    lens = [2 * c["up"] * n_codes[b] for b in rows]
    n = max(lens)
    hist = np.concatenate([np.full((len(rows), 1), n_cls(name) // 2), mu[rows, : n - 1]], axis=1)
    lg = f.logits(hist, f.condition(z[rows], spk[rows], [n_codes[b] for b in rows]), lens).numpy()
    in_range = bool(((mu >= 0) & (mu < n_cls(name))).all())
    exact, gap, bad, first = f64_ref.check_draws(mu[rows, :n], lg, seed, [ids[b] for b in rows], lens, tolerances(name)["logit"][1])
    print("%s %s: %d draws on %d rows, exact %.5f, worst gap %.3g, outside W %d%s"
          % (name, what, sum(lens), len(rows), exact, gap, bad, "" if first is None else " (first at row %d step %d)" % (rows[first[0]], first[1])))
    return in_range and bad == 0 and exact >= EXACT_SHARE, exact, gap, bad, sum(lens)
