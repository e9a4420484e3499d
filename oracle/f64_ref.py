"""Float64 restatement of the vocoder spec, and the comparators that judge the GPU against it (TEST INFRASTRUCTURE).

The spec is the one ``vqcpc_oracle.c`` and ``torch_ref.py`` state in fp32: code and speaker embedding, x2 nearest upsample,
2-layer bidirectional GRU prenet, then per sample a GRU cell on ``[emb(x); cond[t // 160]]``, ``fc1``, ReLU, ``fc2``.  Here
every product and sum is float64, so a GPU error is bounded directly, not through a second fp32 summation order.

* Conditioning is per utterance on ``z[b, :n_codes[b]]``: the backward GRUs start at each utterance's own end (a ragged
  batch equals its utterances run one at a time).
* The sample loop is teacher-forced on a given history and batched over utterances.  The input half of the GRU is
  tabled: ``emb @ W_ih[:, :256]^T`` (256 rows) and ``cond @ W_ih[:, 256:]^T + b_ih`` (one row per frame), so a step is one
  ``h @ W_hh^T``, the gates, and a copy of h; fc1 / fc2 run afterwards as one GEMM per chunk of steps.
* Speed (8 host threads, one CPU process): B = 8 at ~2 900 steps/s, B = 1 at ~6 500 steps/s.
* Every size comes from the state dict and the hop (160 above) is the ``upsample`` argument.  ``dtype=torch.float32`` turns the
  class into an fp32 yardstick of itself, and ``generate`` runs it free (Gumbel-max on the protocol's noise): what
  tests/vocoder_size_cases.py sets its tolerances from at model sizes no other CPU statement covers.

``stressed(sd)`` is a second weight set that drives the decode into saturation without making the recurrence chaotic:
AR GRU W_ih, b_ih, b_hh x10, W_hh x0.7, fc2 weight and bias x16; prenet W_ih and biases x4.  W_hh of both GRUs stays at or
below 1x: W_hh x6 makes the recurrence chaotic, and fp32 then leaves f64 by O(1) within a few thousand steps.  Measured on CPU,
4 utterances x 6 400 steps teacher-forced on random samples:

  ==========  =========================  ==========  =====================================
  weight set  AR |pre-activation| max     logit std   max |torch_ref fp32 - f64| logit
  ==========  =========================  ==========  =====================================
  default     1.8 (none beyond 8)         0.06        6.8e-8, flat over 1 600-sample windows
  stressed    22.2 (3.6 % beyond 8)       2.9         7.5e-6, flat over 1 600-sample windows
  ==========  =========================  ==========  =====================================

The C oracle's prenet output against this module at Tc = 500: 5.4e-7 (default), 3.0e-6 (stressed); its logits over 480
steps: 1.7e-7 and 1.1e-5.
"""
import numpy as np
import torch

from vectorquantizedcpc_amd import synth

from . import torch_ref

WINDOW = 1600          # samples per reporting window of logit_error (10 conditioning frames)

_AR = "rnnms.ar."


def stressed(sd):
    """The stressed weight set (factors in the module docstring) as a new float32 state dict."""
    out = {k: v.clone() for k, v in sd.items()}
    for k in ("rnn.weight_ih_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0"):
        out[_AR + k] = sd[_AR + k] * 10.0
    out[_AR + "rnn.weight_hh_l0"] = sd[_AR + "rnn.weight_hh_l0"] * 0.7
    out[_AR + "fc2.weight"] = sd[_AR + "fc2.weight"] * 16.0
    out[_AR + "fc2.bias"] = sd[_AR + "fc2.bias"] * 16.0
    for layer in range(2):
        for suf in ("", "_reverse"):
            for k in ("weight_ih", "bias_ih", "bias_hh"):
                name = f"rnnms.prenet.{k}_l{layer}{suf}"
                out[name] = sd[name] * 4.0
    return out


def _d(t, dtype=torch.float64):
    return torch.as_tensor(t).detach().cpu().to(dtype)


def _gru_update(gi, gh, h):
    """One GRU cell update from the two projections (gate order r, z, n): h' = (1 - z) n + z h."""
    H = h.shape[-1]
    rz = torch.sigmoid(gi[..., : 2 * H] + gh[..., : 2 * H])
    n = torch.tanh(gi[..., 2 * H:] + rz[..., :H] * gh[..., 2 * H:])
    return n + rz[..., H:] * (h - n)


class F64Vocoder:
    """Every size comes from the state dict; ``upsample`` is ``upsampling_t``.  ``dtype=torch.float32`` runs the very same
    statements in fp32 on the CPU: the yardstick whose distance from float64 sets a GPU tolerance at sizes nothing else covers
    (tests/vocoder_size_cases.py)."""

    def __init__(self, sd, upsample=160, dtype=torch.float64):
        self.up = upsample
        self.dtype = dtype

        def w(t):
            return _d(t, dtype)

        self.code_emb = w(sd["code_embedding.weight"])
        self.spk_emb = w(sd["speaker_embedding.weight"])
        self.prenet = []
        for layer in range(2):
            dirs = []
            for suf in ("", "_reverse"):
                p = f"rnnms.prenet.%s_l{layer}{suf}"
                dirs.append((w(sd[p % "weight_ih"]), w(sd[p % "weight_hh"]), w(sd[p % "bias_ih"]), w(sd[p % "bias_hh"])))
            self.prenet.append(dirs)
        emb = w(sd[_AR + "embedding.weight"])
        w_ih = w(sd[_AR + "rnn.weight_ih_l0"])
        de = emb.shape[1]
        self.n_cls = emb.shape[0]
        self.emb_tab = emb @ w_ih[:, :de].T                       # (n_cls, 3 Hr)
        self.w_ih_cond = w_ih[:, de:]
        self.b_ih = w(sd[_AR + "rnn.bias_ih_l0"])
        self.w_hh_t = w(sd[_AR + "rnn.weight_hh_l0"]).T.contiguous()
        self.b_hh = w(sd[_AR + "rnn.bias_hh_l0"])
        self.Hr = self.w_hh_t.shape[0]
        self.fc1_w, self.fc1_b = w(sd[_AR + "fc1.weight"]), w(sd[_AR + "fc1.bias"])
        self.fc2_w, self.fc2_b = w(sd[_AR + "fc2.weight"]), w(sd[_AR + "fc2.bias"])

    # ------------------------------------------------------------------ prenet
    def _scan(self, x, w_ih, w_hh, b_ih, b_hh):
        """One GRU direction over (B, T, D), forward in time, h0 = 0."""
        B, T, _ = x.shape
        gi = x @ w_ih.T + b_ih
        w_hh_t = w_hh.T.contiguous()
        h = torch.zeros(B, w_hh.shape[1], dtype=self.dtype)
        out = torch.empty(B, T, w_hh.shape[1], dtype=self.dtype)
        for t in range(T):
            h = _gru_update(gi[:, t], torch.addmm(b_hh, h, w_hh_t), h)
            out[:, t] = h
        return out

    @staticmethod
    def _flip(x, lens):
        """Reverse each row within its own length (the padded tail stays behind it)."""
        out = x.clone()
        for b, n in enumerate(lens):
            out[b, :n] = x[b, :n].flip(0)
        return out

    @torch.no_grad()
    def condition(self, z, spk, n_codes=None):
        """Prenet output per utterance: a list of (2 n_codes[b], dim_voc_latent) tensors of the model's dtype."""
        z = torch.as_tensor(z).long().cpu()
        spk = torch.as_tensor(spk).long().cpu()
        B, Tc = z.shape
        n_codes = [Tc] * B if n_codes is None else [int(n) for n in n_codes]
        lens = [2 * n for n in n_codes]
        ze = self.code_emb[z].repeat_interleave(2, dim=1)                           # x2 nearest upsample
        x = torch.cat((ze, self.spk_emb[spk][:, None, :].expand(-1, 2 * Tc, -1)), dim=2)
        for layer in self.prenet:
            fwd = self._scan(x, *layer[0])
            bwd = self._flip(self._scan(self._flip(x, lens), *layer[1]), lens)
            x = torch.cat((fwd, bwd), dim=2)
        return [x[b, :lens[b]].clone() for b in range(B)]

    # ------------------------------------------------------------------ sample loop
    @torch.no_grad()
    def logits(self, inputs, cond, lengths=None, chunk=400):
        """Teacher-forced logits (B, T, n_cls) float64: ``inputs[b, t]`` is the sample fed at step t (the previous draw; the
        first is n_cls / 2), ``cond`` the list ``condition`` returns.  Steps at or past ``lengths[b]`` are left at 0."""
        inputs = torch.as_tensor(inputs).long().cpu()
        B, T = inputs.shape
        lengths = [T] * B if lengths is None else [min(int(n), T) for n in lengths]
        for b in range(B):
            assert lengths[b] <= self.up * cond[b].shape[0], "history longer than the conditioning covers"
        # per-frame input half of the gates, padded with the last frame of each utterance (values past lengths[b] unused)
        nf = max(c.shape[0] for c in cond)
        ctab = torch.empty(B, nf, 3 * self.Hr, dtype=self.dtype)
        for b, c in enumerate(cond):
            ctab[b, : c.shape[0]] = c @ self.w_ih_cond.T + self.b_ih
            ctab[b, c.shape[0]:] = ctab[b, c.shape[0] - 1]
        out = torch.zeros(B, T, self.n_cls, dtype=self.dtype)
        h = torch.zeros(B, self.Hr, dtype=self.dtype)
        rows = torch.arange(B)[:, None]
        for t0 in range(0, max(lengths), chunk):
            n = min(chunk, T - t0)
            t = torch.arange(t0, t0 + n)
            gi = (self.emb_tab[inputs[:, t0:t0 + n]] + ctab[rows, t // self.up]).transpose(0, 1).contiguous()   # (n, B, 3Hr)
            hs = torch.empty(n, B, self.Hr, dtype=self.dtype)
            for s in range(n):
                h = _gru_update(gi[s], torch.addmm(self.b_hh, h, self.w_hh_t), h)
                hs[s] = h
            a = torch.relu(torch.addmm(self.fc1_b, hs.view(n * B, self.Hr), self.fc1_w.T))
            out[:, t0:t0 + n] = torch.addmm(self.fc2_b, a, self.fc2_w.T).view(n, B, self.n_cls).transpose(0, 1)
        for b in range(B):
            out[b, lengths[b]:] = 0.0
        return out

    @torch.no_grad()
    def generate(self, cond, seed, utt_ids, lengths=None):
        """Free-running Gumbel-max decode in the model's dtype: (samples (B, T) int64, logits (B, T, n_cls)), T = the longest
        row; the first input is n_cls / 2, scores are logit + the protocol's fp32 noise, the draw is the first argmax.  Steps at
        or past ``lengths[b]`` (default: all the conditioning covers) are left at 0."""
        B = len(cond)
        full = [self.up * c.shape[0] for c in cond]
        lengths = full if lengths is None else [min(int(n), f) for n, f in zip(lengths, full)]
        T = max(lengths)
        gc = [c @ self.w_ih_cond.T + self.b_ih for c in cond]
        nz = torch.from_numpy(np.stack([noise(seed, [utt_ids[b]], 0, T, self.n_cls)[0] for b in range(B)])).to(self.dtype)
        x = torch.full((B,), self.n_cls // 2, dtype=torch.long)
        h = torch.zeros(B, self.Hr, dtype=self.dtype)
        samples = torch.zeros(B, T, dtype=torch.long)
        logits = torch.zeros(B, T, self.n_cls, dtype=self.dtype)
        for t in range(T):
            gi = self.emb_tab[x] + torch.stack([g[min(t // self.up, g.shape[0] - 1)] for g in gc])
            h = _gru_update(gi, torch.addmm(self.b_hh, h, self.w_hh_t), h)
            lg = torch.addmm(self.fc2_b, torch.relu(torch.addmm(self.fc1_b, h, self.fc1_w.T)), self.fc2_w.T)
            x = torch.argmax(lg + nz[:, t], dim=1)
            live = torch.tensor([t < n for n in lengths])
            samples[:, t] = torch.where(live, x, torch.zeros_like(x))
            logits[:, t] = lg * live[:, None].to(self.dtype)
        return samples, logits


# ---------------------------------------------------------------------- sampling protocol
def noise(seed, utt_ids, t0, n, n_cls=256):
    """Gumbel noise (len(utt_ids), n, n_cls) float32 of samples t0 .. t0 + n - 1: Philox(counter = (t, utt, k >> 2, 0),
    key = seed) word k & 3, converted as ``torch_ref.noise_from_words``."""
    utt = np.asarray(utt_ids, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    B, q = len(utt), n_cls // 4
    ctr = np.zeros((B * n * q, 4), np.uint32)
    ctr[:, 0] = np.tile(np.repeat(np.arange(t0, t0 + n, dtype=np.uint64), q), B).astype(np.uint32)
    ctr[:, 1] = np.repeat(utt, n * q).astype(np.uint32)
    ctr[:, 2] = np.tile(np.arange(q, dtype=np.uint32), B * n)
    w = synth.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)).reshape(B, n, n_cls)
    return torch_ref.noise_from_words(w).numpy()


# ---------------------------------------------------------------------- comparators
def logit_error(gpu, ref, lengths=None, window=WINDOW):
    """max |gpu - ref| over each row's valid steps: (overall, per-window maxima as an array) -- an error that grows late shows
    in the last windows."""
    gpu = np.asarray(gpu, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert gpu.shape == ref.shape, (gpu.shape, ref.shape)
    B, T = gpu.shape[:2]
    lengths = [T] * B if lengths is None else list(lengths)
    nw = (max(lengths) + window - 1) // window
    per = np.zeros(nw)
    for b in range(B):
        e = np.abs(gpu[b, : lengths[b]] - ref[b, : lengths[b]]).reshape(lengths[b], -1).max(axis=1)
        for w in range((lengths[b] + window - 1) // window):
            per[w] = max(per[w], float(e[w * window:(w + 1) * window].max()))
    return float(per.max()) if nw else 0.0, per


def ulp_f32(x):
    """Spacing of fp32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x)).astype(np.float32)).astype(np.float64)


def check_draws(mu, ref_logits, seed, utt_ids, lengths=None, tol_logit=0.0, chunk=4000):
    """Gumbel-max draws ``mu`` (B, T) against the reference logits on the same history.  Scores are the f64 logits plus the
    protocol's fp32 noise.  A draw is exact when it is the argmax of the scores; otherwise its score must lie within
    ``W = tol_logit + 4 ulp_f32(top score)`` of the top: the ulp term covers the fp32 rounding of logit + noise and the device
    logf against the host's.  Returns (fraction of exact draws, worst gap top - drawn, number of draws outside W, first such
    (row, step) or None)."""
    mu = np.asarray(mu)
    ref_logits = np.asarray(ref_logits)
    B, T = mu.shape
    lengths = [T] * B if lengths is None else list(lengths)
    exact = total = bad = 0
    worst = 0.0
    first = None
    for b in range(B):
        for t0 in range(0, lengths[b], chunk):
            n = min(chunk, lengths[b] - t0)
            sc = ref_logits[b, t0:t0 + n].astype(np.float64) + noise(seed, [utt_ids[b]], t0, n, ref_logits.shape[2])[0]
            top = sc.max(axis=1)
            got = np.take_along_axis(sc, mu[b, t0:t0 + n, None].astype(np.int64), axis=1)[:, 0]
            gap = top - got
            exact += int((gap == 0.0).sum())
            total += n
            worst = max(worst, float(gap.max()))
            out = np.nonzero(gap > tol_logit + 4.0 * ulp_f32(top))[0]
            if out.size and first is None:
                first = (b, t0 + int(out[0]))
            bad += int(out.size)
    return exact / max(total, 1), worst, bad, first
