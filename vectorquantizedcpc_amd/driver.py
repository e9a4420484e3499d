"""Batched, length-bucketed drivers for the reference's per-utterance loops.

``encode.py:42-46`` and ``convert.py:52-77`` process ONE utterance per call.  On a GPU the
throughput comes from batching, so these drivers bucket utterances by length, zero-pad inside a
bucket and call the batched HIP path -- while returning, for every utterance, exactly what a
batch-1 call on that utterance alone returns:

* zero right-padding is exact for the valid frames: ``nn.Conv1d(k=4, s=2, p=1)`` zero-pads there
  anyway (``model.py:43``), everything after it is per-frame or causal (LSTM, AR loop);
* the reference's conv back-end (and with it the fp32 summation order) depends on the CALL SHAPE
  (``vqcpc.h``: conv_mode).  A batch-1 call uses im2col order up to 256 frames and the oneDNN order
  above, so buckets never mix the two classes and pass the batch-1 mode explicitly;
* every utterance keeps its own sampling-stream id (``utt_ids``), so the drawn samples do not
  depend on the bucketing.
"""
from typing import List, Optional, Sequence

import torch

from . import _lib, synth
from .model import CPCLoss, Encoder
from .network_vocoder import Vocoder


def out_frames(T: int) -> int:
    """Code frames of a T-frame mel: Conv1d(k=4, s=2, p=1) output length (``model.py:43``)."""
    return (T - 2) // 2 + 1


def batch1_conv_mode(in_channels: int, T: int) -> int:
    """Back-end ATen picks for a (1, C, T) call: 1 = im2col, 2 = oneDNN direct (``vqcpc.h``)."""
    return 2 if in_channels * T > 20480 else 1


def make_buckets(lengths: Sequence[int], modes: Sequence[int], max_batch: int, max_pad_frac: float):
    """Greedy buckets over utterances sorted by (mode, length): at most ``max_batch`` members and
    at most ``max_pad_frac`` of a bucket's frames are padding."""
    order = sorted(range(len(lengths)), key=lambda i: (modes[i], lengths[i], i))
    buckets, cur = [], []
    for i in order:
        if cur:
            lo, hi = lengths[cur[0]], lengths[i]
            total = sum(lengths[j] for j in cur) + lengths[i]
            too_padded = hi * (len(cur) + 1) - total > max_pad_frac * hi * (len(cur) + 1)
            if len(cur) >= max_batch or modes[i] != modes[cur[0]] or too_padded or lo <= 0:
                buckets.append(cur)
                cur = []
        cur.append(i)
    if cur:
        buckets.append(cur)
    return buckets


def _pad_batch(rows, device, dtype=torch.float32, min_len: int = 0, non_blocking: bool = False) -> torch.Tensor:
    """Rows (tensors or arrays, anywhere) that differ in their last dimension only -> one zero-initialised batch
    (len(rows), ..., longest) of ``dtype`` on ``device``, every row at the front of its slot (one copy per row)."""
    rows = [torch.as_tensor(r, dtype=dtype) for r in rows]
    longest = max(min_len, max(int(r.shape[-1]) for r in rows))
    out = torch.zeros(len(rows), *rows[0].shape[:-1], longest, dtype=dtype, device=device)
    for k, r in enumerate(rows):
        out[k, ..., : r.shape[-1]].copy_(r, non_blocking=non_blocking)
    return out


@torch.no_grad()
def encode_utterances(encoder: Encoder, mels: Sequence[torch.Tensor], want_context: bool = False,
                      max_batch: int = 64, max_pad_frac: float = 0.25):
    """``encode.py:42-46`` over a list of (80, T_i) mels -> list of dicts with the per-utterance
    ``z`` (T_i', 64), ``indices`` (T_i') and, if asked, ``c`` (T_i', 256)."""
    dev = next(encoder.parameters()).device
    C = encoder.conf.in_channels
    lengths = [int(m.shape[-1]) for m in mels]
    modes = [batch1_conv_mode(C, t) for t in lengths]
    out: List[Optional[dict]] = [None] * len(mels)
    for ids in make_buckets(lengths, modes, max_batch, max_pad_frac):
        batch = _pad_batch([mels[i] for i in ids], dev)
        run = lambda: encoder._encode_native(batch, want_c=want_context, conv_mode=modes[ids[0]])
        if want_context:                         # the resident context scan of a one-utterance call may have given up
            z, c, idx, _ = _lib.run_checked(run, encoder.check, "encode repeated on the fallback path: {}")
        else:
            z, c, idx, _ = run()
        for k, i in enumerate(ids):
            n = out_frames(lengths[i])
            out[i] = {"z": z[k, :n], "indices": idx[k, :n], "c": c[k, :n] if want_context else None}
    return out


@torch.no_grad()
def adapt_codebook(encoder: Encoder, mels: Sequence[torch.Tensor], epochs: int = 1, max_batch: int = 64,
                   max_pad_frac: float = 0.25):
    """Fit the encoder's codebook to a corpus: ``Encoder.adapt_codebook`` (front end + the EMA update of ``model.py:136-145``,
    no gradient) over the length buckets of ``encode_utterances``, ``epochs`` times, in a fixed order -- buckets by
    (conv mode, length), the same every epoch -- so a run is reproducible.  Padding rows take no part (``n_frames``).  Returns
    ``{"loss": [[...] per epoch], "perplexity": ..., "rows": rows per batch, "codes_in_use": per epoch}``: loss / perplexity of
    every batch under the codebook as it was before that batch; ``codes_in_use`` = the distinct codes the rows of that epoch
    were assigned to, from the indices of the update calls themselves (``ema_count`` cannot tell: a code no row reaches settles
    at epsilon / (1 - decay), not at zero).  Everything is read back once at the end."""
    dev = next(encoder.parameters()).device
    C = encoder.conf.in_channels
    lengths = [int(m.shape[-1]) for m in mels]
    modes = [batch1_conv_mode(C, t) for t in lengths]
    buckets = make_buckets(lengths, modes, max_batch, max_pad_frac)
    batches = [(_pad_batch([mels[i] for i in ids], dev), [out_frames(lengths[i]) for i in ids], modes[ids[0]]) for ids in buckets]
    n_epochs = int(epochs)
    stats = torch.zeros(n_epochs, len(batches), 2, device=dev)
    hit = torch.zeros(n_epochs, encoder.conf.n_embeddings, dtype=torch.bool, device=dev)
    for e in range(n_epochs):
        for k, (batch, n_frames, mode) in enumerate(batches):
            loss, ppl, idx = encoder.adapt_codebook(batch, n_frames, conv_mode=mode, return_indices=True)
            stats[e, k, 0], stats[e, k, 1] = loss, ppl
            hit[e, idx] = True
    host, used = stats.cpu(), hit.sum(dim=1).cpu()
    return {"loss": host[..., 0].tolist(), "perplexity": host[..., 1].tolist(), "rows": [sum(n) for _, n, _ in batches],
            "codes_in_use": [int(u) for u in used]}


@torch.no_grad()
def convert_utterances(encoder: Encoder, vocoder: Vocoder, mels: Sequence[torch.Tensor], speakers: Sequence[int],
                       seed: int, utt_ids: Optional[Sequence[int]] = None, max_batch: int = 64,
                       max_pad_frac: float = 0.25, slots: int = 0, clock=None,
                       mem_budget_bytes: int = 8 << 30) -> List[torch.Tensor]:
    """``convert.py:72-77`` over a list of utterances -> list of 1-D waveforms (160 * 2 * T_i' samples).

    ``slots`` > 0: continuous batching -- decode calls over as many utterances as ``mem_budget_bytes`` of device work space
    allow (see ``decode_chunks``; the reference's 9 474-utterance set, ``README.md:125``, is ~35 GB of conditioning rows in one
    call), each with that many decode slots, a slot running utterances back to back (longest first), instead of one call per
    length bucket.  The samples are the same either way (per-utterance sampling streams).
    """
    dev = next(encoder.parameters()).device
    C = encoder.conf.in_channels
    up = vocoder.conf.rnnms.upsampling_t
    lengths = [int(m.shape[-1]) for m in mels]
    modes = [batch1_conv_mode(C, t) for t in lengths]
    utt_ids = list(range(len(mels))) if utt_ids is None else list(utt_ids)
    n_codes_all = [out_frames(t) for t in lengths]
    out: List[Optional[torch.Tensor]] = [None] * len(mels)
    codes: List[Optional[torch.Tensor]] = [None] * len(mels)
    for ids in make_buckets(lengths, modes, max_batch, max_pad_frac):
        batch = _pad_batch([mels[i] for i in ids], dev)
        idx = encoder._encode_native(batch, want_c=False, conv_mode=modes[ids[0]])[2]
        if clock: clock("encode")
        if slots > 0:
            for k, i in enumerate(ids):
                codes[i] = idx[k, : n_codes_all[i]]
            continue
        n_codes = [n_codes_all[i] for i in ids]
        spk = torch.tensor([int(speakers[i]) for i in ids], device=dev)
        wav = vocoder.generate(idx, spk, n_codes=n_codes, seed=seed, utt_ids=[utt_ids[i] for i in ids])
        if clock: clock("decode")
        for k, i in enumerate(ids):
            out[i] = wav[k, : 2 * up * n_codes[k]]
    if slots > 0:
        vocoder.set_option("slots", slots)
        try:
            for ids in decode_chunks(n_codes_all, mem_budget_bytes, up):
                idx = _pad_batch([codes[i] for i in ids], dev, torch.int64)
                spk = torch.tensor([int(speakers[i]) for i in ids], device=dev)
                wav = vocoder.generate(idx, spk, n_codes=[n_codes_all[i] for i in ids], seed=seed, utt_ids=[utt_ids[i] for i in ids])
                for k, i in enumerate(ids):
                    out[i] = wav[k, : 2 * up * n_codes_all[i]].clone() if len(ids) < len(mels) else wav[k, : 2 * up * n_codes_all[i]]
        finally:
            vocoder.set_option("slots", 0)
        if clock: clock("decode")
    return out


# device bytes a decode call needs per conditioning frame of an utterance's OWN (ragged rows: glue series 128 + hoisted gate
# inputs 768 + two prenet layers' outputs 2 x 256 + the Gcond row 3 x 896, fp32), and per code / output sample of the padded
# (B, T_max) grids that remain (int64 code indices, fp32 waveform)
BYTES_PER_OWN_FRAME = 4 * (128 + 768 + 256 + 256 + 3 * 896)
BYTES_PER_PADDED_FRAME = 4                  # half an int64 code index
BYTES_PER_PADDED_SAMPLE = 4


def decode_chunks(n_codes: Sequence[int], mem_budget_bytes: int, upsample: int = 160) -> List[List[int]]:
    """Utterance ids, in order, cut into decode calls whose device work space stays under ``mem_budget_bytes`` (at least one
    utterance per call).  Sizes for the reference's dimensions (``config.py:62-77``).

    Assumes: ``BYTES_PER_OWN_FRAME`` counts a glue width of 128, ``dim_voc_latent`` 256 and ``size_h_rnn`` 896 -- per frame
    ``4 * ((dz + ds) + 6 Hp + 2 * 2 Hp + 3 Hr)`` bytes in general, so a model with a wider prenet or GRU (up to 2.1x at
    256 / 1024 / 1024) needs a budget scaled by that ratio; only ``upsample`` is an argument.  The padded grids do not depend
    on the model's widths."""
    chunks, cur, own, tmax = [], [], 0, 0
    for i, nc in enumerate(n_codes):
        f = 2 * int(nc)
        t2 = max(tmax, f)
        need = (own + f) * BYTES_PER_OWN_FRAME + (len(cur) + 1) * t2 * (BYTES_PER_PADDED_FRAME + BYTES_PER_PADDED_SAMPLE * upsample)
        if cur and need > mem_budget_bytes:
            chunks.append(cur)
            cur, own, t2 = [], 0, f
        cur.append(i)
        own += f
        tmax = t2
    if cur:
        chunks.append(cur)
    return chunks


@torch.no_grad()
def front_end_utterances(waves, rates, device, sr: int = 16000, max_batch: int = 64, max_pad_frac: float = 0.25, conf=None,
                         clock=None):
    """``convert.py:54-70`` for a list of mono waveforms (numpy / CPU tensors at their files' own rates): resample to ``sr``
    (``librosa.load(sr=...)``), reference loudness (``convert.py:57``, before the peak normalisation), log-mel -- each ONE
    batched call per length bucket instead of three synchronising calls per utterance (the C ABI takes (B, Lmax) + lengths).
    Returns (list of (80, T_i) device mels, list of float reference LUFS).  ``clock(name)``: optional stage timer."""
    from . import loudness, preprocess
    n = len(waves)
    mels, ref = [None] * n, [None] * n
    meter = loudness.Meter(sr)
    lens_in = [int(len(w)) for w in waves]
    hop = (conf or preprocess.ConfPreprocessing()).hop_length
    for ids in make_buckets(lens_in, [int(r) for r in rates], max_batch, max_pad_frac):
        rate = int(rates[ids[0]])
        batch = _pad_batch([waves[i] for i in ids], device, non_blocking=True)    # each utterance straight into its padded row
        lens = [lens_in[i] for i in ids]
        if clock: clock("upload")
        if rate != sr:
            batch = preprocess.resample(batch, rate, sr, lengths=lens)
            lens = [-(-l * sr // rate) for l in lens]                       # ceil(l * sr / rate), as librosa.resample(fix=True)
            if clock: clock("resample")
        lufs = meter.integrated_loudness(batch, lengths=lens)
        if clock: clock("loudness_in")
        mel = preprocess.wave_to_mel(batch, conf, lengths=lens)
        lufs = lufs.tolist()
        for k, i in enumerate(ids):
            mels[i] = mel[k, :, : 1 + lens[k] // hop]
            ref[i] = lufs[k]
        if clock: clock("mel")
    return mels, ref


def score_groups(lengths_by_speaker, n_speakers: int, n_utterances: int, need_frames: int):
    """Batches of one scoring pass: ``n_speakers`` speakers x the first ``n_utterances`` utterances of each that hold at least
    ``need_frames`` mel frames.  -> (batches = lists of (speaker, [utterance ids]), speakers skipped for having too few
    long-enough utterances, speakers left over after the last whole batch).  Nothing is dropped without being named."""
    ready, skipped = [], []
    for spk, lengths in lengths_by_speaker.items():
        ids = [i for i, t in enumerate(lengths) if t >= need_frames][:n_utterances]
        (ready if len(ids) == n_utterances else skipped).append((spk, ids))
    whole = len(ready) - len(ready) % n_speakers
    batches = [ready[i:i + n_speakers] for i in range(0, whole, n_speakers)]
    return batches, [spk for spk, _ in skipped], [spk for spk, _ in ready[whole:]]


def cut_positions(seed: int, batch: int, lengths: Sequence[int], need_frames: int) -> List[int]:
    """Where each utterance of batch number ``batch`` is cut to ``need_frames`` frames: slot i starts at
    ``w mod (T_i - need_frames + 1)``, w = word ``i & 3`` of Philox4x32-10(counter = (i >> 2, 2 << 16, batch, 0), key = seed)
    -- the generator of the negative draws (``synth.cpc_negatives``: which = 0, 1), here with which = 2."""
    import numpy as np
    n = len(lengths)
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = np.arange(n) >> 2
    ctr[:, 1] = 2 << 16
    ctr[:, 2] = batch & 0xFFFFFFFF
    words = synth.philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return [int(words[i, i & 3]) % (int(t) - need_frames + 1) for i, t in enumerate(lengths)]


def _score_plan(cpc, mels_by_speaker, sample_frames: int, seed: int, dev):
    """The batching ``score_batches`` and ``fit_predictors`` share.  -> (n batches, skipped speakers, left-over speakers,
    ``mels(b)`` = the (Spk * Utt, 80, need) mel batch number ``b`` on ``dev``, cut by ``cut_positions`` with stream = b)."""
    need = sample_frames + cpc.conf.n_prediction_steps
    S, U = cpc.n_speakers_per_batch, cpc.n_utterances_per_speaker
    lengths = {spk: [int(m.shape[-1]) for m in mels] for spk, mels in mels_by_speaker.items()}
    batches, skipped, left = score_groups(lengths, S, U, need)

    def mels(b):
        picked = [mels_by_speaker[spk][i] for spk, ids in batches[b] for i in ids]
        starts = cut_positions(seed, b, [int(m.shape[-1]) for m in picked], need)
        return torch.stack([m[:, s:s + need] for m, s in zip(picked, starts)]).to(dev)

    return len(batches), skipped, left, mels


@torch.no_grad()
def score_batches(encoder: Encoder, cpc: CPCLoss, mels_by_speaker, sample_frames: int = 128, seed: int = 13, device=None):
    """One pass of ``train_cpc.py:104-131`` without the optimiser: checkpoint scoring.  ``mels_by_speaker``: speaker ->
    list of (80, T) mels.  Batches of ``cpc.n_speakers_per_batch`` speakers x ``cpc.n_utterances_per_speaker`` utterances,
    each cut to ``sample_frames + n_prediction_steps`` mel frames (``config.py:202``) at a position drawn by
    ``cut_positions`` (stream = batch number); ``encoder(mels)`` -> ``cpc(z, c, seed=seed, stream_id=batch)``.

    Returns the running means the reference logs (``train_cpc.py:128-131``) -- ``cpc_loss``, ``vq_loss``, ``perplexity``,
    ``accuracies`` (one per prediction step) -- with ``batches``, ``utterances`` and the speakers that could not be
    scored: ``speakers_skipped`` (fewer than Utt long-enough utterances) and ``speakers_left_over`` (after the last whole
    batch)."""
    S, U = cpc.n_speakers_per_batch, cpc.n_utterances_per_speaker
    dev = device if device is not None else next(encoder.parameters()).device
    n_batches, skipped, left, batch_mels = _score_plan(cpc, mels_by_speaker, sample_frames, seed, dev)
    res = {"cpc_loss": 0.0, "vq_loss": 0.0, "perplexity": 0.0, "accuracies": None, "batches": n_batches,
           "utterances": n_batches * S * U, "speakers_skipped": skipped, "speakers_left_over": left}
    for b in range(n_batches):
        z, c, vq_loss, perplexity = encoder(batch_mels(b))
        loss, acc = cpc(z, c, seed=seed, stream_id=b)
        if hasattr(encoder, "check"):
            encoder.check()                          # nothing incomplete may be reported
        n = b + 1                                    # running means as train_cpc.py:128-131 keeps them
        res["cpc_loss"] += (float(loss) - res["cpc_loss"]) / n
        res["vq_loss"] += (float(vq_loss) - res["vq_loss"]) / n
        res["perplexity"] += (float(perplexity) - res["perplexity"]) / n
        res["accuracies"] = list(acc) if res["accuracies"] is None else [a + (x - a) / n for a, x in zip(res["accuracies"], acc)]
    return res


def fit_predictors(encoder: Encoder, cpc: CPCLoss, mels_by_speaker, steps: int = 200, lr: float = 4e-4, optimizer=torch.optim.Adam,
                   sample_frames: int = 128, seed: int = 13, device=None, scheduler=None, opt_state: Optional[dict] = None):
    """Refit the K linear predictors of ``cpc`` on a FROZEN ``encoder`` -- what an adapted codebook needs before its CPC
    score means anything again (``adapt_codebook`` -> ``fit_predictors`` -> ``score_batches``).  Log-sum-exp of affine functions
    is convex in ``(W_k, b_k)``, so this is a convex fit.

    The batches, the cuts and ``stream_id`` = batch number are those of ``score_batches``; step i takes batch ``i mod batches``.
    The encoder runs under ``no_grad``, once per batch (it does not change; the encoded ``z``, ``c`` are kept on the device);
    ``cpc(z, c, seed=seed, stream_id=batch, differentiable=True)`` and ``backward()`` are one ``vqcpc_cpc_grad`` call asking
    for dW and db only; ``optimizer(params, lr=lr)`` -- torch's, as glue -- is given ``cpc.predictors[:K]`` alone, the K
    predictors the loss never reads stay as they are.  ``optimizer=optim.Adam`` (``vectorquantizedcpc_amd.optim``) makes the update
    one ``vqcpc_adam_step`` call as well.

    ``scheduler``: None (a constant ``lr``) or a factory called with the optimizer, e.g.
    ``lambda opt: optim.WarmupScheduler(opt, 150, 1e-5, 4e-4, [300, 400], 0.25)``; it is stepped when the batch index wraps (one
    epoch = one pass over the batches, ``train_cpc.py:136``).  ``opt_state``: None or a dict.  Its ``"optimizer"`` (and
    ``"scheduler"``) entries, where it has them, are loaded before step 0 -- the learning rate among them, which then wins over
    ``lr`` --, the step-to-batch map continues from ``opt_state.get("steps_done", 0)``, and after the last step the dict holds both
    state dicts and the new ``"steps_done"``: a fit of 2n steps equals two fits of n steps joined by one ``opt_state``, bit for bit.

    Returns ``losses`` and ``accuracies`` (per step; reading them synchronises once per step), ``steps``, ``batches``,
    ``utterances`` and the speakers ``score_batches`` would name: ``speakers_skipped``, ``speakers_left_over``."""
    return _fit(encoder, cpc, mels_by_speaker, steps, lr, optimizer, sample_frames, seed, device, _predictor_params(cpc),
                _encoded_step(cpc, seed, lambda z, c: c), scheduler=scheduler, opt_state=opt_state)


def _predictor_params(cpc):
    """The parameters of the K predictors the loss reads."""
    return [p for m in cpc.predictors[:cpc.n_prediction_steps] for p in m.parameters()]


def _encoded_step(cpc, seed, context):
    """The step of a fit on a frozen front end, for ``_fit``: ``context(z, c)`` -> the contexts the loss reads."""
    def step(b, batch):
        z, c = batch
        loss, acc = cpc(z, context(z, c), seed=seed, stream_id=b, differentiable=True)
        return loss, loss, acc, {}
    return step


def _fit(encoder, cpc, mels_by_speaker, steps, lr, optimizer, sample_frames, seed, device, params, step_of, frozen=(),
         encode_once=True, extras=(), scheduler=None, opt_state=None):
    """The loop the three fits share: the batches of ``_score_plan``, step i on batch ``i mod batches``; per step
    ``step_of(b, batch)`` -> (the loss to back-propagate, the CPC loss, the accuracies, dict of the ``extras``), ``backward()`` and
    one step of ``optimizer(params, lr=lr)``.  ``encode_once``: ``batch`` is ``(z, c)`` of ``encoder(mels)``, computed under
    ``no_grad`` at the batch's first turn, checked and kept on the device; otherwise it is the mels, nothing is encoded ahead and
    ``encoder.check()`` follows ``backward()``.  ``frozen``: parameters that require no gradient while the loop runs.  ``extras``:
    the names of further per-step lists in the result.  ``scheduler``, ``opt_state``: ``fit_predictors`` describes them."""
    S, U = cpc.n_speakers_per_batch, cpc.n_utterances_per_speaker
    dev = device if device is not None else next(encoder.parameters()).device
    n_batches, skipped, left, batch_mels = _score_plan(cpc, mels_by_speaker, sample_frames, seed, dev)
    res = {"losses": [], **{k: [] for k in extras}, "accuracies": [], "steps": 0, "batches": n_batches,
           "utterances": n_batches * S * U, "speakers_skipped": skipped, "speakers_left_over": left}
    if n_batches == 0 or steps <= 0:
        return res
    opt = optimizer(params, lr=lr)
    sched, done = _resume(opt, scheduler, opt_state)
    for p in frozen:                                     # a part that does not step costs no backward either
        p.requires_grad_(False)
    encoded = {}
    try:
        for step in range(steps):
            b = (done + step) % n_batches
            if not encode_once:
                batch = batch_mels(b)
            elif b in encoded:
                batch = encoded[b]
            else:
                with torch.no_grad():
                    z, c, _, _ = encoder(batch_mels(b))
                    if hasattr(encoder, "check"):
                        encoder.check()
                batch = encoded[b] = (z.detach(), c.detach())
            opt.zero_grad(set_to_none=True)
            with torch.enable_grad():
                loss, cpc_loss, acc, extra = step_of(b, batch)
                loss.backward()
            if not encode_once and hasattr(encoder, "check"):
                encoder.check()
            opt.step()
            if sched is not None and b == n_batches - 1:         # the batch index wraps: an epoch is over
                sched.step()
            if opt_state is not None:
                opt_state["steps_done"] = done + step + 1
            res["losses"].append(float(cpc_loss.detach()))
            for k in extras:
                res[k].append(float(extra[k]))
            res["accuracies"].append(list(acc))
            res["steps"] = step + 1
    finally:
        for p in frozen:
            p.requires_grad_(True)
    _keep(opt, sched, opt_state)
    return res


def _resume(opt, scheduler, opt_state):
    """What a fit does with its optimizer before step 0: ``scheduler(opt)`` (None stays None), then the ``"optimizer"`` and
    ``"scheduler"`` entries of ``opt_state`` loaded where it has them.  -> (the scheduler, the steps done before this fit)."""
    sched = scheduler(opt) if scheduler is not None else None
    if not opt_state:
        return sched, 0
    if opt_state.get("optimizer") is not None:
        opt.load_state_dict(opt_state["optimizer"])
    if sched is not None and opt_state.get("scheduler") is not None:
        sched.load_state_dict(opt_state["scheduler"])
    return sched, int(opt_state.get("steps_done", 0))


def _keep(opt, sched, opt_state):
    """After the last step: both state dicts into ``opt_state``, in place (``"steps_done"`` is the loop's)."""
    if opt_state is not None:
        opt_state["optimizer"] = opt.state_dict()
        opt_state["scheduler"] = sched.state_dict() if sched is not None else None


def fit_context(encoder: Encoder, cpc: CPCLoss, mels_by_speaker, steps: int = 200, lr: float = 4e-4, optimizer=torch.optim.Adam,
                sample_frames: int = 128, seed: int = 13, device=None, train_predictors: bool = True, scheduler=None,
                opt_state: Optional[dict] = None):
    """Refit the context LSTM ``encoder.rnn`` -- and, with ``train_predictors``, the K predictors of ``cpc`` with it, under one
    optimizer as ``train_cpc.py:53-55`` has them -- on a frozen front end and codebook: after the codebook moves the LSTM sees units
    it was never trained on (``adapt_codebook`` -> ``fit_context`` -> ``score_batches``).

    The batches, the cuts and ``stream_id`` = batch number are those of ``score_batches`` and ``fit_predictors``.  The front end
    and the VQ run under ``no_grad``, once per batch (they do not change; ``z`` is kept on the device).  Every step runs
    ``c = encoder.context(z, differentiable=True)``, ``cpc(z, c, seed=seed, stream_id=batch, differentiable=True)`` and
    ``backward()`` -- one ``vqcpc_cpc_grad`` call for dc (and dW, db), one ``vqcpc_encoder_context_bwd`` call for the LSTM's
    gradients, dz not asked for -- then one step of ``optimizer(params, lr=lr)`` over ``encoder.rnn.parameters()`` (+
    ``cpc.predictors[:K]``).  The native handles are not rebuilt between steps; the next ``encode`` / ``forward`` rebuilds the
    encoder's once.

    ``scheduler``, ``opt_state``: as for ``fit_predictors``.  Returns what ``fit_predictors`` returns."""
    params = list(encoder.rnn.parameters()) + (_predictor_params(cpc) if train_predictors else [])
    return _fit(encoder, cpc, mels_by_speaker, steps, lr, optimizer, sample_frames, seed, device, params,
                _encoded_step(cpc, seed, lambda z, c: encoder.context(z, differentiable=True)), scheduler=scheduler, opt_state=opt_state)


FIT_ENCODER_PARTS = ("front", "rnn", "predictors")


def fit_encoder(encoder: Encoder, cpc: CPCLoss, mels_by_speaker, steps: int = 200, lr: float = 4e-4, optimizer=torch.optim.Adam,
                sample_frames: int = 128, seed: int = 13, device=None, adapt_codebook: bool = True, train=FIT_ENCODER_PARTS,
                scheduler=None, opt_state: Optional[dict] = None):
    """Refit the whole encoder -- the training step of ``train_cpc.py:116-124`` -- after the codebook moved
    (``adapt_codebook`` -> ``fit_encoder`` -> ``score_batches``): the Conv1d / LayerNorm / Linear front end that produces the units
    follows the codebook, which ``fit_context`` and ``fit_predictors`` cannot make it do.

    ``train``: which parts step, any of ``"front"`` (``encoder.conv`` and ``encoder.encoder``), ``"rnn"`` (``encoder.rnn``) and
    ``"predictors"`` (``cpc.predictors[:K]``), under ONE ``optimizer(params, lr=lr)`` as ``train_cpc.py:53-55`` has them -- torch's,
    as glue; the parameters of a part that is not named are left alone and receive no gradient.  ``adapt_codebook``: run the EMA
    update of ``model.py:136-145`` in every step, as the reference's training branch does; False keeps the codebook frozen.

    The batches, the cuts and ``stream_id`` = batch number are those of ``score_batches``; step i takes batch ``i mod batches``.
    Nothing is encoded ahead, because the front end moves.  Every step is ``encoder.forward_differentiable(mels)`` ->
    ``cpc(z, c, seed=seed, stream_id=batch, differentiable=True)`` -> ``loss = cpc_loss + vq_loss`` -> ``backward()``: one
    ``vqcpc_cpc_grad``, one ``vqcpc_encoder_context_bwd``, one ``vqcpc_encoder_vq_bwd`` and one ``vqcpc_encoder_front_bwd`` call,
    each asking only for what is needed -- then ``opt.step()``.  The native handles are not rebuilt between steps.

    ``scheduler``, ``opt_state``: as for ``fit_predictors``.  Returns what ``fit_context`` returns (``losses`` = the CPC loss per step), plus per-step ``vq_losses`` and ``perplexities``."""
    train = tuple(train)
    unknown = [t for t in train if t not in FIT_ENCODER_PARTS]
    if unknown or not train or len(set(train)) != len(train):
        raise ValueError(f"fit_encoder: train must name each of {FIT_ENCODER_PARTS} at most once and at least one of them, got {train!r}")
    parts = {"front": list(encoder.conv.parameters()) + list(encoder.encoder.parameters()), "rnn": list(encoder.rnn.parameters()),
             "predictors": _predictor_params(cpc)}
    params = [p for name in FIT_ENCODER_PARTS if name in train for p in parts[name]]
    frozen = [p for name in FIT_ENCODER_PARTS if name not in train for p in parts[name] if p.requires_grad]

    def step(b, mels):
        z, c, vq_loss, perplexity = encoder.forward_differentiable(mels, adapt_codebook=adapt_codebook)
        cpc_loss, acc = cpc(z, c, seed=seed, stream_id=b, differentiable=True)
        return cpc_loss + vq_loss, cpc_loss, acc, {"vq_losses": vq_loss.detach(), "perplexities": perplexity}

    return _fit(encoder, cpc, mels_by_speaker, steps, lr, optimizer, sample_frames, seed, device, params, step, frozen=frozen,
                encode_once=False, extras=("vq_losses", "perplexities"), scheduler=scheduler, opt_state=opt_state)


# ---------------------------------------------------------------------------------------- vocoder scoring
def mulaw_classes(wave, bits: int = 8):
    """Mu-law classes of a 16 kHz waveform as the reference makes its vocoder targets (``preprocess.py:20-27, :90-91``): peak
    normalisation to 0.999, then ``preprocess.mulaw_encode`` -- the host formula itself (numpy, elementwise, not a hot path)."""
    import numpy as np
    from . import preprocess
    w = np.asarray(torch.as_tensor(wave).detach().cpu().numpy() if isinstance(wave, torch.Tensor) else wave)
    return preprocess.mulaw_encode(w / np.abs(w).max() * 0.999, 2 ** bits).astype(np.int64)


def scored_samples(n_audio: int, n_codes: int, upsample: int = 160) -> int:
    """Samples of an utterance that a scoring call takes: ``min(len, 2 * upsample * n_codes + 1)`` -- the encoder halves the frame
    rate, so the codes may cover a few hundred samples fewer than the file holds; one sample more than they cover is kept, as
    the last target."""
    return min(int(n_audio), 2 * upsample * int(n_codes) + 1)


@torch.no_grad()
def _vocoder_utterances(encoder, vocoder, waves_or_mels, audio, speakers, max_batch, max_pad_frac, conf, who):
    """What ``score_vocoder`` and ``fit_vocoder`` make of their utterances before the vocoder runs: waveforms -> mels (batched HIP
    front end), mels -> ``encode_utterances`` -> code indices, the mu-law classes (``mulaw_classes`` of the waveforms where
    ``audio`` is None) and the samples of each that a scoring call takes.  -> ``(codes, n_codes, audio, keep)``."""
    from . import preprocess
    dev = next(encoder.parameters()).device
    up = vocoder.conf.rnnms.upsampling_t
    n = len(waves_or_mels)
    if len(speakers) != n or (audio is not None and len(audio) != n):
        raise ValueError(f"{who}: one speaker (and one audio array) per utterance")
    mels = list(waves_or_mels)
    is_wave = [torch.as_tensor(m).dim() == 1 for m in mels]
    if audio is None:
        if not all(is_wave):
            raise ValueError(f"{who}: audio=None needs waveforms (the classes are made from them)")
        audio = [mulaw_classes(w, vocoder.conf.rnnms.bits_mu_law) for w in mels]
    wave_ids = [i for i in range(n) if is_wave[i]]
    if wave_ids:
        lens = [int(len(mels[i])) for i in wave_ids]
        hop = (conf or preprocess.ConfPreprocessing()).hop_length
        for ids in make_buckets(lens, [0] * len(lens), max_batch, max_pad_frac):
            batch = _pad_batch([mels[wave_ids[k]] for k in ids], dev)
            mel = preprocess.wave_to_mel(batch, conf, lengths=[lens[k] for k in ids])
            for r, k in enumerate(ids):
                mels[wave_ids[k]] = mel[r, :, : 1 + lens[k] // hop]
    codes = encode_utterances(encoder, mels, max_batch=max_batch, max_pad_frac=max_pad_frac)
    n_codes = [int(c["indices"].numel()) for c in codes]
    audio = [torch.as_tensor(a).to(torch.int64).reshape(-1) for a in audio]
    keep = [scored_samples(a.numel(), nc, up) for a, nc in zip(audio, n_codes)]
    return codes, n_codes, audio, keep


@torch.no_grad()
def score_vocoder(encoder: Encoder, vocoder: Vocoder, waves_or_mels, audio, speakers: Sequence[int], max_batch: int = 64,
                  max_pad_frac: float = 0.25, conf=None):
    """Teacher-forced score of a vocoder checkpoint on held-out utterances -- the validation number the reference does not
    compute (its ``validation_step`` returns 0 because whole utterances do not batch there, ``vocoder.py:68-94``).

    ``waves_or_mels``: per utterance a 1-D waveform at the front end's rate (16 kHz: after any resampling, before pre-emphasis)
    or a (n_mels, T) log-mel.  ``audio``: per utterance the int mu-law classes to score, or None with waveforms: then they are
    ``mulaw_classes`` of the same waveform.  mel -> ``Encoder.encode`` -> code indices -> length buckets -> ``Vocoder.nll`` with
    ``n_codes`` / ``lengths`` per bucket.  Returns ``(records, totals)``: one dict per utterance (``nll_sum``, ``n_scored``,
    ``n_correct``, ``n_codes``, ``indices`` = the code indices it was conditioned on, ``n_cut`` = samples of the utterance that
    the codes do not cover and that were cut) and the
    corpus totals (``loss`` in nats per sample, ``bits_per_sample``, ``accuracy``, ``n_scored``, ``n_correct``, ``nll_sum``,
    ``n_cut``, ``n_utterances``)."""
    import math
    dev = next(encoder.parameters()).device
    n = len(waves_or_mels)
    codes, n_codes, audio, keep = _vocoder_utterances(encoder, vocoder, waves_or_mels, audio, speakers, max_batch, max_pad_frac, conf,
                                                      "score_vocoder")
    records: List[Optional[dict]] = [None] * n
    for ids in make_buckets(keep, [0] * n, max_batch, max_pad_frac):
        z = _pad_batch([codes[i]["indices"] for i in ids], dev, torch.int64, min_len=1)
        a = _pad_batch([audio[i][: keep[i]] for i in ids], "cpu", torch.int64, min_len=1)       # one upload for the batch
        spk = torch.tensor([int(speakers[i]) for i in ids], device=dev)
        res = vocoder.nll(a.to(dev), z, spk, lengths=[keep[i] for i in ids], n_codes=[n_codes[i] for i in ids])
        sums, cnt, ok = res.nll_sum.tolist(), res.n_scored.tolist(), res.n_correct.tolist()
        for r, i in enumerate(ids):
            records[i] = {"nll_sum": sums[r], "n_scored": cnt[r], "n_correct": ok[r], "n_codes": n_codes[i],
                          "n_cut": int(audio[i].numel()) - keep[i], "indices": codes[i]["indices"]}
    tot = {k: sum(r[k] for r in records) for k in ("nll_sum", "n_scored", "n_correct", "n_cut")}
    tot["n_utterances"] = n
    tot["loss"] = tot["nll_sum"] / tot["n_scored"] if tot["n_scored"] else float("nan")
    tot["bits_per_sample"] = tot["loss"] / math.log(2.0)
    tot["accuracy"] = tot["n_correct"] / tot["n_scored"] if tot["n_scored"] else float("nan")
    return records, tot


def training_cuts(indices, audio, n_codes, keep, upsample: int, clip_codes: Optional[int], seed: int):
    """The cuts ``fit_vocoder`` trains on: per utterance its code indices and the ``keep`` classes they cover; with ``clip_codes``,
    an utterance with more codes keeps a cut of that many from a start drawn from ``torch.Generator().manual_seed(seed)`` (one draw
    per such utterance, in order) and the ``2 * upsample * clip_codes + 1`` samples under it.  -> ``(indices, audio, n_codes, keep)``
    as new lists.  Pure host code: the float64 reference of the tests cuts with it as well."""
    indices, audio = list(indices), [a[:k] for a, k in zip(audio, keep)]
    n_codes, keep = list(n_codes), list(keep)
    if clip_codes is not None:
        if clip_codes < 1:
            raise ValueError(f"fit_vocoder: clip_codes must be at least 1 or None, got {clip_codes}")
        gen = torch.Generator().manual_seed(int(seed))
        for i, nc in enumerate(n_codes):
            if nc > clip_codes:
                start = int(torch.randint(0, nc - clip_codes + 1, (1,), generator=gen))
                indices[i] = indices[i][start:start + clip_codes]
                audio[i] = audio[i][2 * upsample * start: 2 * upsample * (start + clip_codes) + 1]
                n_codes[i], keep[i] = clip_codes, int(audio[i].numel())
    return indices, audio, n_codes, keep


def fit_vocoder(encoder: Encoder, vocoder: Vocoder, waves_or_mels, audio, speakers: Sequence[int], steps: int = 200, lr: float = 4e-4,
                optimizer=torch.optim.Adam, max_batch: int = 32, max_pad_frac: float = 0.25, clip_codes: Optional[int] = 16, seed: int = 13,
                conf=None, train=("ar",), scheduler=None, opt_state: Optional[dict] = None):
    """Refit the vocoder on the units a frozen encoder produces -- the vocoder objective of ``vocoder.py:62-63`` -- after
    ``adapt_codebook`` or ``fit_encoder`` moved those units, or for new speakers and recording conditions (``score_vocoder`` ->
    ``fit_vocoder`` -> ``score_vocoder``).

    ``train``: which parts step, any of ``"ar"`` (the sample-rate network ``vocoder.rnnms.ar``: embedding, GRU, fc1, fc2),
    ``"prenet"`` (``vocoder.rnnms.prenet``) and ``"embeddings"`` (``code_embedding`` -- the table the moved code indices index --
    and ``speaker_embedding``), under ONE ``optimizer(params, lr=lr)`` as the reference's trainer has them; the parameters of a part
    that is not named are left alone and receive no gradient.  The default refits the sample-rate network around a frozen
    conditioning path.

    The utterances, their codes and classes are prepared exactly as ``score_vocoder`` prepares them (the same function), once,
    under ``no_grad``.  ``clip_codes``: every utterance with more codes keeps a seeded cut of that many codes and the
    ``2 * upsampling_t * clip_codes + 1`` samples they cover -- 16 gives the reference's (., 5120) training shape; None: whole
    utterances.  The reference clips the MEL before it encodes; this cuts the CODES after the whole utterance was encoded, so the
    units at the edges of a cut have seen their context.  The buckets are ``score_vocoder``'s (``make_buckets``); step i takes bucket
    ``i mod n``.  Every step is ``vocoder.nll(..., differentiable=True, train=train).loss.backward()`` -- one
    ``vqcpc_vocoder_ar_fwd`` and one ``vqcpc_vocoder_ar_bwd`` call; with a conditioning part named, ``vqcpc_vocoder_cond_fwd``,
    ``vqcpc_vocoder_ar_fwd_cond``, ``vqcpc_vocoder_ar_bwd_cond`` and ``vqcpc_vocoder_cond_bwd`` -- then one step of
    ``optimizer(params, lr=lr)`` (torch's, as glue).  The native handle is not rebuilt between steps; it is refreshed once at the
    end, so that ``generate`` and ``nll`` see the new weights.

    ``scheduler``: None or a factory called with the optimizer; it is stepped after EVERY step, as the reference's trainer steps its
    ``MultiStepLR`` (``vocoder.py:102-105``).  ``opt_state``: as for ``fit_predictors`` (step i takes bucket
    ``(steps_done + i) mod n``).

    Returns ``losses`` (per step, before that step's update), ``steps``, ``batches`` and ``utterances`` (those with at least one
    sample to score)."""
    train = vocoder._train_parts(train, "fit_vocoder")
    dev = next(encoder.parameters()).device
    up = vocoder.conf.rnnms.upsampling_t
    codes, n_codes, audio, keep = _vocoder_utterances(encoder, vocoder, waves_or_mels, audio, speakers, max_batch, max_pad_frac, conf,
                                                      "fit_vocoder")
    idx, audio, n_codes, keep = training_cuts([c["indices"] for c in codes], audio, n_codes, keep, up, clip_codes, seed)
    live = [i for i in range(len(idx)) if keep[i] >= 2]
    batches = []
    for ids in make_buckets([keep[i] for i in live], [0] * len(live), max_batch, max_pad_frac):
        ids = [live[k] for k in ids]
        batches.append((_pad_batch([audio[i] for i in ids], "cpu", torch.int64, min_len=1).to(dev),
                        _pad_batch([idx[i] for i in ids], dev, torch.int64, min_len=1),
                        torch.tensor([int(speakers[i]) for i in ids], device=dev), [keep[i] for i in ids], [n_codes[i] for i in ids]))
    res = {"losses": [], "steps": 0, "batches": len(batches), "utterances": len(live)}
    if not batches or steps <= 0:
        return res
    params = [p for part in vocoder.TRAIN_PARTS if part in train for p in vocoder._part_params(part)]
    if not any(p.requires_grad for p in params):
        raise ValueError("fit_vocoder: no parameter of " + (" / ".join(train) if train != ("ar",) else "vocoder.rnnms.ar") + " requires a gradient")
    opt = optimizer(params, lr=lr)
    sched, done = _resume(opt, scheduler, opt_state)
    for step in range(steps):
        a, z, spk, lengths, ncs = batches[(done + step) % len(batches)]
        opt.zero_grad(set_to_none=True)
        with torch.enable_grad():
            loss = vocoder.nll(a, z, spk, lengths=lengths, n_codes=ncs, differentiable=True, train=train).loss
            loss.backward()
        opt.step()
        if sched is not None:
            sched.step()
        if opt_state is not None:
            opt_state["steps_done"] = done + step + 1
        res["losses"].append(float(loss.detach()))
        res["steps"] = step + 1
    _keep(opt, sched, opt_state)
    vocoder.refresh()
    return res


# ---------------------------------------------------------------------------------------- ABX scoring
@torch.no_grad()
def score_abx(encoder: Encoder, mels_by_file, items, feature: str = "z", mode: str = "within", frame_shift: float = None,
              frame_offset: float = None, max_batch: int = 64, max_pad_frac: float = 0.25, mem_budget_bytes: int = 1 << 30,
              metric: str = "angular"):
    """encode -> ABX in one process, without the text files of ``encode.py:48-52`` and the outside script of the reference's
    README 4-B (own protocol: ``abx.py``).  ``mels_by_file``: file name (as the items file names it) -> (80, T)
    mel; ``items``: a path or a list of ``abx.Item``; ``feature``: "z" (the quantised units), "c" (the context) or "indices"
    (the units as codebook indices: ``abx.score_indices`` with the encoder's codebook -- with ``metric="angular"`` the counts of
    "z", from 4 bytes per frame and one table; ``metric="edit"``: the edit distance between index runs, "indices" only).  The
    utterances go through ``encode_utterances`` and ``encoder.check()`` before anything is scored.  Returns ``abx.score``'s
    dict."""
    from . import abx
    if feature not in ("z", "c", "indices"):
        raise ValueError(f"score_abx: feature must be 'z', 'c' or 'indices', got {feature!r}")
    if metric not in abx.METRICS:
        raise ValueError(f"score_abx: metric must be one of {sorted(abx.METRICS)}, got {metric!r}")
    if metric != "angular" and feature != "indices":
        raise ValueError(f"score_abx: metric {metric!r} is defined on feature 'indices', not on {feature!r}")
    files = sorted(mels_by_file)
    enc = encode_utterances(encoder, [mels_by_file[f] for f in files], want_context=feature == "c", max_batch=max_batch,
                            max_pad_frac=max_pad_frac)
    if hasattr(encoder, "check"):
        encoder.check()                              # nothing incomplete may be scored
    feats = {f: r[feature] for f, r in zip(files, enc)}
    kw = dict(mode=mode, frame_shift=abx.FRAME_SHIFT if frame_shift is None else frame_shift,
              frame_offset=abx.FRAME_OFFSET if frame_offset is None else frame_offset, mem_budget_bytes=mem_budget_bytes)
    if feature == "indices":
        return abx.score_indices(encoder.codebook.embedding, feats, items, metric=metric, **kw)
    return abx.score(feats, items, **kw)
