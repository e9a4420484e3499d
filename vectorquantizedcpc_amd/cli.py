"""Command-line equivalents of the reference's ``encode.py`` and ``convert.py`` on MI355X.

    python -m vectorquantizedcpc_amd.cli encode  --dataset datasets/2019/english --out-dir out/z
                                                 [--cpc-checkpoint ckpt.pt | --random-init] [--save-auxiliary]
    python -m vectorquantizedcpc_amd.cli convert --dataset datasets/2019/english --synthesis-list list.json
                                                 --in-dir mels/ --out-dir out/wav
                                                 [--cpc-checkpoint .. --vocoder-checkpoint .. | --random-init] [--seed 13]

    python -m vectorquantizedcpc_amd.cli score   --dataset datasets/2019/english --cpc-checkpoint ckpt.pt | --random-init
                                                 [--speakers 8 --utterances 8 --negatives 17 --sample-frames 128 --seed 13]

    python -m vectorquantizedcpc_amd.cli score-vocoder --dataset datasets/2019/english --in-dir wavs/
                                                 [--cpc-checkpoint .. --vocoder-checkpoint .. | --random-init] [--per-utterance]
    python -m vectorquantizedcpc_amd.cli fit-vocoder   --dataset datasets/2019/english --in-dir wavs/ --out vocoder.pt
                                                 [--cpc-checkpoint .. --vocoder-checkpoint .. | --random-init]
                                                 [--steps 200 --lr 4e-4 --clip-codes 16 --seed 13]

    python -m vectorquantizedcpc_amd.cli abx     --items FILE --mode within|across [--frame-shift 0.02 --frame-offset 0.01]
                                                 --features DIR | --dataset datasets/2019/english
                                                                  [--cpc-checkpoint ckpt.pt | --random-init]
                                                                  [--feature z|c|indices] [--metric angular|edit]

    python -m vectorquantizedcpc_amd.cli adapt-codebook --dataset datasets/2019/english --cpc-checkpoint in.pt | --random-init
                                                 --out-checkpoint out.pt [--epochs 1]

    python -m vectorquantizedcpc_amd.cli fit-predictors --dataset datasets/2019/english --cpc-checkpoint in.pt | --random-init
                                                 --out-checkpoint out.pt [--steps 200 --lr 4e-4] [the options of score]

    python -m vectorquantizedcpc_amd.cli fit-context --dataset datasets/2019/english --cpc-checkpoint in.pt | --random-init
                                                 --out-checkpoint out.pt [--steps 200 --lr 4e-4] [--freeze-predictors]
                                                 [the options of score]

    python -m vectorquantizedcpc_amd.cli fit-encoder --dataset datasets/2019/english --cpc-checkpoint in.pt | --random-init
                                                 --out-checkpoint out.pt [--steps 200 --lr 4e-4] [--train front,rnn,predictors]
                                                 [--freeze-codebook] [the options of score]

``fit-encoder`` runs the reference's whole training step (``train_cpc.py:116-124``, ``driver.fit_encoder``): the front end, the
context LSTM and the K predictors under one Adam, ``loss = cpc_loss + vq_loss``, the codebook following by its EMA update unless
``--freeze-codebook`` -- every gradient from the loss down to ``conv.weight`` is a HIP call (``vqcpc_cpc_grad``,
``vqcpc_encoder_context_bwd``, ``vqcpc_encoder_vq_bwd``, ``vqcpc_encoder_front_bwd``).  It prints the ``score`` lines before and
after and writes a checkpoint with ``"encoder"`` and ``"cpc"`` replaced.
``fit-context`` refits the context LSTM ``encoder.rnn`` together with the K predictors (``driver.fit_context``: back-propagation
through time is ``vqcpc_encoder_context_bwd``'s, the optimizer torch's Adam over both, as ``train_cpc.py:53-55`` has them) on the
frozen front end and codebook -- the step after ``adapt-codebook``.  It prints the ``score`` lines before and after and writes a
checkpoint in which only ``encoder.rnn.*`` and the K predictors in use differ.
``fit-predictors`` refits the K linear predictors of a checkpoint's ``"cpc"`` entry on its frozen encoder
(``driver.fit_predictors``: the gradient is ``vqcpc_cpc_grad``'s, the optimizer torch's Adam) -- what an adapted codebook needs
before ``score`` means anything again.  It prints the ``score`` lines before and after the fit and writes a checkpoint with
``"encoder"`` untouched and ``"cpc"`` replaced.
``adapt-codebook`` fits a checkpoint's codebook to the mels of ``test.json`` with the EMA update of ``model.py:136-145`` (no
gradient: ``driver.adapt_codebook``), prints loss, perplexity and codes in use per epoch and writes a checkpoint whose
``"encoder"`` entry has the reference's keys: ``encode``, ``abx`` and ``score`` run on it as on any other.
``abx`` stands in for the outside "ABX evaluation script" of the reference's README 4-B (own protocol, ``abx.py``): the ABX
error rate of the units on an items file (``file onset offset phone prev next speaker`` per line), from the ``.txt`` frames
``encode`` wrote (``--features``) or straight from the mels of ``test.json`` (``--dataset``, ``driver.score_abx``);
``--feature indices`` scores the units as codebook indices (the numbers of ``z`` from a distance table, or ``--metric edit``:
the edit distance between index runs).
``fit-vocoder`` refits the vocoder's sample-rate network ``rnnms.ar`` (embedding, GRU, fc1, fc2) on the same utterances, conditioned
on the units of the (frozen) encoder -- the step after ``adapt-codebook`` / ``fit-encoder``, or for a new speaker
(``driver.fit_vocoder``: forward and back-propagation through time are ``vqcpc_vocoder_ar_fwd`` / ``_bwd``, the optimizer torch's
Adam).  ``--train ar,prenet,embeddings`` names the parts that step: by default the prenet and the two embedding tables stay
frozen; with them named the whole ``loss.backward()`` runs in HIP down to ``code_embedding.weight`` (``vqcpc_vocoder_cond_fwd`` /
``_bwd``) -- after the codebook moved, ``code_embedding`` is the table the moved indices index.  It prints the ``score-vocoder`` line before and after and writes
``{"vocoder": state_dict}``.
The four ``fit-*`` commands share the optimizer options: ``--optimizer hip`` makes the update ``vqcpc_adam_step`` (``optim.Adam``;
the default stays torch's Adam), ``--warmup E --initial-lr A --milestones M1,M2 --gamma G`` schedules the learning rate as the
reference's ``scheduler.py`` does, from ``A`` to ``--lr`` over ``E`` epochs and times ``G`` at every milestone (``--milestones``
alone: torch's ``MultiStepLR``; an epoch is one pass over the batches, for ``fit-vocoder`` one step, ``vocoder.py:102-105``), and
``--optimizer-state PATH`` reads ``{"optimizer", "scheduler", "steps_done"}`` from the file if it exists and writes it at the end,
so that a later run goes on where this one stopped.
``score-vocoder`` is the validation number the reference's vocoder training never computes (``vocoder.py:68-94``): the
teacher-forced cross-entropy of ``vocoder.py:62-63`` on ``<in_dir>/<utterance>.wav`` of every entry of ``test.json``, speaker id
from ``speakers.json`` by the file name's prefix: loss in nats per sample, bits per sample and top-1 accuracy
(``driver.score_vocoder``, one fused HIP head per chunk of the scan).
``score`` is one pass of ``train_cpc.py:104-148`` without the optimiser: the CPC loss, VQ loss, perplexity and per-step
prediction accuracies of a checkpoint (its ``"encoder"`` and ``"cpc"`` entries) on the utterances of ``test.json``, grouped by
the speaker their file name starts with (``<speaker>_<utterance>``).
``encode`` mirrors ``encode.py:14-67``.  ``convert`` mirrors ``convert.py:17-83`` from the mel onwards: inputs are
``<in_dir>/<utterance>.mel.npy`` or, if absent, ``<utterance>.wav`` (16 kHz) run through the HIP mel
front-end (``preprocess.wave_to_mel`` = ``convert.py:54-70``).  For ``.wav`` inputs the output is re-normalised
to the input's integrated loudness (``convert.py:57,79-80``) by the HIP meter in ``loudness.py``; a ``.mel.npy``
input carries no reference loudness and its output is written as generated.  Utterances are batched by the
length-bucketed drivers; every output equals the batch-1 result.
"""
import argparse
import functools
import sys
from pathlib import Path

import torch

from . import ConfCPC, ConfEncoder, ConfVocoder, CPCLoss, Encoder, Vocoder, _lib, driver, io, loudness, synth


def _models(args, need_vocoder):
    dev = torch.device(args.device)
    enc = Encoder(ConfEncoder(80, 512, 512, 64, 256))
    enc.load_state_dict(synth.encoder_state_dict() if args.random_init else io.load_encoder_checkpoint(args.cpc_checkpoint))
    enc = enc.to(dev).eval()
    voc = None
    if need_vocoder:
        voc = Vocoder(ConfVocoder())
        voc.load_state_dict(synth.vocoder_state_dict() if args.random_init else
                            io.load_vocoder_checkpoint(args.vocoder_checkpoint, expected=voc.state_dict()))
        voc = voc.to(dev).eval()
    return enc, voc


def encode_dataset(args) -> int:
    paths = io.read_test_metadata(args.dataset)
    out_dir = Path(args.out_dir)
    out_dir.mkdir(exist_ok=True, parents=True)
    enc, _ = _models(args, need_vocoder=False)
    aux = []
    if args.save_auxiliary:                                    # encode.py:34-40
        enc.encoder[-1].register_forward_hook(lambda m, i, o: aux.append(o.clone()))
    mels = [io.load_mel(p) for p in paths]
    if args.save_auxiliary:
        # the hook delivers one batch at a time: keep the reference's one-utterance-per-call order
        for p, mel in zip(paths, mels):
            def run():
                aux.clear()                                    # a repeat leaves one captured batch, as a single call does
                return enc.encode(mel[None].to(args.device))

            z, c, _ = _lib.run_checked(run, enc.check, "encode repeated on the fallback path: {}")   # nothing incomplete is written
            io.save_frames_text(out_dir / p.stem, z[0])
            for name, t in (("auxiliary_embedding1", c[0]), ("auxiliary_embedding2", aux.pop()[0])):
                d = out_dir.parent / name
                d.mkdir(exist_ok=True, parents=True)
                io.save_frames_text(d / p.stem, t)
    else:
        for p, r in zip(paths, driver.encode_utterances(enc, mels, max_batch=args.max_batch)):
            io.save_frames_text(out_dir / p.stem, r["z"])
    print(f"encoded {len(paths)} utterances -> {out_dir}")
    return 0


def _score_setup(args):
    """Encoder, CPCLoss and the mels of ``test.json`` by speaker, for ``score`` and ``fit-predictors``."""
    paths = io.read_test_metadata(args.dataset)
    enc, _ = _models(args, need_vocoder=False)
    cpc = CPCLoss(ConfCPC(args.prediction_steps, args.speakers, args.utterances, args.negatives, 64, 256))
    cpc.load_state_dict(synth.cpc_state_dict(n_prediction_steps=args.prediction_steps) if args.random_init
                        else io.load_cpc_checkpoint(args.cpc_checkpoint))
    cpc = cpc.to(torch.device(args.device)).eval()
    by_speaker = {}
    for p in paths:
        by_speaker.setdefault(p.stem.split("_")[0], []).append(io.load_mel(p))
    return enc, cpc, by_speaker


def _print_score(args, enc, cpc, by_speaker) -> int:
    r = driver.score_batches(enc, cpc, by_speaker, sample_frames=args.sample_frames, seed=args.seed)
    if r["batches"] == 0:
        print(f"no batch of {args.speakers} speakers x {args.utterances} utterances could be formed; skipped speakers: "
              f"{r['speakers_skipped']}, left over: {r['speakers_left_over']}")
        return 1
    # train_cpc.py:146-148
    print(f"cpc loss:{r['cpc_loss']:.2E}, vq loss:{r['vq_loss']:.2E}, perpexlity:{r['perplexity']:.3f}")
    print([f"{a:.3f}" for a in r["accuracies"]])
    print(f"scored {r['utterances']} utterances in {r['batches']} batches; speakers skipped (too few long-enough utterances): "
          f"{len(r['speakers_skipped'])} {r['speakers_skipped']}; speakers left over after the last whole batch: "
          f"{len(r['speakers_left_over'])} {r['speakers_left_over']}")
    return 0


def score_dataset(args) -> int:
    return _print_score(args, *_score_setup(args))


def _optimizer_kwargs(args) -> dict:
    """``--optimizer``, the schedule options and ``--optimizer-state`` of a fit command -> the ``optimizer=``, ``scheduler=`` and
    ``opt_state=`` its driver takes.  ``--warmup`` (with ``--milestones``) is ``optim.WarmupScheduler`` from ``--initial-lr`` to
    ``--lr``; ``--milestones`` alone is torch's ``MultiStepLR``; neither: a constant ``--lr``, as before.  ``opt_state`` is what
    ``--optimizer-state`` holds if the file exists, else an empty dict to be filled; None without the option."""
    from . import optim
    kw = {"optimizer": optim.Adam if args.optimizer == "hip" else torch.optim.Adam}
    milestones = [int(m) for m in args.milestones.split(",") if m] if args.milestones else None
    gamma = 0.1 if args.gamma is None else args.gamma
    if args.warmup is not None:
        initial = args.lr if args.initial_lr is None else args.initial_lr
        kw["scheduler"] = lambda opt: optim.WarmupScheduler(opt, args.warmup, initial, args.lr, milestones, gamma)
    elif milestones:
        kw["scheduler"] = lambda opt: torch.optim.lr_scheduler.MultiStepLR(opt, milestones, gamma)
    if args.optimizer_state:
        path = Path(args.optimizer_state)
        kw["opt_state"] = torch.load(path, map_location=args.device, weights_only=True) if path.exists() else {}
    return kw


def _save_optimizer_state(args, kw) -> None:
    if args.optimizer_state:
        state = kw["opt_state"]
        torch.save({k: state.get(k) for k in ("optimizer", "scheduler", "steps_done")}, args.optimizer_state)
        print(f"wrote {args.optimizer_state}: optimizer and scheduler state after {state.get('steps_done', 0)} steps")


def _fit_dataset(args, fit, what, losses, encoder_update, wrote) -> int:
    """The body of the three fit commands: score, ``fit(enc, cpc, by_speaker, ...)``, a summary line -- ``what(cpc)`` was fitted,
    ``losses(r)`` closes it --, score again, and save with ``encoder_update(enc)`` (None: ``"encoder"`` stays as it was), which
    ``wrote(enc, update)`` describes."""
    enc, cpc, by_speaker = _score_setup(args)
    print("before the fit:")
    if _print_score(args, enc, cpc, by_speaker):
        return 1
    okw = _optimizer_kwargs(args)
    r = fit(enc, cpc, by_speaker, steps=args.steps, lr=args.lr, sample_frames=args.sample_frames, seed=args.seed, **okw)
    _save_optimizer_state(args, okw)
    print(f"fitted {what(cpc)} in {r['steps']} steps of Adam (lr {args.lr:g}) over {r['batches']} batches{losses(r)}")
    print("after the fit:")
    rc = _print_score(args, enc, cpc, by_speaker)
    update = encoder_update(enc)
    io.save_fitted_checkpoint(args.out_checkpoint, cpc.state_dict(), None if args.random_init else args.cpc_checkpoint,
                              encoder_state=enc.state_dict() if args.random_init else None,
                              encoder_update=None if args.random_init else update)
    print(f"wrote {args.out_checkpoint}: {wrote(enc, update)}, \"cpc\" replaced ({len(cpc.state_dict())} keys)")
    return rc


def _cpc_losses(r) -> str:
    return f": cpc loss {r['losses'][0]:.6f} -> {r['losses'][-1]:.6f}"


def fit_predictors_dataset(args) -> int:
    return _fit_dataset(args, driver.fit_predictors, lambda cpc: f"{cpc.n_prediction_steps} predictors", _cpc_losses,
                        lambda enc: None, lambda enc, update: "\"encoder\" as it was")


def fit_context_dataset(args) -> int:
    return _fit_dataset(args, functools.partial(driver.fit_context, train_predictors=not args.freeze_predictors),
                        lambda cpc: "the context LSTM" + ("" if args.freeze_predictors else f" and {cpc.n_prediction_steps} predictors"),
                        _cpc_losses, lambda enc: {f"rnn.{k}": v for k, v in enc.rnn.state_dict().items()},
                        lambda enc, update: f"\"encoder\" with rnn.* replaced ({len(update)} keys)")


def fit_encoder_dataset(args) -> int:
    train = tuple(t for t in args.train.split(",") if t)

    def losses(r):
        return (f", codebook {'frozen' if args.freeze_codebook else 'following'}: loss {r['losses'][0] + r['vq_losses'][0]:.6f} -> "
                f"{r['losses'][-1] + r['vq_losses'][-1]:.6f} = cpc loss {r['losses'][0]:.6f} -> {r['losses'][-1]:.6f} + "
                f"vq loss {r['vq_losses'][0]:.2E} -> {r['vq_losses'][-1]:.2E}")

    return _fit_dataset(args, functools.partial(driver.fit_encoder, adapt_codebook=not args.freeze_codebook, train=train),
                        lambda cpc: ", ".join(train), losses, lambda enc: enc.state_dict(),
                        lambda enc, update: f"\"encoder\" replaced ({len(update)} keys)")


def _vocoder_setup(args):
    """Encoder, Vocoder and the waveforms (at 16 kHz) and speaker ids of ``test.json``, for ``score-vocoder`` and ``fit-vocoder``;
    None after a message when a file's speaker is not in ``speakers.json``."""
    import json
    from . import preprocess
    paths = io.read_test_metadata(args.dataset)
    with open(Path(args.dataset) / "speakers.json") as f:
        names = sorted(json.load(f))
    enc, voc = _models(args, need_vocoder=True)
    dev = next(enc.parameters()).device
    waves, speakers = [], []
    for p in paths:
        prefix = p.stem.split("_")[0]
        if prefix not in names:
            print(f"{p.stem}: speaker {prefix!r} is not in speakers.json")
            return None
        rate, a = io.read_wav_file(Path(args.in_dir) / p.stem)
        if rate != 16000:                                      # the resampling of librosa.load(sr=16000), convert.py:54-56
            a = preprocess.resample(torch.as_tensor(a, dtype=torch.float32, device=dev)[None], rate, 16000)[0].cpu().numpy()
        waves.append(a)
        speakers.append(names.index(prefix))
    return enc, voc, paths, waves, speakers


def _vocoder_line(tot) -> str:
    return (f"vocoder loss:{tot['loss']:.4f} nats/sample, {tot['bits_per_sample']:.4f} bits/sample, top-1 accuracy:{tot['accuracy']:.4f} "
            f"over {tot['n_scored']} samples of {tot['n_utterances']} utterances ({tot['n_cut']} samples past the codes cut)")


def score_vocoder_dataset(args) -> int:
    setup = _vocoder_setup(args)
    if setup is None:
        return 1
    enc, voc, paths, waves, speakers = setup
    records, tot = driver.score_vocoder(enc, voc, waves, None, speakers, max_batch=args.max_batch)
    if args.per_utterance:
        for p, r in zip(paths, records):
            loss = r["nll_sum"] / r["n_scored"] if r["n_scored"] else float("nan")
            print(f"{p.stem}: loss:{loss:.4f} nats/sample over {r['n_scored']} samples, correct {r['n_correct']}, "
                  f"codes {r['n_codes']}, samples cut {r['n_cut']}")
    print(_vocoder_line(tot))
    return 0


def _vocoder_parts(train: str):
    """``--train ar,prenet,embeddings`` -> the tuple ``driver.fit_vocoder`` takes."""
    return tuple(t for t in train.split(",") if t)


def fit_vocoder_dataset(args) -> int:
    """score, ``driver.fit_vocoder``, score again on the same utterances, and the vocoder checkpoint (``{"vocoder": state_dict}``,
    as ``convert`` and ``score-vocoder`` read it)."""
    setup = _vocoder_setup(args)
    if setup is None:
        return 1
    enc, voc, paths, waves, speakers = setup
    print("before the fit:")
    print(_vocoder_line(driver.score_vocoder(enc, voc, waves, None, speakers, max_batch=args.max_batch)[1]))
    okw = _optimizer_kwargs(args)
    r = driver.fit_vocoder(enc, voc, waves, None, speakers, steps=args.steps, lr=args.lr, max_batch=min(args.max_batch, 32),
                           clip_codes=args.clip_codes if args.clip_codes > 0 else None, seed=args.seed, train=_vocoder_parts(args.train), **okw)
    _save_optimizer_state(args, okw)
    if r["steps"] == 0:
        print("no utterance with two samples to score: nothing fitted")
        return 1
    fitted = {"ar": "rnnms.ar (embedding, GRU, fc1, fc2)", "prenet": "rnnms.prenet", "embeddings": "code_embedding and speaker_embedding"}
    print(f"fitted {', '.join(fitted[t] for t in _vocoder_parts(args.train))} in {r['steps']} steps of Adam (lr {args.lr:g}) over {r['batches']} batches of "
          f"{r['utterances']} utterances: loss {r['losses'][0]:.6f} -> {r['losses'][-1]:.6f}")
    print("after the fit:")
    print(_vocoder_line(driver.score_vocoder(enc, voc, waves, None, speakers, max_batch=args.max_batch)[1]))
    sd = {k: v.detach().cpu().clone() for k, v in voc.state_dict().items()}
    torch.save({"vocoder": sd}, args.out)
    print(f"wrote {args.out}: \"vocoder\" ({len(sd)} keys; {args.train} refitted, the rest as it was)")
    return 0


def adapt_codebook_dataset(args) -> int:
    paths = io.read_test_metadata(args.dataset)
    enc, _ = _models(args, need_vocoder=False)
    r = driver.adapt_codebook(enc, [io.load_mel(p) for p in paths], epochs=args.epochs, max_batch=args.max_batch)
    for e, (loss, ppl, used) in enumerate(zip(r["loss"], r["perplexity"], r["codes_in_use"])):
        w = r["rows"]                                          # batch means weighted by their rows
        print(f"epoch {e + 1}: vq loss:{sum(l * n for l, n in zip(loss, w)) / sum(w):.2E}, "
              f"perpexlity:{sum(q * n for q, n in zip(ppl, w)) / sum(w):.3f}, codes in use:{used}/{enc.conf.n_embeddings}")
    io.save_adapted_checkpoint(args.out_checkpoint, enc.state_dict(), None if args.random_init else args.cpc_checkpoint)
    print(f"adapted the codebook on {len(paths)} utterances ({sum(r['rows'])} frames) x {args.epochs} epochs -> {args.out_checkpoint}")
    return 0


def abx_line(r) -> str:
    metric = r.get("metric", "angular")
    return (f"abx {r['mode']}: error rate {r['error_rate']:.4f} % over {r['n_triples']} triples, {r['n_pairs']} pairs, "
            f"{r['n_blocks']} blocks" + ("" if metric == "angular" else f", metric {metric}"))


def abx_dataset(args) -> int:
    from . import abx
    items = abx.read_items(args.items)
    if args.features:
        dev = torch.device(args.device)
        feats = {f: torch.from_numpy(io.load_frames_text(Path(args.features) / f)).to(dev) for f in sorted({it.file for it in items})}
        r = abx.score(feats, items, mode=args.mode, frame_shift=args.frame_shift, frame_offset=args.frame_offset)
    else:
        enc, _ = _models(args, need_vocoder=False)
        mels = {p.stem: io.load_mel(p) for p in io.read_test_metadata(args.dataset)}
        r = driver.score_abx(enc, mels, items, feature=args.feature, mode=args.mode, frame_shift=args.frame_shift,
                             frame_offset=args.frame_offset, max_batch=args.max_batch, metric=args.metric)
    if r["n_triples"] == 0:
        print(f"abx {args.mode}: no (A, B, X) triple could be formed from {len(items)} items")
        return 1
    print(abx_line(r))
    return 0


def convert_files(enc, voc, entries, out_dir, seed, max_batch: int = 64, slots: int = 0, timings=None):
    """``convert.py:52-83`` over ``entries`` = [(input path without suffix, speaker id, output name)]: ``.mel.npy`` inputs
    are used as they are; ``.wav`` inputs go through the batched HIP front end (resample at load, reference loudness, log-mel:
    ``driver.front_end_utterances``) and their outputs are re-normalised to the input's loudness (``convert.py:79-80``).
    ``timings``: a dict that receives wall seconds per stage (the device is synchronised at every stage boundary then)."""
    import time
    dev = next(enc.parameters()).device
    t_last = [time.perf_counter()]

    def clock(name):
        if timings is None:
            return
        torch.cuda.synchronize(dev)
        now = time.perf_counter()
        timings[name] = timings.get(name, 0.0) + now - t_last[0]
        t_last[0] = now

    mels = [None] * len(entries)
    wav_ids, waves, rates = [], [], []
    for i, (p, _, _) in enumerate(entries):
        if Path(p).with_suffix(".mel.npy").exists():
            mels[i] = io.load_mel(p).to(dev)
        else:
            rate, a = io.read_wav_file(p)
            wav_ids.append(i); waves.append(a); rates.append(rate)
    clock("read_files")
    ref = {}
    if wav_ids:
        fm, fl = driver.front_end_utterances(waves, rates, dev, max_batch=max_batch, clock=clock)
        for i, m, l in zip(wav_ids, fm, fl):
            mels[i] = m
            ref[i] = l
    wavs = driver.convert_utterances(enc, voc, mels, [s for _, s, _ in entries], seed=seed, max_batch=max_batch, slots=slots,
                                     clock=clock)
    if ref:                                                    # convert.py:79-80, one batched call each way
        ids = sorted(ref)
        for i, w in zip(ids, loudness.match_loudness([wavs[i] for i in ids], [ref[i] for i in ids])):
            wavs[i] = w
    clock("loudness_out")
    host = [w.cpu() for w in wavs]
    clock("download")
    for (_, _, name), w in zip(entries, host):
        io.save_wav(Path(out_dir) / name, w, 16000)
    clock("write_files")
    return wavs


def convert_dataset(args) -> int:
    items, _ = io.read_synthesis_list(args.synthesis_list, Path(args.dataset) / "speakers.json")
    in_dir, out_dir = Path(args.in_dir), Path(args.out_dir)
    out_dir.mkdir(exist_ok=True, parents=True)
    enc, voc = _models(args, need_vocoder=True)
    convert_files(enc, voc, [(in_dir / p, s, name) for p, s, name in items], out_dir, args.seed, max_batch=args.max_batch)
    print(f"converted {len(items)} utterances -> {out_dir}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="vectorquantizedcpc_amd.cli")
    sub = ap.add_subparsers(dest="cmd", required=True)
    for name in ("encode", "convert", "score", "score-vocoder", "fit-vocoder", "adapt-codebook", "fit-predictors", "fit-context", "fit-encoder"):
        p = sub.add_parser(name)
        p.add_argument("--dataset", required=True, help="datasets/<name> directory (test.json, speakers.json)")
        if name in ("encode", "convert"):
            p.add_argument("--out-dir", required=True)
        p.add_argument("--cpc-checkpoint")
        p.add_argument("--random-init", action="store_true", help="seeded random-init weights (no checkpoint ships with the reference)")
        p.add_argument("--device", default="cuda")
        p.add_argument("--max-batch", type=int, default=64)
        if name.startswith("fit-"):
            p.add_argument("--optimizer", choices=("torch", "hip"), default="torch", help="hip: the update is vqcpc_adam_step (optim.Adam)")
            p.add_argument("--warmup", type=int, help="epochs (fit-vocoder: steps) of linear warm-up from --initial-lr to --lr; needs --milestones")
            p.add_argument("--initial-lr", type=float, help="the learning rate the warm-up starts from")
            p.add_argument("--milestones", help="comma-separated epochs (fit-vocoder: steps) at which the rate is multiplied by --gamma, e.g. 300,400")
            p.add_argument("--gamma", type=float, help="the factor at a milestone (default 0.1)")
            p.add_argument("--optimizer-state", help="file of {optimizer, scheduler, steps_done}: read if it exists, written at the end")
        if name in ("score", "fit-predictors", "fit-context", "fit-encoder"):               # config.py:42-47, :202
            p.add_argument("--prediction-steps", type=int, default=12)
            p.add_argument("--speakers", type=int, default=8)
            p.add_argument("--utterances", type=int, default=8)
            p.add_argument("--negatives", type=int, default=17)
            p.add_argument("--sample-frames", type=int, default=128)
            p.add_argument("--seed", type=int, default=synth.SEED)
            if name != "score":
                p.add_argument("--out-checkpoint", required=True)
                p.add_argument("--steps", type=int, default=200)
                p.add_argument("--lr", type=float, default=4e-4, help="Adam's learning rate (config.py's CPC training rate)")
            if name == "fit-context":
                p.add_argument("--freeze-predictors", action="store_true", help="step the LSTM alone")
            if name == "fit-encoder":
                p.add_argument("--train", default=",".join(driver.FIT_ENCODER_PARTS), help="comma-separated parts that step")
                p.add_argument("--freeze-codebook", action="store_true", help="no EMA update of the codebook")
        elif name == "encode":
            p.add_argument("--save-auxiliary", action="store_true")
        elif name == "adapt-codebook":
            p.add_argument("--out-checkpoint", required=True)
            p.add_argument("--epochs", type=int, default=1)
        elif name in ("score-vocoder", "fit-vocoder"):
            p.add_argument("--vocoder-checkpoint")
            p.add_argument("--in-dir", required=True, help="directory of <utterance>.wav files")
            if name == "score-vocoder":
                p.add_argument("--per-utterance", action="store_true", help="also print one line per file")
            else:
                p.add_argument("--steps", type=int, default=200)
                p.add_argument("--lr", type=float, default=4e-4, help="Adam's learning rate")
                p.add_argument("--clip-codes", type=int, default=16, help="codes per training cut (16: the reference's 5120 samples); 0: whole utterances")
                p.add_argument("--seed", type=int, default=synth.SEED)
                p.add_argument("--train", default="ar", help="comma-separated parts that step, of " + ",".join(Vocoder.TRAIN_PARTS) +
                               ": rnnms.ar, rnnms.prenet, and the code and speaker embedding tables")
                p.add_argument("--out", required=True, help="the vocoder checkpoint to write")
        else:
            p.add_argument("--vocoder-checkpoint")
            p.add_argument("--synthesis-list", required=True)
            p.add_argument("--in-dir", required=True)
            p.add_argument("--seed", type=int, default=synth.SEED)
    p = sub.add_parser("abx")
    p.add_argument("--items", required=True, help="items file: '#' header, then file onset offset phone prev next speaker")
    p.add_argument("--mode", choices=("within", "across"), default="within")
    p.add_argument("--frame-shift", type=float, default=0.02, help="seconds between frames (10 ms mel hop x the encoder's stride 2)")
    p.add_argument("--frame-offset", type=float, default=0.01, help="time of frame 0 in seconds")
    p.add_argument("--features", help="directory of <file>.txt frames, as `encode` writes them")
    p.add_argument("--dataset", help="datasets/<name> directory (test.json): encode its mels in-process")
    p.add_argument("--cpc-checkpoint", "--checkpoint", dest="cpc_checkpoint")
    p.add_argument("--random-init", action="store_true")
    p.add_argument("--feature", choices=("z", "c", "indices"), default="z")
    p.add_argument("--metric", choices=("angular", "edit"), default="angular", help="edit: Levenshtein distance between index runs (--feature indices)")
    p.add_argument("--device", default="cuda")
    p.add_argument("--max-batch", type=int, default=64)
    args = ap.parse_args(argv)
    if args.cmd == "abx":
        if bool(args.features) == bool(args.dataset):
            ap.error("abx: give --features DIR or --dataset DIR")
        if args.dataset and not args.random_init and not args.cpc_checkpoint:
            ap.error("abx --dataset: give --cpc-checkpoint or --random-init")
        if args.features and args.feature == "indices":
            ap.error("abx --feature indices needs --dataset: `encode` writes frames, not indices")
        if args.metric != "angular" and args.feature != "indices":
            ap.error(f"abx --metric {args.metric} needs --feature indices")
        return abx_dataset(args)
    if not args.random_init and not args.cpc_checkpoint:
        ap.error("give --cpc-checkpoint (and --vocoder-checkpoint for convert) or --random-init")
    if args.cmd == "fit-encoder":
        parts = [t for t in args.train.split(",") if t]
        if not parts or len(set(parts)) != len(parts) or any(t not in driver.FIT_ENCODER_PARTS for t in parts):
            ap.error(f"fit-encoder --train: name each of {','.join(driver.FIT_ENCODER_PARTS)} at most once, and at least one")
    if args.cmd == "fit-vocoder":
        parts = _vocoder_parts(args.train)
        if not parts or len(set(parts)) != len(parts) or any(t not in Vocoder.TRAIN_PARTS for t in parts):
            ap.error(f"fit-vocoder --train: name each of {','.join(Vocoder.TRAIN_PARTS)} at most once, and at least one")
    if args.cmd.startswith("fit-"):
        if args.warmup is not None and not args.milestones:
            ap.error(f"{args.cmd} --warmup needs --milestones (the warm-up ends before the first)")
        if (args.initial_lr is not None and args.warmup is None) or (args.gamma is not None and not args.milestones):
            ap.error(f"{args.cmd}: --initial-lr goes with --warmup, --gamma with --milestones")
    if args.cmd in ("score-vocoder", "fit-vocoder") and not args.random_init and not args.vocoder_checkpoint:
        ap.error("give --cpc-checkpoint and --vocoder-checkpoint, or --random-init")
    return {"encode": encode_dataset, "convert": convert_dataset, "score": score_dataset,
            "score-vocoder": score_vocoder_dataset, "fit-vocoder": fit_vocoder_dataset, "adapt-codebook": adapt_codebook_dataset,
            "fit-predictors": fit_predictors_dataset, "fit-context": fit_context_dataset,
            "fit-encoder": fit_encoder_dataset}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
