#!/usr/bin/env python3
"""train_audio.py -- x-vector (TDNN / E-TDNN) entry point on the MI355X engine.

Re-creation of the reference's train_audio.py surface that the A+V hot path uses: config schema
(conf/audio_config.yaml: data / model / train / test), ``Trainer`` with the reference's method names --
``__call__`` (:473-483), ``_train`` / ``_train_epoch``, ``_adjust_margin`` (:141-145), ``model_average`` (checkpoint averaging,
:216-232), ``extract_train_xv`` (:234-258), ``save`` / ``load`` / ``load_finetune`` (:260-296), ``train_plda`` (:298-341),
``extract_test_xv`` (x-vector extraction + F.normalize, :343-373), ``extract_test_xv_lomgrid`` / ``_grid`` (:375-437) -- each
extraction leaving the reference's ``exp/<run>/<set>/<utt>.npy`` store, and ``__main__`` scoring it through
``models.audio_models.utils.eer*(log_time)`` as the reference's does (:485-543); modes ``train``, ``test``, ``av_test``, ``av_fusion``.  ``train`` is the reference's loop (train_audio.py:167-199): ``model.train()``, forward
through every TDNN layer with batch-statistics BatchNorm, LMCL / CrossEntropy, ``loss.backward()`` through the
whole encoder (conv dgrad / wgrad, BN and pooling backward as dlip_* launches -- deeplip_amd/autograd.py),
SGD over model + criterion parameters, MultiStepLR, margin schedule, per-epoch checkpoints and checkpoint
averaging.  ``train.freeze_encoder: true`` keeps the older criterion-only step on frozen x-vectors.

A batch is cut to ONE crop length drawn from a short ladder over ``train.crop_frames`` (the collate's random crop,
models/audio_models/datasets.py:112-115) and the optimisation step is recorded once per crop length (and margin) and replayed
(``train.graph_step``, ``--eager-step``); ragged test lists go through ONE extractor per trainer; ``--arith`` / ``model.arith`` pick the
arithmetic (deeplip_amd/arith.py: auto = f16x3 with an in-process f32 re-run -- and calibration -- of what leaves its range).  The run
plumbing (config + ``--set``, self-launch, run name, optimizer, ``main()``'s tail) and the speech input chain of extraction (front-end,
voiced frames, encoder, the kept extractor) are deeplip_amd/trainer_common.py's, the pieces of the step loop deeplip_amd/train_loop.py's.

Data parallelism (the reference wraps the model in nn.DataParallel over ``gpus_id``, train_audio.py:80-83): launched
under ``torch.distributed.run`` every rank draws its own batches, replicas start from rank 0's weights, gradients are
averaged by bucketed all-reduces over RCCL that overlap the backward pass (deeplip_amd.dist.GradBuckets), metrics are
summed over ranks and rank 0 alone writes checkpoints.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from deeplip_amd import _lib, arith, dist as ddist, ops, scoring, train_loop as tl, trainer_common as tc, weightgen as wg  # noqa: E402
from deeplip_amd.synthetic import SyntheticAVSet, synthetic_trials  # noqa: E402
from models.audio_models.loss import AAMSoftmax, ASoftmax, Contrastive, LMCL, CrossEntropy, OnlineTriplet  # noqa: E402


def build_criterion(train_opts, embedding_dim, n_spk):
    """The criterion ``train.loss`` names (train_audio.py:90-97; host-side construction, no GPU needed).  ``LMCL`` and ``AAMSoftmax``
    start at ``train.margin[0]``; ``Triplet`` (conf/audio_config.yaml:130 lists it, the reference's trainer never builds it) is
    OnlineTriplet on the build-owned block ``train.triplet: {margin: 0.2, selector: hardest | semihard | random | all}`` (absent
    block or key: those defaults; one margin for mining and loss).  ``ASoftmax`` and its config spelling ``A-Softmax`` (a stub upstream,
    loss.py:53-59) build deeplip_amd.loss.ASoftmax from the build-owned block ``train.asoftmax: {m: 4, lambda_min: 5.0, lambda_base: 1000.0,
    gamma: 0.12, power: 1.0}``; ``OnlineContrastive`` builds deeplip_amd.loss.Contrastive from ``train.contrastive: {margin: 0.5, selector:
    hard_negative | all}``.  Every other value is CrossEntropy, as upstream -- INCLUDING the config comment's own ``Contrastive``: the
    reference's trainer falls through to CrossEntropy for it and that behaviour is kept, which is why the value that builds the
    contrastive criterion carries the ``Online`` prefix."""
    kind = train_opts["loss"]
    if kind == "LMCL":
        return LMCL(embedding_dim, n_spk, train_opts["scale"], train_opts["margin"][0])
    if kind == "AAMSoftmax":                                            # a stub upstream (loss.py:62-67); ArcFace here
        return AAMSoftmax(embedding_dim, n_spk, train_opts["scale"], train_opts["margin"][0])
    if kind == "Triplet":
        from deeplip_amd.triplet import make_selector
        t = train_opts.get("triplet") or {}
        unknown = sorted(set(t) - {"margin", "selector"})
        if unknown:
            raise ValueError(f"train.triplet: unknown key(s) {unknown}; expected margin, selector")
        if train_opts.get("freeze_encoder", False):
            raise ValueError("train.loss: Triplet has no parameters of its own: train.freeze_encoder would leave nothing to train")
        margin = float(t.get("margin", 0.2))
        return OnlineTriplet(margin, make_selector(str(t.get("selector", "hardest")), margin))
    if kind in ("ASoftmax", "A-Softmax"):
        a = train_opts.get("asoftmax") or {}
        known = ("m", "lambda_min", "lambda_base", "gamma", "power")
        unknown = sorted(set(a) - set(known))
        if unknown:
            raise ValueError(f"train.asoftmax: unknown key(s) {unknown}; expected {', '.join(known)}")
        return ASoftmax(embedding_dim, n_spk, **{k: a[k] for k in known if k in a})
    if kind == "OnlineContrastive":
        from deeplip_amd.pairs import make_pair_selector
        t = train_opts.get("contrastive") or {}
        unknown = sorted(set(t) - {"margin", "selector"})
        if unknown:
            raise ValueError(f"train.contrastive: unknown key(s) {unknown}; expected margin, selector")
        if train_opts.get("freeze_encoder", False):
            raise ValueError("train.loss: OnlineContrastive has no parameters of its own: train.freeze_encoder would leave nothing to train")
        return Contrastive(float(t.get("margin", 0.5)), make_pair_selector(str(t.get("selector", "hard_negative"))))
    return CrossEntropy(embedding_dim, n_spk)


def build_model(model_opts, data_opts):
    """The encoder the ``model`` section names, the ResNet's ``feat_dim`` filled in from the ``data`` section when it is left out."""
    return tc.build_speech_encoder(model_opts, int(data_opts.get("feat_dim", 40)), wave_cfg=data_opts.get("python_data_config") or data_opts)


def check_sincnet(model_opts, data_opts):
    """``arch: sincnet`` (host only): the encoder's first layer reads waveforms and trains, so the step is fed the waveform
    itself -- ``data.train_from_waves: true`` is required -- and ``data.spec_augment`` has no features in front of the step to act on.
    The ``sinc`` sub-dict is checked here too (deeplip_amd.sincnet.parse_sinc_section).  Other architectures pass."""
    if model_opts.get("arch") != "sincnet":
        return
    from deeplip_amd.sincnet import parse_sinc_section
    parse_sinc_section(model_opts["sincnet"].get("sinc"))
    if not bool(data_opts.get("train_from_waves", False)):
        raise ValueError("model.arch: sincnet takes waveforms: set data.train_from_waves: true")
    if data_opts.get("spec_augment") not in (None, False):
        raise ValueError("data.spec_augment acts on the feature batch in front of the step; with model.arch: sincnet the features are "
                         "formed inside the step (waveform augmentation, data.augment / data.speed_perturb, still applies)")


def parse_wave_training(data_opts):
    """(train_from_waves, augment keyword arguments or None) of a ``data`` section (host only).  ``data.augment`` is the section
    deeplip_amd.augment.parse_augment_section checks -- unknown keys, ``p_reverb`` outside [0, 1] and an empty ``snr_levels`` raise
    ValueError -- and needs ``data.train_from_waves``: there is no waveform to augment on the feature path."""
    from deeplip_amd.augment import parse_augment_section
    from_waves = bool(data_opts.get("train_from_waves", False))
    aug = parse_augment_section(data_opts.get("augment"))
    if aug is not None and not from_waves:
        raise ValueError("data.augment: waveform augmentation needs data.train_from_waves: true")
    return from_waves, aug


def parse_speed_perturb(data_opts):
    """The keyword arguments of ``deeplip_amd.resample.SpeedPerturb`` a ``data`` section names (``data.speed_perturb``, a sibling of
    ``data.augment``; host only), or None for an absent one.  Unknown keys and speeds outside [0.5, 2.0] raise ValueError, and so does
    the section without ``data.train_from_waves``: there is no waveform to perturb on the feature path."""
    from deeplip_amd.resample import parse_speed_perturb_section
    sp = parse_speed_perturb_section(data_opts.get("speed_perturb"))
    if sp is not None and not bool(data_opts.get("train_from_waves", False)):
        raise ValueError("data.speed_perturb: speed perturbation needs data.train_from_waves: true")
    return sp


def parse_spec_augment(data_opts):
    """The keyword arguments of ``deeplip_amd.spec_augment.SpecAugment`` a ``data`` section names (``data.spec_augment``; host only), or
    None for an absent one.  The stage acts on the feature batch, so it needs no ``data.train_from_waves``: it is the one augmentation
    the feature-fed path takes.  Unknown keys, counts and widths out of range and a section that would do nothing raise ValueError."""
    from deeplip_amd.spec_augment import parse_spec_augment_section
    return parse_spec_augment_section(data_opts.get("spec_augment"))


class Trainer(object):
    def __init__(self, config="conf/audio_config.yaml", overrides=None, arith_mode=None):
        opts = tc.load_config(ROOT, config, overrides)
        self.train_opts, self.model_opts = opts["train"], opts["model"]
        self.data_opts, self.test_opts = opts["data"], opts["test"]
        # data.train_from_waves / data.augment (build-owned, off by default): batches of WAVEFORMS, augmented on the device and turned
        # into features by the GPU front-end in front of the unchanged step (_train_epoch).  Parsed before anything touches the GPU.
        self.train_from_waves, self.augment_opts = parse_wave_training(self.data_opts)
        # data.speed_perturb (build-owned, absent = off): each training row resampled at a drawn speed in front of the augmentation
        self.speed_opts = parse_speed_perturb(self.data_opts)
        # data.spec_augment (build-owned, absent = off): time warp, frequency and time masks on the feature batch in front of the step,
        # on the feature-fed path and from waves alike; evaluation and extraction never see it
        self.spec_opts = parse_spec_augment(self.data_opts)
        check_sincnet(self.model_opts, self.data_opts)
        # data.voiced_frames (build-owned, absent = off): sliding-window CMN + energy-VAD frame selection in front of the encoder on the
        # feature-fed ragged test lists -- the `nn_input` / `plda_input` pipe (conf/audio_config.yaml:21,25; deeplip_amd/voiced_frames.py).
        from deeplip_amd.voiced_frames import parse_voiced_frames_section
        self.voiced_frames_opts = parse_voiced_frames_section(self.data_opts.get("voiced_frames"))
        # the arithmetic of the engine (--arith > $DLIP_ARITH > model.arith > auto), before the first weight pack
        self.arith = arith.configure(arith_mode, self.model_opts.get("arith"))
        if not torch.cuda.is_available():
            raise RuntimeError("train_audio.py needs a ROCm GPU: the deeplip_amd engine has no CPU path")
        self.device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
        torch.cuda.set_device(self.device)
        self.rank, self.world = ddist.init_from_env(self.device)
        arch = self.model_opts["arch"]
        self.model = build_model(self.model_opts, self.data_opts)
        d = self.data_opts
        # the resnet takes [B,1,F,T] with F = the feature dimension of the data section (train_audio.py:183-184)
        F_ = self.model_opts[arch]["input_dim"] if arch != "resnet" else int(d.get("feat_dim", 40))
        self.trainset = SyntheticAVSet(d["n_spk"], d["utt_per_spk"], 0, 1, F_, d["audio_frames"], key="atrain")
        # test lists hold utterances of differing duration, as the reference's do (data.test_ragged; train_audio.py:343-373 feeds them
        # one at a time at their own lengths); every encoder takes them as length-bucketed ragged batches
        rag = dict(ragged=bool(d.get("test_ragged", False)), audio_range=tuple(d.get("test_audio_frames", (137, 412))))
        self.voxtestset = SyntheticAVSet(d["test_speakers"], d["test_utt_per_spk"], 0, 1, F_, d["audio_frames"], key="atest", **rag)
        # the reference's three A+V evaluation lists (train_audio.py:119-139: lomgriddevloader / lomgridtestloader / gridtestloader)
        self.lomgriddevset = SyntheticAVSet(d["test_speakers"], d["test_utt_per_spk"], 0, 1, F_, d["audio_frames"], key="alomdev", **rag)
        self.lomgridtestset = SyntheticAVSet(d["test_speakers"], d["test_utt_per_spk"], 0, 1, F_, d["audio_frames"], key="alomgrid", **rag)
        self.gridtestset = SyntheticAVSet(d["test_speakers"], d["test_utt_per_spk"], 0, 1, F_, d["audio_frames"], key="agrid", **rag)
        self.resume = self.train_opts.get("resume", "exp/none/net_avg.pth")
        # (the sinc layer keeps its own initial values, mel-spaced band edges: generated ones would not be a filter bank)
        sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in self.model.state_dict().items() if not k.startswith("sinc.")}, prefix="audio.")
        self.model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=arch != "sincnet")
        if arch == "sincnet" and self.voiced_frames_opts is not None:
            raise ValueError("data.voiced_frames selects frames of a feature batch in front of the encoder; model.arch: sincnet forms its "
                             "features inside the encoder")
        self.model.eval().to(self.device)
        E = self.model_opts[arch]["embedding_dim"]
        self.criterion = build_criterion(self.train_opts, E, d["n_spk"]).to(self.device)
        if isinstance(self.criterion, (LMCL, AAMSoftmax)):
            self.init_margin, self.end_margin = self.train_opts["margin"]
        self.triplet = isinstance(self.criterion, (OnlineTriplet, Contrastive))     # no parameters, no logits: (loss, count of tuples)
        self.tuples = "pairs" if isinstance(self.criterion, Contrastive) else "triplets"
        o = self.train_opts["sgd"]
        self.freeze_encoder = bool(self.train_opts.get("freeze_encoder", False))
        groups = [{"params": self.criterion.parameters()}] if self.freeze_encoder else \
                 [{"params": self.model.parameters()}, {"params": self.criterion.parameters()}]   # train_audio.py:112
        if self.triplet:
            groups = groups[:1]         # OnlineTriplet / Contrastive have no parameters: the optimiser gets the model's alone
        # train.graph_step (default on): the optimisation step is recorded once per crop length and replayed as one HIP graph
        # (deeplip_amd/train_plan.py); a recorded step reads its learning rate from a device tensor, which MultiStepLR updates in
        # place, and takes the fused SGD kernel.  train.graph_step: false keeps the loop of eager launches.
        self.graph_step = bool(self.train_opts.get("graph_step", True)) and os.environ.get("DLIP_GRAPH_STEP", "1") != "0"
        self.optim = tc.make_optimizer("sgd", groups, o, self.graph_step, self.device)
        # arch: ftdnn: the semi-orthogonal step on every factor matrix behind optim.step(), each train.semi_orth_every-th
        # optimizer step (build-owned, default 4; 0: off), counted on the device so that a recorded step follows the same schedule
        self.semi_orth = None
        every = self.train_opts.get("semi_orth_every", 4)
        if isinstance(every, bool) or not isinstance(every, int) or every < 0:
            raise ValueError(f"train.semi_orth_every is an int >= 0 (0: off), got {every!r}")
        if getattr(self.model, "factorized_layers", ()) and every > 0 and not self.freeze_encoder:
            from deeplip_amd.audio import SemiOrthStep
            self.semi_orth = SemiOrthStep(self.model, every)
        self._steps = None          # ShapeKeyedSteps, built with the first recorded step
        self._extractor = tc.ExtractorCache()   # one RaggedExtractor for every list and epoch of this trainer (its recorded plans are kept)
        self._cohort = None         # (key, EmbeddingTable): the score-normalisation cohort of the current weights (build_cohort)
        self.lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optim, milestones=self.train_opts["lr_decay_step"], gamma=0.1)
        self.epoch, self.current_epoch = self.train_opts["epoch"], 0
        self.log_time = tc.run_name()
        ddist.broadcast_params(list(self.model.parameters()) + list(self.criterion.parameters()))
        self.buckets = None         # built on the first training step (gradient views need the final placement)
        self._wave_fe, self._augment = self._wave_stages(arch, F_) if self.train_from_waves else (None, None)
        self._speed = None
        if self.speed_opts is not None:
            from deeplip_amd.resample import SpeedPerturb
            self._speed = SpeedPerturb(device=self.device, **self.speed_opts)
        self._spec = None
        if self.spec_opts is not None:
            from deeplip_amd.spec_augment import SpecAugment
            self._spec = SpecAugment(device=self.device, **self.spec_opts)
        self._ring, self._prefetch = tl.BatchRing(self._host_batch, self.train_opts.get("data_cache", 0)), tl.Prefetch(self.device)
        self._speed_out = {}                # data.speed_perturb: width of a staged cut -> samples of its crop

    def _wave_stages(self, arch, feat_dim):
        """data.train_from_waves: the loaders' feature extraction (models/audio_models/datasets.py:65-83) as the GPU front-end -- MFCC
        with as many coefficients as the TDNNs take, fbank with ``feat_dim`` bands for ``arch: resnet`` -- and, with ``data.augment``,
        the waveform augmentation in front of it (train_audio.py:454; a synthetic noise bank and synthetic room responses)."""
        from deeplip_amd.augment import WaveAugment
        from deeplip_amd.synthetic import noise_bank, room_responses
        d = self.data_opts
        if arch == "sincnet":           # the encoder's own first layer frames the waveform: its geometry cuts the crops, the step gets the samples
            fe = self.model.sinc
        else:
            fe = tc.frontend_from_section(d, arch, feat_dim, self.device, where="data.train_from_waves")
        if self.augment_opts is None:
            return fe, None
        import warnings
        with warnings.catch_warnings():                # (the synthetic set holds one response longer than max_taps on purpose)
            warnings.simplefilter("ignore")
            longest = fe.frame_len + (int(d["audio_frames"]) - 1) * fe.frame_step          # samples of the longest crop
            aug = WaveAugment(noise=noise_bank(max(5.0, 1.25 * longest / fe.rate), rate=fe.rate), rirs=room_responses(rate=fe.rate), device=self.device, **self.augment_opts)
        return fe, aug

    def crop_ladder(self):
        """The crop lengths of the training batches.  The reference's collate cuts every batch to ONE random length of 200 .. 400
        frames (models/audio_models/datasets.py:112-115); here that length is drawn from the short geometric ladder of
        deeplip_amd.ragged.rung_tops over ``train.crop_frames`` (neighbouring lengths within ``train.crop_ladder_waste`` = 10 % of
        each other, 8 rungs for 200 .. 400): one recorded step per rung.  No ``crop_frames``: every batch at ``data.audio_frames``."""
        from deeplip_amd.ragged import rung_tops
        cf = self.train_opts.get("crop_frames")
        Ta = int(self.data_opts["audio_frames"])
        if not cf:
            return [Ta]
        lo, hi = int(cf[0]), min(int(cf[1]), Ta)
        lo = min(lo, hi)
        need = self._min_frames()
        if lo < need:
            raise ValueError(f"train.crop_frames: the encoder needs utterances of >= {need} frames")
        return rung_tops(lo, hi, float(self.train_opts.get("crop_ladder_waste", 0.10)), 4 if hi % 4 == 0 else 1)

    def _one_step(self, x, lab):
        """One optimisation step, launches only (what a recorded step replays): train_audio.py:185-200."""
        def forward_loss(x, lab):
            with torch.set_grad_enabled(not self.freeze_encoder):
                emb = self.model(x)                   # output of bn2 / LeakyReLU (train_audio.py:187)
            return self.criterion(emb, lab)
        # (semi_orth behind optim.step() reads and advances its device counter: due or not is decided by the launch)
        return tl.optim_step(forward_loss, self.optim, lambda: self.buckets, self.semi_orth)(x, lab)

    def _adjust_margin(self):
        if isinstance(self.criterion, (LMCL, AAMSoftmax)):
            tc.scheduled_margin(self.criterion, self.current_epoch, self.init_margin, self.end_margin)

    def _host_batch(self, k, rng, ladder):
        """A pinned host batch by name: ``x`` (one crop length of ``ladder``), ``lab`` and each configured augmentation stage's draws under
        the names it takes them by.  Drawn from the epoch's ``rng`` in a fixed order, the optional stages last: a run without one keeps its stream."""
        bs = self.train_opts["bs"]
        idx = rng.integers(0, len(self.trainset), bs)
        T = int(ladder[int(rng.integers(0, len(ladder)))])
        draws = {}
        if self.train_from_waves:
            # the same crop as WAVEFORMS: frame_len + (T - 1) frame_step samples (T frames) cut from the zero-padded batch at
            # an offset that fits the shortest row -- a rectangular batch; the augmentation's choices are drawn beside it.
            # (feat_type stft: the loader cuts the same samples, datasets.py:113-115, and librosa.stft makes T + 2 frames of them)
            fl, fs = self._wave_fe.frame_len, self._wave_fe.frame_step
            Sb = fl + (T - 1) * fs
            # data.speed_perturb: the cut is as wide as the fastest speed needs to leave Sb samples (_features cuts there)
            Sc = Sb if self._speed is None else self._speed.in_samples(Sb)
            wl = self.trainset.wave_len(fl, fs)[idx]
            wav, _ = self.trainset.waves_padded(idx, S=max(int(wl.max()), Sc), frame_len=fl, frame_step=fs)
            s0 = int(rng.integers(0, max(int(wl.min()) - Sc, 0) + 1))
            xb = np.ascontiguousarray(wav[:, s0:s0 + Sc])
            if self._augment is not None:
                draws.update(self._augment.draw([Sb] * bs, rng))         # snr_db, noise_start, rir_idx
            if self._speed is not None:
                self._speed_out[Sc] = Sb
                draws["speed_idx"] = self._speed.draw(bs, rng)["speed_idx"]
        else:
            t0_ = int(rng.integers(0, int(self.data_opts["audio_frames"]) - T + 1))
            xb = np.ascontiguousarray(self.trainset.audio(idx)[:, :, t0_:t0_ + T])   # the batch's one crop (datasets.py:112-115)
        if self._spec is not None:
            draws["draws"] = self._spec.draw(bs, rng)["draws"]
        host = {"x": xb, "lab": self.trainset.labels(idx), **draws}
        return {n: torch.from_numpy(v).pin_memory() for n, v in host.items()}

    def _features(self, b):
        """data.train_from_waves: speed perturbation and augmentation (when configured) and front-end on the staged batch ``b``, eager
        launches in front of the step -- Kaldi's order: the row is resampled to exactly the crop's samples, then reverberated / mixed."""
        wave = b["x"]
        with torch.no_grad():
            if self._speed is not None:
                wave, _ = self._speed(wave, params={"speed_idx": b["speed_idx"]}, out_samples=self._speed_out[wave.shape[1]])
            if self._augment is not None:
                wave = self._augment(wave, params={n: b[n] for n in ("snr_db", "noise_start", "rir_idx")})
            if getattr(self.model, "sinc", None) is not None:      # arch: sincnet -- the layer runs inside the step, on the waveform itself
                return wave
            return self._wave_fe(wave)

    def _train_epoch(self):
        """train_audio.py:167-199 on the synthetic set: full-encoder step (or criterion-only with freeze_encoder)."""
        bs = self.train_opts["bs"]
        rng = np.random.Generator(np.random.PCG64([self.current_epoch, 5, self.rank]))    # every rank its own batches
        self.model.train(not self.freeze_encoder)
        if ddist.active() and self.buckets is None:
            self.buckets = ddist.GradBuckets([p for g in self.optim.param_groups for p in g["params"]])
        steps = self.train_opts.get("steps_per_epoch", 2)
        ladder = self.crop_ladder()
        recorded = self.graph_step and tl.records_with(self.buckets)
        if recorded and self._steps is None:
            mods = [self.criterion] if self.freeze_encoder else [self.model, self.criterion]
            if self.semi_orth is not None:
                mods = mods + [self.semi_orth]         # (its step counter is part of what a step mutates: snapshot / restore cover it)
            self._steps = tl.recorded_steps(self._one_step, mods, [self.optim], self.buckets, self.device, branch_streams=self.buckets is None)
        meter = tl.EpochMeter(self.device)
        anneal = getattr(self.criterion, "anneal", None)
        staged = self._prefetch.stage(self._ring.get(0, rng, ladder)) if steps > 0 else None
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        for i in range(steps):
            b = self._prefetch.take(staged)
            x, lab = b["x"], b["lab"]
            if self.train_from_waves:
                x = self._features(b)
            if self._spec is not None:   # on the feature batch, directly in front of the step and outside the recorded graph
                with torch.no_grad():
                    x = self._spec(x, params={"draws": b["draws"]})
            if anneal is not None:
                anneal()                 # ASoftmax: lambda of this step, written on the device in front of the step, outside the recorded graph
            if recorded:
                # keyed by the crop length (the shape) AND the margin the criterion bakes into the recorded launches
                loss, logits = self._steps.step(x, lab, key=float(getattr(self.criterion, "margin", 0.0)))
            else:
                loss, logits = self._one_step(x, lab)
            # (OnlineTriplet returns the number of triplets, a device scalar, where the classifiers return logits)
            meter.add(loss, logits.detach().double() if self.triplet else (torch.max(logits.detach(), dim=1)[1] == lab).sum(), x.shape[0])
            staged = self._prefetch.stage(self._ring.get(i + 1, rng, ladder)) if i + 1 < steps else None      # copies behind this step
        if recorded:
            self._steps.finish()
        tot, correct, n = meter.read()
        _lib.check_range(sync=True)                       # f16x3 packing: an overflow in this epoch is an error, not a NaN
        dt = time.perf_counter() - t0
        tot, correct, n = ddist.allreduce_metrics([tot, correct, n], self.device)
        # Triplet: there are no logits, hence no accuracy; the statistics carry the mean number of triplets per step (and rank) instead
        quality = {self.tuples: correct / max(steps * self.world, 1)} if self.triplet else {"acc": correct / n}
        self.last_epoch_stats = {"loss": tot / n, **quality, "utt_per_s": n / dt, "steps": steps, "bs": bs * self.world,
                                 "step_mode": (self._steps.mode if recorded else "eager"), "crop_ladder": [int(t) for t in ladder]}
        if self.train_from_waves:
            self.last_epoch_stats.update(from_waves=True, augment=None if self.augment_opts is None else dict(self.augment_opts))
            if self.speed_opts is not None:
                self.last_epoch_stats.update(speed_perturb=dict(self.speed_opts))
        if self.spec_opts is not None:
            self.last_epoch_stats.update(spec_augment=dict(self.spec_opts))
        self.model.eval()
        return tot / n

    def _train(self):
        for epoch in range(self.current_epoch + 1, self.epoch + 1):
            self.current_epoch = epoch
            self._adjust_margin()
            loss = self._train_epoch()
            st = self.last_epoch_stats
            quality = "{}/step {:.0f}".format(self.tuples, st[self.tuples]) if self.triplet else "acc {:.3f}".format(st["acc"])
            print("Epoch {} loss {:.4f} {} ({:.0f} utt/s, {} steps of {})".format(epoch, loss, quality, st["utt_per_s"],
                                                                              st["steps"], st["bs"]), flush=True)
            self.lr_scheduler.step()
            self.save()
            if ddist.active():
                torch.distributed.barrier()     # rank 0's checkpoint is on disk before anybody averages / resumes

    def save(self, filename=None):
        path = "exp/{}/{}".format(self.log_time, filename or "net_{}.pth".format(self.current_epoch))
        if self.rank != 0:          # replicas are identical: one writer
            return path
        os.makedirs(os.path.dirname(path), exist_ok=True)
        # keys carry the DataParallel 'module.' prefix like the reference's checkpoints (train_audio.py:262)
        torch.save({"epoch": self.current_epoch, "state_dict": {"module." + k: v for k, v in self.model.state_dict().items()},
                    "criterion": self.criterion.state_dict(), "optimizer": self.optim.state_dict(),
                    **({"semi_orth": self.semi_orth.state_dict()} if self.semi_orth is not None else {})}, path)
        return path

    def load(self, resume):
        """Resume from one of this trainer's checkpoints or from a reference one (train_audio.py:234-296): there
        ``criterion`` is the pickled criterion MODULE (train_audio.py:264), and ``net_avg.pth`` (written by
        model_average, :229-232) has neither ``criterion`` nor ``epoch``."""
        import pickle
        try:
            ck = torch.load(resume, map_location="cpu", weights_only=True)       # tensors and plain containers only
        except pickle.UnpicklingError as ex:   # what torch raises for anything beyond that; a missing / truncated file propagates as itself
            # a reference checkpoint pickles the criterion MODULE: loading it executes the pickle, i.e. arbitrary code.
            # Allowed only on request (train.allow_pickled_checkpoints: True / DLIP_ALLOW_PICKLED_CHECKPOINTS=1).
            if not (self.train_opts.get("allow_pickled_checkpoints") or os.environ.get("DLIP_ALLOW_PICKLED_CHECKPOINTS") == "1"):
                raise RuntimeError(f"{resume} holds pickled objects (a reference-style checkpoint stores the criterion module); loading it "
                                   "runs code from the file. Set train.allow_pickled_checkpoints: True (or "
                                   "DLIP_ALLOW_PICKLED_CHECKPOINTS=1) if you trust it.") from ex
            ck = torch.load(resume, map_location="cpu", weights_only=False)
        self.model.load_state_dict({k.replace("module.", "", 1) if k.startswith("module.") else k: v for k, v in ck["state_dict"].items()})
        crit = ck.get("criterion")
        if crit is not None:
            if isinstance(crit, torch.nn.Module):
                crit = crit.state_dict()
            self.criterion.load_state_dict(crit)
        if self.semi_orth is not None and ck.get("semi_orth") is not None:
            self.semi_orth.load_state_dict(ck["semi_orth"])      # the optimizer-step count the constraint's schedule runs on
        self.current_epoch = int(ck.get("epoch", self.current_epoch))

    def model_average(self, avg_num=4):
        """train_audio.py:216-232: average the state dicts of the last ``avg_num`` epoch checkpoints."""
        paths = ["exp/{}/net_{}.pth".format(self.log_time, e) for e in range(self.current_epoch - avg_num + 1, self.current_epoch + 1)]
        paths = [p for p in paths if os.path.exists(p)]
        avg = None
        for p in paths:
            sd = torch.load(p, map_location="cpu")["state_dict"]
            avg = {k: v.clone().double() for k, v in sd.items()} if avg is None else {k: avg[k] + v.double() for k, v in sd.items()}
        own = self.model.state_dict()
        avg = {k.replace("module.", "", 1): (v / len(paths)).to(own[k.replace("module.", "", 1)].dtype) for k, v in avg.items()}
        self.model.load_state_dict(avg)
        if self.rank == 0 and paths:      # the file the reference's extract_* methods load (train_audio.py:229-232,300,346)
            torch.save({"state_dict": {"module." + k: v for k, v in avg.items()}}, "exp/{}/net_avg.pth".format(self.log_time))
        return len(paths)

    def _xvectors(self, dataset, batch=64, normalize=True):
        """The embedding the reference extracts (train_audio.py:362-366): CrossEntropy -> the 1st fc layer's output; LMCL (and
        the ArcFace stand-in) -> the 2nd fc layer's, L2-normalised (``F.normalize``) for the test lists."""
        rows = []
        ce = self.train_opts["loss"] == "CrossEntropy"
        self.model.eval()
        if self.voiced_frames_opts is not None and not dataset.ragged:
            raise ValueError("data.voiced_frames needs data.test_ragged: true (the stage hands the encoder one length per utterance)")
        sinc = getattr(self.model, "sinc", None)
        if sinc is not None and not dataset.ragged:
            raise ValueError("model.arch: sincnet extracts from the lists' waveforms: set data.test_ragged: true (the rectangular lists "
                             "are fed features)")
        with torch.no_grad():
            if dataset.ragged:
                # utterances at their own lengths (train_audio.py:343-373 feeds them one by one): length-bucketed batches,
                # every row equal to the one-at-a-time result (deeplip_amd/extract.py).  ONE extractor per trainer: the plans it
                # records (a dozen padded shapes x two input sets) serve every list and every epoch's evaluation.
                D = self.model.embedding_dim
                ex = self._ragged_extractor(batch)
                both, _ = ex.run(dataset, 0, len(dataset), 2 * D, waves=sinc is not None)
                self.extract_stats = dict(ex.stats)
                xv, x_a = both[:, :D].contiguous(), both[:, D:].contiguous()
                rows.append(x_a if ce else ops.l2_normalize(xv) if normalize else xv)
            else:
                for b0 in range(0, len(dataset), batch):
                    idx = list(range(b0, min(len(dataset), b0 + batch)))
                    xv, x_a = self.model.extract_embedding(torch.from_numpy(dataset.audio(idx)).to(self.device))
                    rows.append(x_a if ce else ops.l2_normalize(xv) if normalize else xv)
        table = scoring.EmbeddingTable(dataset.utt_ids, torch.cat(rows))
        _lib.check_range(sync=True)       # a range report of the LAST batch must surface here, not at some later call
        return table

    def _ragged_extractor(self, batch):
        """The trainer's RaggedExtractor (built on first use, per batch size).  Its recorded plans address the model's packed
        weights: a plan whose weights changed since (training, a checkpoint load) is stale -- the extractor is rebuilt then."""
        from deeplip_amd import holders, packing
        from deeplip_amd.extract import RaggedExtractor

        def build():
            chain = tc.SpeechChain(self.model, voiced=self._voiced_frames_stage())
            # (arch: sincnet: run(waves=True) feeds waveforms and sample counts, planned on the layer's frame geometry)
            geom = {} if chain.wave_geometry is None else {"wave_geometry": chain.wave_geometry}
            return RaggedExtractor(lambda a, l: torch.cat(chain(a, l), dim=1), None, self.device, batch=batch,
                                   audio_min_frames=self._min_frames(), **geom)
        return self._extractor.get((int(batch), holders.PACK_GEN[0], packing.state_version(self.model, self.device)), build)

    def _voiced_frames_stage(self):
        """The VoicedFrames stage of data.voiced_frames (None: off)."""
        return tc.voiced_frames_stage(self.voiced_frames_opts, self._min_frames(), "data.voiced_frames")

    def _min_frames(self) -> int:
        return tc.encoder_min_frames(self.model)

    def close(self):
        """Release the recorded extraction plans (their arenas) and the recorded training steps."""
        self._extractor.close()
        self._steps = None

    def _load_for_extract(self, avg_only=False):
        """train_audio.py:235-236,300-301 (net_avg.pth if the run has one) / :345-347,377-379 (``resume`` unless fine-tuning)."""
        avg = "exp/{}/net_avg.pth".format(self.log_time)
        if avg_only:
            if os.path.exists(avg):
                self.load(avg)
        elif os.path.exists(self.resume) and self.train_opts.get("train_type") != "finetune":
            self.load(self.resume)

    def _store(self, sub, table, flat=False):
        """One ``[1, D]`` .npy per utterance under exp/<run>/<sub>/ (train_audio.py:367-369); rank 0 writes."""
        if self.rank == 0 and self.test_opts.get("write_store", True):
            root = "exp/{}/{}".format(self.log_time, sub)
            if flat:                      # train_plda stores by basename (train_audio.py:320-322)
                scoring.EmbeddingTable([os.path.basename(u) for u in table.utt_ids], table.emb).save_npy_tree(root)
            else:
                table.save_npy_tree(root)
        if ddist.active():
            torch.distributed.barrier()

    def score_norm(self):
        """The run's score normalisation (build-owned): ``test.score_norm`` (none | znorm | tnorm | snorm | asnorm,
        default none), ``test.score_norm_top_k`` (asnorm's cohort cut, default 300) and ``test.cohort`` (speaker_mean: one row per
        training speaker, the mean of that speaker's x-vectors; utterances: every training x-vector) -> (kind or None, top_k, form)."""
        kind = scoring.score_norm_kind(self.test_opts.get("score_norm", "none"))
        form = str(self.test_opts.get("cohort", "speaker_mean"))
        if form not in ("speaker_mean", "utterances"):
            raise ValueError("test.cohort: {!r} is neither 'speaker_mean' nor 'utterances'".format(form))
        return kind, int(self.test_opts.get("score_norm_top_k", 300)), form

    def build_cohort(self, batch=64):
        """The normalisation cohort of this run, from the training list's x-vectors (``extract_train_xv``): speaker means over the
        training set's own labels, or the utterances themselves; L2-normalised where the test x-vectors are; rank 0 writes it
        under exp/<run>/cohort_xv/ (one file per row).  None when no normalisation is set.  Kept until the weights change."""
        from deeplip_amd import holders, packing
        kind, _, form = self.score_norm()
        if kind is None:
            return None
        key = (form, holders.PACK_GEN[0], packing.state_version(self.model, self.device))
        if self._cohort is not None and self._cohort[0] == key:
            return self._cohort[1]
        train = self.extract_train_xv(batch)
        if form == "speaker_mean":
            lab = self.trainset.labels(np.arange(len(self.trainset)))
            emb = scoring.speaker_mean_cohort(train.emb, lab)
            ids = ["spk{:05d}.npy".format(int(l)) for l in scoring.speaker_groups(lab)[2]]
        else:
            emb, ids = train.emb, train.utt_ids
        if self.train_opts["loss"] != "CrossEntropy":       # as _xvectors normalises the test lists
            emb = ops.l2_normalize(emb)
        table = scoring.EmbeddingTable(ids, emb)
        self._store("cohort_xv", table)
        self._cohort = (key, table)
        return table

    def _point_score_norm(self, fns):
        """Point the cosine entry points ``fns`` at this run's normalisation and cohort store (they are called with one argument)."""
        from deeplip_amd import scoring_entry as se
        kind, top_k, _ = self.score_norm()
        if kind is None:
            return
        self.build_cohort()
        if not self.test_opts.get("write_store", True):
            return
        for fn in fns:
            se.set_paths(fn, score_norm=kind, top_k=top_k, cohort_dir="exp/{}/cohort_xv".format(self.log_time))

    def extract_test_xv(self, batch=64):
        """x-vectors of the test set, L2-normalised (train_audio.py:343-373) -> EmbeddingTable (+ exp/<run>/test_xv/)."""
        self._load_for_extract()
        self.table = self._xvectors(self.voxtestset, batch)
        self._store("test_xv", self.table)
        self._point_scoring("eer", self.voxtestset, "task")
        return self.table

    def extract_train_xv(self, batch=64):
        """train_audio.py:234-258: embeddings of the training list, NOT normalised, under exp/<run>/train_xv/."""
        self._load_for_extract(avg_only=True)
        self.train_table = self._xvectors(self.trainset, batch, normalize=False)
        self._store("train_xv", self.train_table)
        return self.train_table

    def extract_test_xv_lomgrid(self, batch=64):
        """train_audio.py:375-405 -> exp/<run>/test_xv_lomgrid/."""
        self._load_for_extract()
        self.lomgrid_table = self._xvectors(self.lomgridtestset, batch)
        self._store("test_xv_lomgrid", self.lomgrid_table)
        self._point_scoring("lomgrid", self.lomgridtestset, "trial_lomgrid")
        return self.lomgrid_table

    def extract_test_xv_grid(self, batch=64):
        """train_audio.py:407-437 -> exp/<run>/test_xv_grid/."""
        self._load_for_extract()
        self.grid_table = self._xvectors(self.gridtestset, batch)
        self._store("test_xv_grid", self.grid_table)
        self._point_scoring("grid", self.gridtestset, "trial_grid")
        return self.grid_table

    def _point_scoring(self, name, dataset, fname):
        """The synthetic trial list of a test set, written in the reference's format, and this run's scoring calls pointed at
        it (the reference hard-codes ``task.txt`` / ``data/trial/A_*_trial_2w``: models/audio_models/utils.py:237,254,271)."""
        from deeplip_amd import scoring_entry as se
        if not self.test_opts.get("write_store", True):
            return
        path = "exp/{}/{}.txt".format(self.log_time, fname)
        if self.rank == 0:
            y, pairs = synthetic_trials(dataset, self.data_opts["trials"], self.data_opts["trial_targets"])
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as fh:
                fh.writelines("{} {} {}\n".format(int(l), a, b) for l, (a, b) in zip(y, pairs))
        if ddist.active():
            torch.distributed.barrier()
        for fn in (("eer",) if name == "eer" else ("eer_cos_" + name, "eer_plda_" + name)):
            se.set_paths(fn, trial=path)
        self._point_score_norm(("eer",) if name == "eer" else ("eer_cos_" + name,))     # the PLDA entry points refuse one

    def train_plda(self, n_principal_components=20):
        """train_audio.py:298-341: x-vectors of the LombardGRID development list -> exp/<run>/dev_xv_lomgrid/<basename>.npy, labels
        from the speaker id in the file name (``s<k>_...``), a PLDA model with ``n_principal_components=20`` fitted on them
        (host: the `plda` package's algorithm, deeplip_amd/plda.py) -> ``exp/plda.pkl``."""
        from deeplip_amd.plda import PLDA
        self._load_for_extract(avg_only=True)
        dev = self._xvectors(self.lomgriddevset)
        self._store("dev_xv_lomgrid", dev, flat=True)
        labels = [int(os.path.basename(u).split("_")[0].replace("s", "")) for u in dev.utt_ids]      # :334
        X = dev.emb.cpu().numpy()
        self.plda = PLDA.fit(X, labels, n_principal_components=min(n_principal_components, X.shape[1], max(2, len(set(labels)) - 1)))
        if self.rank == 0:
            self.plda.save("exp/plda.pkl")
        if ddist.active():
            torch.distributed.barrier()
        return self.plda

    def load_finetune(self, resume, param_groups=None):
        """train_audio.py:276-296: load an encoder checkpoint, freeze the encoder and rebuild optimizer + schedule over the
        criterion's parameters alone (``param_groups`` is overwritten there too)."""
        print("loading model from {}".format(resume))
        self.log_time = resume.split("/")[1]
        self.load(resume)
        for p in self.model.parameters():
            p.requires_grad = False
        self.freeze_encoder = True
        self.semi_orth = None           # (a frozen encoder's factor matrices stay as the checkpoint holds them)
        param_groups = [{"params": self.criterion.parameters()}]
        kind = self.train_opts.get("type", "sgd")
        if kind not in ("sgd", "adam"):
            raise NotImplementedError(kind)
        self.optim = tc.make_optimizer(kind, param_groups, self.train_opts[kind], self.graph_step, self.device)
        self.lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(self.optim, milestones=self.train_opts["lr_decay_step"], gamma=0.1)
        self.buckets = None
        self._steps = None              # the recorded steps addressed the old optimizer's state

    def __call__(self):
        """train_audio.py:473-483."""
        if self.rank == 0:
            print("[LOG Time: {}]".format(self.log_time))
            os.makedirs("exp/{}".format(self.log_time), exist_ok=True)
        self._train()

    def eer(self):
        y, pairs = synthetic_trials(self.voxtestset, self.data_opts["trials"], self.data_opts["trial_targets"])
        ia, ib = self.table.trial_indices(pairs)
        s = scoring.cosine_scores(self.table.emb, ia, ib)
        kind, top_k, _ = self.score_norm()
        if kind is not None:
            s = scoring.normalised_scores(self.table.emb, ia, ib, self.build_cohort().emb, kind, top_k, scores=s)
        return scoring.eer_from_scores(y, s.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="test", choices=["train", "test", "av_test", "av_fusion"])    # reference: hard-coded at :486
    ap.add_argument("--config", default="conf/audio_config.yaml")
    ap.add_argument("--set", nargs="*", default=[])
    ap.add_argument("--run", default=None, help="name of an existing exp/<run>/ directory to score (av_fusion; the reference edits log_time by hand)")
    ap.add_argument("--gpus", type=int, default=None,
                    help="GPUs of this node, one process each (default: len(train.gpus_id), as the reference sizes nn.DataParallel: "
                         "train_audio.py:80-83)")
    ap.add_argument("--eager-step", action="store_true",
                    help="training: issue every launch of every step from Python instead of replaying one recorded HIP graph per crop "
                         "length (train.graph_step: false)")
    arith.add_argument(ap)
    a = ap.parse_args()
    ov = tc.parse_set(a.set)
    rc = tc.self_launch(__file__, a.gpus, a.config, ov)
    if rc is not None:
        sys.exit(rc)
    if a.eager_step:
        ov["train.graph_step"] = False
    tr = Trainer(a.config, ov, arith_mode=a.arith)
    from models.audio_models import utils           # the scoring entry points, called as train_audio.py:499-543 calls them

    if a.mode == "train":
        tr()
        tr.model_average(min(4, tr.epoch))
        tr.extract_test_xv()
        tc.report(tr, utils.eer)
    elif a.mode == "test":
        tr.extract_test_xv()
        tc.report(tr, utils.eer)
    else:                           # av_test: cosine / PLDA on the x-vectors (train_audio.py:504-520)
        if a.run:
            tr.log_time = a.run     # av_fusion scores the stores an earlier run left under exp/<run>/ (:521-543: extraction commented out)
        if a.mode == "av_test" and tr.test_opts.get("train_plda"):
            tr.train_plda()
        for name in ("lomgrid", "grid"):
            if not tr.test_opts.get("eval_" + name, True):
                continue
            if a.mode == "av_test":
                getattr(tr, "extract_test_xv_" + name)()
            if tr.test_opts.get("use_cos", True):
                tc.report(tr, getattr(utils, "eer_cos_" + name + ("_featurefusion" if a.mode == "av_fusion" else "")))
            if tr.test_opts.get("use_plda"):
                tc.report(tr, getattr(utils, "eer_plda_" + name))
    tc.finish(tr)


if __name__ == "__main__":
    main()
