"""What train_audio.py and train_fusion.py share: the run plumbing around a ``Trainer`` (config + ``--set`` overrides, self-launch, run
name, optimizer, margin schedule, the tail of ``main()``) and the speech input chain of extraction (wave -> [resample] -> front-end ->
[voiced frames] -> encoder, and the one RaggedExtractor a trainer keeps): the host glue that decides which launches a recorded plan
holds.  Host-only at import: nothing here touches the GPU or loads the library until a stage is built on a device."""
from __future__ import annotations

import os
import sys
import time

import torch
import yaml

from . import arith, dist as ddist


def load_config(root, config, overrides=None):
    """The config file (absolute, or relative to ``root``) with dotted overrides such as {"train.bs": 8} written into it.  A missing
    section is a KeyError, except ``python_data_config``: an optional section that older configs lack."""
    with open(os.path.join(root, config)) as f:             # (an absolute ``config`` wins over ``root``)
        opts = yaml.safe_load(f)
    for k, v in (overrides or {}).items():
        d = opts
        *path, leaf = k.split(".")
        for p in path:
            d = d.setdefault(p, {}) if p == "python_data_config" else d[p]
        d[leaf] = v
    return opts


def parse_set(pairs):
    """``--set k=v ...`` -> {k: value}, the values read as YAML."""
    return {k: yaml.safe_load(v) for k, v in (kv.split("=", 1) for kv in pairs)}


def self_launch(script_path, gpus, config, overrides, key="train.gpus_id"):
    """One command starts every GPU (the reference: gpus_id -> nn.DataParallel).  Outside a torch.distributed job and asked for N > 1
    GPUs (--gpus, else the length of the config's gpus_id list): run the N-rank job of this same command (deeplip_amd/launch.py) and
    return its exit code; None otherwise.  Runs before anything touches the GPU."""
    from . import launch
    if launch.in_job():
        return None
    script_path = os.path.abspath(script_path)
    if gpus is None:
        ids = load_config(os.path.dirname(script_path), config, overrides)
        for part in key.split("."):
            ids = ids.get(part, {}) if isinstance(ids, dict) else {}
        gpus = len(ids) if isinstance(ids, (list, tuple)) else 1
    return launch.maybe_self_launch(script_path, sys.argv[1:], gpus)


def run_name():
    """The ``log_time`` of a run: one directory name for the job (rank 0's clock)."""
    name = [time.asctime(time.localtime(time.time())).replace(" ", "_")[4:]]
    if ddist.active():
        torch.distributed.broadcast_object_list(name, 0)
    return name[0]


def make_optimizer(kind, groups, opts, graph_step, device):
    """``sgd`` / ``adam`` over ``groups`` from their config section.  A recorded step (``graph_step``) reads its learning rate from a
    device tensor, which MultiStepLR updates in place, and takes the fused kernel; otherwise the plain optimizer."""
    lr = torch.tensor(float(opts["init_lr"]), device=device) if graph_step else opts["init_lr"]
    if kind == "sgd":
        return torch.optim.SGD(groups, lr, momentum=opts["momentum"], weight_decay=opts["weight_decay"], **({"fused": True} if graph_step else {}))
    if kind == "adam":
        return torch.optim.Adam(groups, lr, weight_decay=opts["weight_decay"], **({"capturable": True, "fused": True} if graph_step else {}))
    raise NotImplementedError(kind)


def scheduled_margin(criterion, epoch, init, end):
    """The margin schedule of the margin criteria (train_audio.py:141-145): ``init`` through epoch 5, ``end`` after."""
    criterion.margin = init if epoch <= 5 else end


def report(trainer, fn):
    """The store is on disk and complete (every rank extracted its shard, barrier behind the write): rank 0 scores and prints."""
    if trainer.rank == 0:
        eer, threshold = fn(trainer.log_time)
        print("EER: {:.6f}%".format(eer * 100))


def finish(trainer):
    """The tail of ``main()``: the arithmetic's re-runs reported, the recorded plans released, the job left together."""
    if trainer.rank == 0 and arith.STATS["f32_reruns"]:
        print("arith auto: {} batch(es) computed again in exact f32".format(arith.STATS["f32_reruns"]))
    trainer.close()
    if ddist.active():
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def build_speech_encoder(model_cfg, feat_dim=None, wave_cfg=None):
    """The speech encoder ``model_cfg["arch"]`` names (train_audio.py:60-68).  The ResNet's statistics poolings size their vector by
    the feature dimension, which the data section knows: ``feat_dim`` is filled into the ``resnet`` sub-dict when that leaves it out.
    ``arch: sincnet`` frames the waveform itself: ``rate`` / ``win_len`` / ``win_shift`` of ``wave_cfg`` (the section that
    describes the waveforms: ``data`` of train_audio.py, ``data.python_data_config`` of train_fusion.py) are filled into its ``sinc``
    sub-dict where that leaves them out (16000, 0.025, 0.01 when neither names them)."""
    arch = model_cfg["arch"]
    if arch == "sincnet":
        from .sincnet import GEOMETRY_KEYS, parse_sinc_section
        sinc = model_cfg[arch].get("sinc")
        sinc = dict(sinc) if isinstance(sinc, dict) else ({} if sinc is None else sinc)
        if isinstance(sinc, dict):
            for k in GEOMETRY_KEYS:
                if k in (wave_cfg or {}):
                    sinc.setdefault(k, wave_cfg[k])
        parse_sinc_section(sinc)                                             # (a bad section is a ValueError before any model is built)
        model_cfg[arch]["sinc"] = sinc
    if arch in ("tdnn", "etdnn", "ftdnn", "sincnet"):                        # (ftdnn: conf/audio_config.yaml:84-92; sincnet: 4l)
        from models.audio_models import tdnn
        return tdnn.SpeakerEmbNet(model_cfg)
    if arch == "resnet":                                                     # train_audio.py:64-66 (`import models.resnet`)
        import models.resnet as resnet
        if feat_dim is not None:
            model_cfg[arch].setdefault("feat_dim", int(feat_dim))
        return resnet.SpeakerEmbNet(model_cfg)
    raise NotImplementedError("Other models are not implemented!")           # train_audio.py:67-68


def encoder_min_frames(model) -> int:
    """The shortest utterance the encoder embeds.  The ResNet says itself (one frame, or what leaves two frames on its last map under
    `pooling: statistic`); a TDNN needs what its valid convolutions consume + the two pooled frames of the unbiased std (pooling.py:24-26)."""
    if hasattr(model, "min_frames"):
        return int(model.min_frames())
    return model.frames_consumed() + 2


def frontend_from_section(section, arch, feat_dim, device, normalize=True, where="data.train_from_waves"):
    """The loaders' feature extraction (models/audio_models/datasets.py:65-83) as the GPU front-end, from the config section that
    describes it: MFCC with as many coefficients as the TDNNs take, fbank with ``feat_dim`` bands for ``arch: resnet``; ``feat_type:
    stft`` yields nfft // 2 + 1 bins and has nothing else to choose.  ``where``: the config path named when the sizes disagree."""
    from .frontend import AudioFrontend
    feat = section.get("feat_type", "mfcc" if arch != "resnet" else "fbank")
    size = {} if feat == "stft" else {"num_cep": feat_dim} if feat == "mfcc" else {"num_cep": feat_dim, "num_bin": feat_dim}
    fe = AudioFrontend(feat, rate=int(section.get("rate", 16000)), win_len=float(section.get("win_len", 0.025)),
                       win_shift=float(section.get("win_shift", 0.01)), nfft=int(section.get("nfft", 512)), device=device,
                       normalize=normalize, **size)
    # (mfcc / fbank: num_cep / num_bin were set to feat_dim above, so only stft -- sized by nfft -- can disagree)
    if fe.feat_dim != feat_dim:
        raise ValueError(f"{where}: the front-end yields {fe.feat_dim} features, the encoder takes {feat_dim}")
    return fe


def voiced_frames_stage(opts, min_frames, where):
    """The VoicedFrames stage of a parsed ``voiced_frames`` section (None: off).  ``min_keep`` defaults to the encoder's minimum frame
    count: a row the VAD leaves fewer frames keeps all of its frames, which the extractor has checked on the host."""
    if opts is None:
        return None
    from .voiced_frames import VoicedFrames
    o = dict(opts)
    if o["min_keep"] is None:
        o["min_keep"] = int(min_frames)
    if o["min_keep"] < min_frames:
        raise ValueError(f"{where}.min_keep: {o['min_keep']} is below the {min_frames} frames the speech encoder needs")
    return VoicedFrames(**o)


class SpeechChain:
    """The ordered stages in front of a speech encoder, as one launch-only step function: [resample] -> [front-end] -> [voiced frames]
    -> ``encoder.extract_embedding``.  Without a front-end the input is features and their frame counts."""

    def __init__(self, encoder, frontend=None, resample=None, voiced=None):
        self.encoder, self.frontend, self.resample, self.voiced = encoder, frontend, resample, voiced

    def __call__(self, x, lengths):
        if self.resample is not None:     # datasets.py:459-463: the recording's rate -> the configured one (a row of another length)
            x, lengths = self.resample(x, lengths)
        if self.frontend is not None:     # the frame lengths stay on the device
            x, lengths = self.frontend(x, lengths)
        if self.voiced is not None:       # conf/audio_config.yaml:25: sliding CMN, then the voiced frames alone (a shorter row per utterance)
            x, lengths = self.voiced(x, lengths)
        return self.encoder.extract_embedding(x, lengths=lengths)

    @property
    def wave_geometry(self):
        """What RaggedExtractor's ``wave_geometry`` takes: None for a feature-fed chain; the front-end itself for ``stft`` (its own
        frame count decides), else (frame_len, frame_step); behind a resampler every sample count is at the source rate."""
        fe = self.frontend
        if fe is None:                    # (arch: sincnet frames the waveform itself: its layer stands where the front-end stands)
            fe = getattr(self.encoder, "sinc", None)
        if fe is None:
            return None
        if self.resample is not None:
            from .resample import ResampledGeometry
            return ResampledGeometry(fe, self.resample)
        return fe if fe.feat_type == "stft" else (fe.frame_len, fe.frame_step)


class ExtractorCache:
    """The one RaggedExtractor a trainer keeps: the plans it records serve every list and every later evaluation.  Its plans address
    the encoders' packed weights, so the key names them (batch size, pack generation, state versions): another key closes the held
    extractor and builds a new one."""

    def __init__(self):
        self._held = None

    def get(self, key, build):
        if self._held is not None and self._held[0] != key:
            self.close()
        if self._held is None:
            self._held = (key, build())
        return self._held[1]

    def close(self):
        if self._held is not None:
            self._held[1].close()
            self._held = None
