"""deeplip_amd/trainer_common.py on the host: the run plumbing and the speech input chain both trainers are built from.  Nothing here
launches: front-ends are built with device="cpu", encoders stay on the CPU, the chain's stages are stand-ins."""
import os

import pytest
import yaml

from deeplip_amd import launch, trainer_common as tc
from oracle import deeplip_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def config(tmp_path):
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump({"train": {"bs": 4, "gpus_id": [0, 1, 2], "sgd": {"init_lr": 0.1}}, "data": {"n_spk": 5}}))
    return path


# ------------------------------------------------------------------------------------------ run plumbing
def test_load_config_writes_nested_overrides(config):
    opts = tc.load_config(str(config.parent), "cfg.yaml", {"train.sgd.init_lr": 0.5, "data.n_spk": 7})
    assert opts["train"]["sgd"]["init_lr"] == 0.5 and opts["data"]["n_spk"] == 7 and opts["train"]["bs"] == 4


def test_load_config_creates_python_data_config_and_no_other_section(config):
    opts = tc.load_config("/nonexistent", str(config), {"data.python_data_config.test_from_waves": True})      # absolute path: root unused
    assert opts["data"]["python_data_config"] == {"test_from_waves": True}
    with pytest.raises(KeyError):
        tc.load_config(str(config.parent), "cfg.yaml", {"test.batch": 4})
    with pytest.raises(KeyError):
        tc.load_config(str(config.parent), "cfg.yaml", {"data.augment.p_reverb": 0.5})


def test_load_config_reads_the_shipped_configs_relative_to_the_root():
    assert tc.load_config(ROOT, "conf/audio_config.yaml")["model"]["arch"] in ("tdnn", "etdnn", "resnet")
    assert tc.load_config(ROOT, os.path.join(ROOT, "conf/fusion_config.yaml"), {"train.bs": 8})["train"]["bs"] == 8


def test_parse_set_reads_values_as_yaml():
    assert tc.parse_set(["train.bs=8", "data.test_audio_frames=[60, 120]", "train.graph_step=false", "a.b=x=y"]) == \
        {"train.bs": 8, "data.test_audio_frames": [60, 120], "train.graph_step": False, "a.b": "x=y"}


def test_self_launch_sizes_the_job_from_the_flag_the_overrides_or_the_file(config, monkeypatch):
    calls = []
    monkeypatch.setattr(launch, "maybe_self_launch", lambda script, argv, gpus: calls.append((script, gpus)) or 17)
    script = str(config.parent / "train_x.py")
    for k in ("RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    assert tc.self_launch(script, None, "cfg.yaml", {}) == 17                                  # the file's list: 3 GPUs
    assert tc.self_launch(script, None, str(config), {"train.gpus_id": [0, 1]}) == 17          # the overrides win
    assert tc.self_launch(script, 5, "cfg.yaml", {}) == 17                                     # --gpus wins over both
    assert tc.self_launch(script, None, "cfg.yaml", {"train.gpus_id": 0}) == 17                # not a list: one GPU
    assert tc.self_launch(script, None, "cfg.yaml", {}, key="train.no_such_key") == 17
    assert calls == [(script, 3), (script, 2), (script, 5), (script, 1), (script, 1)]
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert tc.self_launch(script, 4, "cfg.yaml", {}) is None and len(calls) == 5               # inside a job: a rank carries on


def test_scheduled_margin_switches_after_epoch_five():
    class Crit:
        margin = None
    c = Crit()
    for epoch, want in ((1, 0.2), (5, 0.2), (6, 0.35)):
        tc.scheduled_margin(c, epoch, 0.2, 0.35)
        assert c.margin == want


# ------------------------------------------------------------------------------------------ speech input chain
@pytest.mark.parametrize("arch,feat,want", [("etdnn", None, "mfcc"), ("tdnn", None, "mfcc"), ("resnet", None, "fbank"),
                                            ("resnet", "logfbank", "logfbank"), ("etdnn", "fbank", "fbank")])
def test_frontend_from_section_sizes_the_features_by_the_encoder(arch, feat, want):
    fe = tc.frontend_from_section({} if feat is None else {"feat_type": feat}, arch, 30, "cpu")
    assert fe.feat_type == want and fe.feat_dim == 30 and fe.normalize is True
    assert (fe.rate, fe.frame_len, fe.frame_step) == (16000, 400, 160)
    assert fe.num_cep == 30 if want == "mfcc" else fe.num_bin == 30


def test_frontend_from_section_stft_and_normalize():
    geom = {"feat_type": "stft", "nfft": 128, "win_len": 0.00625, "win_shift": 0.0025}
    fe = tc.frontend_from_section(geom, "resnet", 65, "cpu", normalize=False)
    assert fe.feat_type == "stft" and fe.feat_dim == 65 and fe.normalize is False and (fe.frame_len, fe.frame_step) == (100, 40)
    with pytest.raises(ValueError, match=r"data\.python_data_config\.test_from_waves: the front-end yields 65 features, the encoder takes 64"):
        tc.frontend_from_section(geom, "resnet", 64, "cpu", where="data.python_data_config.test_from_waves")


def test_voiced_frames_stage_defaults_and_checks_min_keep():
    from deeplip_amd.voiced_frames import parse_voiced_frames_section
    assert tc.voiced_frames_stage(None, 24, "data.voiced_frames") is None
    assert tc.voiced_frames_stage(parse_voiced_frames_section({}), 24, "data.voiced_frames").min_keep == 24
    assert tc.voiced_frames_stage(parse_voiced_frames_section({"min_keep": 30}), 24, "data.voiced_frames").min_keep == 30
    with pytest.raises(ValueError, match=r"data\.python_data_config\.voiced_frames\.min_keep: 23 is below the 24"):
        tc.voiced_frames_stage(parse_voiced_frames_section({"min_keep": 23}), 24, "data.python_data_config.voiced_frames")


def _resnet_cfg(pooling, **extra):
    return {"arch": "resnet", "resnet": dict({"input_dim": 1, "hidden_dim": [32, 64], "residual_block_layers": [1, 1], "fc_layers": 1,
                                             "embedding_dim": 32, "pooling": pooling}, **extra)}


def test_encoder_min_frames_asks_the_encoder():
    et = {"input_dim": 24, "hidden_dim": [512] * 9 + [1500], "context": O.ETDNN_CONTEXT, "tdnn_layers": 10, "embedding_dim": 512,
          "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}
    etdnn = tc.build_speech_encoder({"arch": "etdnn", "etdnn": et})
    assert etdnn.frames_consumed() == 22 and tc.encoder_min_frames(etdnn) == 24
    assert tc.encoder_min_frames(tc.build_speech_encoder(_resnet_cfg("average"))) == 1
    stat = tc.build_speech_encoder(_resnet_cfg("statistic"), feat_dim=24)
    assert tc.encoder_min_frames(stat) == stat.min_frames() == (1 << stat.stages2) + 1 > 1


def test_build_speech_encoder_fills_the_resnet_feat_dim_unless_given():
    cfg = _resnet_cfg("statistic")
    assert tc.build_speech_encoder(cfg, feat_dim=24).feat_dim == 24 and cfg["resnet"]["feat_dim"] == 24
    assert tc.build_speech_encoder(_resnet_cfg("statistic", feat_dim=26), feat_dim=24).feat_dim == 26       # an explicit key wins
    with pytest.raises(NotImplementedError):
        tc.build_speech_encoder({"arch": "lstm"})


class _Stage:
    """A stand-in stage: records its call and marks what passes through."""

    def __init__(self, name, log, **attrs):
        self.name, self.log = name, log
        self.__dict__.update(attrs)

    def __call__(self, x, lengths):
        self.log.append(self.name)
        return x + [self.name], lengths + 1

    def extract_embedding(self, x, lengths=None):
        self.log.append(self.name)
        return (tuple(x), lengths), "second"


def test_speech_chain_runs_its_stages_in_order():
    log = []
    enc = _Stage("encoder", log)
    assert tc.SpeechChain(enc)([], 0) == (((), 0), "second") and log == ["encoder"]
    del log[:]
    chain = tc.SpeechChain(enc, frontend=_Stage("frontend", log), resample=_Stage("resample", log), voiced=_Stage("voiced", log))
    assert chain([], 0) == ((("resample", "frontend", "voiced"), 3), "second")
    assert log == ["resample", "frontend", "voiced", "encoder"]
    del log[:]
    assert tc.SpeechChain(enc, voiced=_Stage("voiced", log))([], 0)[0] == (("voiced",), 1) and log == ["voiced", "encoder"]


def test_speech_chain_wave_geometry_takes_its_four_forms():
    from deeplip_amd.resample import ResampledGeometry
    enc = _Stage("encoder", [])
    mfcc = _Stage("frontend", [], feat_type="mfcc", frame_len=400, frame_step=160)
    stft = _Stage("frontend", [], feat_type="stft", frame_len=100, frame_step=40)
    assert tc.SpeechChain(enc).wave_geometry is None
    assert tc.SpeechChain(enc, voiced=_Stage("voiced", [])).wave_geometry is None
    assert tc.SpeechChain(enc, frontend=mfcc).wave_geometry == (400, 160)
    assert tc.SpeechChain(enc, frontend=stft).wave_geometry is stft
    g = tc.SpeechChain(enc, frontend=mfcc, resample=_Stage("resample", [], up=1, down=3)).wave_geometry
    assert isinstance(g, ResampledGeometry) and g.frontend is mfcc and (g.frame_len, g.frame_step) == (1200, 480)


class _Closable:
    def __init__(self):
        self.closed = 0

    def close(self):
        self.closed += 1


def test_extractor_cache_keeps_one_extractor_per_key():
    cache, built = tc.ExtractorCache(), []

    def build():
        built.append(_Closable())
        return built[-1]
    a = cache.get((4, 0, 1), build)
    assert cache.get((4, 0, 1), build) is a and len(built) == 1 and a.closed == 0       # the same key: nothing is built
    b = cache.get((4, 0, 2), build)                                                    # the weights changed: the old one is closed, once
    assert b is not a and len(built) == 2 and (a.closed, b.closed) == (1, 0)
    cache.close()
    cache.close()
    assert (a.closed, b.closed) == (1, 1)
    assert cache.get((4, 0, 2), build) is built[2]                                     # after close(): built again
