"""The trainers on deeplip_amd/trainer_common.py (-m gpu): the extractor asks the speech encoder for its shortest utterance, and the
recorded extraction plans hold the launches they held before the chain moved into one module."""
import pytest

pytestmark = pytest.mark.gpu

SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,
         "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],
         "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 4, "test.write_store": False}
WAVES = {"data.python_data_config.test_from_waves": True}
RESNET = {"model.audio_config.arch": "resnet", "data.python_data_config.feat_dim": 26, "data.python_data_config.feat_type": "fbank",
          "model.audio_config.resnet": {"input_dim": 1, "hidden_dim": [32, 64], "residual_block_layers": [1, 1], "fc_layers": 1,
                                        "embedding_dim": 512, "pooling": "average"}}


def test_fusion_extractor_takes_its_minimum_from_the_resnet(tmp_path, monkeypatch):
    """``arch: resnet`` with ``pooling: statistic``: a row must leave two frames on the encoder's last map, and the extractor refuses a
    shorter one on the host.  (The resnet's ``feat_dim`` comes from the data section: the audio_config does not repeat it.)"""
    import train_fusion
    monkeypatch.chdir(tmp_path)
    ov = dict(SMALL, **RESNET)
    ov["model.audio_config.resnet"] = dict(ov["model.audio_config.resnet"], pooling="statistic")
    tr = train_fusion.Trainer("av_test", overrides=ov)
    try:
        assert tr.model_audio.feat_dim == 26 and tr.model_audio.min_frames() > 1
        assert tr._ragged_extractor(4).audio_min_frames == tr.model_audio.min_frames()
    finally:
        tr.close()


# {modality: [(padded item shape, launches of its recorded plan)]} of the lomgrid list under SMALL at batch 4, read at commit 166ae0a
VIDEO = [((1, 7, 88, 88), 21), ((1, 9, 88, 88), 21), ((1, 10, 88, 88), 21), ((1, 12, 88, 88), 21)]
PARENT_LAUNCHES = {
    "features": ({}, [((24, 88), 16), ((24, 96), 16), ((24, 112), 16)]),
    "waves": (WAVES, [((14320,), 23), ((15600,), 23), ((18160,), 23)]),
    "resample_voiced": (dict(WAVES, **{"data.python_data_config.source_rate": 48000, "data.python_data_config.rate": 16000,
                                      "data.python_data_config.voiced_frames": {"vad": {"energy_threshold": -5.0}}}),
                        [((42960,), 27), ((46800,), 27), ((54480,), 27)]),
    "resnet_waves": (dict(RESNET, **WAVES), [((14320,), 21), ((15600,), 21), ((18160,), 21)]),
}


@pytest.mark.parametrize("case", sorted(PARENT_LAUNCHES))
def test_extraction_plans_hold_the_launches_they_held(case, tmp_path, monkeypatch):
    """The chain of every configuration (features; front-end; resampler + front-end + voiced frames; the ResNet) records, per padded
    shape, as many launches as at the commit named above: no stage was added, dropped or doubled."""
    import train_fusion
    monkeypatch.chdir(tmp_path)
    extra, audio = PARENT_LAUNCHES[case]
    tr = train_fusion.Trainer("av_test", overrides=dict(SMALL, **extra))
    try:
        tr.extract_test_xv_lomgrid()
        ex = tr._ragged_extractor(4)
        got = {m: sorted((tuple(k[1][0]), p.launches) for k, p in b.pipes.items()) for m, b in (("a", ex.pa), ("v", ex.pv))}
        assert got == {"a": audio, "v": VIDEO}
        assert tr.extract_stats["plans_recorded"] == len(audio) + len(VIDEO)
    finally:
        tr.close()
