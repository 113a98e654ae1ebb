"""The three trainers on deeplip_amd/train_loop.py (-m gpu): an eager epoch issues the dlip_* entry points it issued before the step
loop moved into one module, and the recorded default still records every shape it meets.  The cases are the smallest at which the
loop can go wrong: a ring of cached batches that wraps around, more than one crop length, every optional staged tensor present (a
mix-up of names can occur) and only one of them, the mixup step variant with its clip parameters."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

AUDIO = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 2, "data.test_utt_per_spk": 2, "data.audio_frames": 120,
         "train.bs": 8, "train.crop_frames": [60, 120], "train.steps_per_epoch": 3, "train.data_cache": 2}
WAVES = {"data.train_from_waves": True}
AUGMENT = {"snr_levels": [0, 10, 9999], "p_reverb": 0.5, "keep_power": True, "normalize": False, "max_taps": 8192}
SPEEDS = {"speeds": [0.9, 1.0, 1.1]}
SPEC = {"time_warp": 5, "freq_masks": 2, "freq_width": 4, "time_masks": 2, "time_width": 10, "time_ratio": 0.5, "fill": "mean"}
FUSION = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300,       # SMALL of
          "data.trial_targets": 60, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],       # tests/test_trainer_common_gpu.py
          "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 2, "test.batch": 4, "test.write_store": False,
          "train.bs": 6, "train.steps_per_epoch": 3, "model.fusion": "linear"}
VIDEO = ["--batch-size", "3", "--frames", "7", "--steps", "3", "--maxepoch", "1", "--data-cache", "2", "--num-classes", "10"]
CASES = {
    "audio_features": ("audio", {}),
    "audio_waves_all": ("audio", dict(WAVES, **{"data.augment": AUGMENT, "data.speed_perturb": SPEEDS, "data.spec_augment": SPEC})),
    "audio_waves_spec": ("audio", dict(WAVES, **{"data.spec_augment": SPEC})),
    "fusion_linear": ("fusion", {}),
    "video_gray": ("video", []),
    "video_rgb_mixup": ("video", ["--rgb", "--time-masks", "1", "--time-mask-width", "3", "--cutouts", "1", "--cutout-size", "20",
                                  "--mixup-alpha", "0.4"]),
}

# dlip_* entry points issued through _lib.check over ONE eager epoch of each case (train_video: the three steps of main()), read with
# this file's own counter at commit 5f03e89, the last one whose trainers each carried their own step loop.  The epoch counted is the
# SECOND the process runs (a Trainer's second epoch, the second run of main()).  The first epoch, the one that fills the ring, issues
# the same calls and one-off set-up calls on top, counted apart: 17 per speech Trainer, and 2 the first time a process trains at all
# (331 / 358 / 349 / 167 / 1415 / 1424 in a fresh process at that commit, 2 fewer behind any other training in the process).  Whether
# a case is the first training of its process depends on what pytest ran before it, so its first epoch may carry those 2 or not: both
# values are accepted there, and only there -- the fill path itself is host work and copies, no launches; the second epoch's count is exact
PARENT_DLIP_CALLS = {"audio_features": 312, "audio_waves_all": 339, "audio_waves_spec": 330, "fusion_linear": 165,
                     "video_gray": 1413, "video_rgb_mixup": 1422}
TRAINER_SETUP_CALLS = {"audio": 17, "fusion": 0, "video": 0}
PROCESS_SETUP_CALLS = 2


def _count_dlip_calls(fn):
    """tools/bench_tcn_heads.py's counting wrapper around _lib.check (every dlip_* entry point hands its status to it)."""
    spec = importlib.util.spec_from_file_location("bench_tcn_heads", os.path.join(ROOT, "tools", "bench_tcn_heads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.count_dlip_calls(fn)


def run_case(case, recorded, epochs, save_path):
    """``epochs`` epochs of a case (train_video: as many runs of main(), three steps each, every one from the initial weights) ->
    {"calls": dlip_* calls per epoch, "losses": per epoch, "mode": the last step mode reported, "summary": of the recorded steps or
    None, "owner": what holds the trained state}."""
    kind, extra = CASES[case]
    out = {"calls": [], "losses": [], "summary": None}
    if kind == "video":
        import train_video
        res = []
        argv = VIDEO + extra + ["--save-path", str(save_path)] + ([] if recorded else ["--eager-step"])
        for _ in range(epochs):
            out["calls"].append(_count_dlip_calls(lambda: res.append(train_video.main(argv))))
            out["losses"].append(res[-1][0])
        out["mode"] = train_video.train.last_stats["step_mode"]
        plan = train_video.train.last_plan
        out["summary"], out["owner"] = plan.summary() if plan is not None else None, plan
        return out
    torch.manual_seed(0)                    # the criteria's weights come from torch's generator
    if kind == "audio":
        import train_audio
        tr = train_audio.Trainer(overrides=dict(AUDIO, **extra, **{"train.graph_step": recorded}))
    else:
        import train_fusion
        tr = train_fusion.Trainer("train", overrides=dict(FUSION, **extra, **{"train.graph_step": recorded}))
    for epoch in range(1, epochs + 1):
        tr.current_epoch = epoch
        tr._adjust_margin()
        out["calls"].append(_count_dlip_calls(tr._train_epoch))
        out["losses"].append(tr.last_epoch_stats["loss"])
    out["mode"] = tr.last_epoch_stats["step_mode"]
    if recorded:
        out["summary"] = tr._steps.summary()
    out["owner"] = tr
    return out


@pytest.mark.parametrize("case", sorted(CASES))
def test_an_eager_epoch_issues_the_entry_points_it_issued(case, tmp_path, monkeypatch):
    """No stage was added, dropped or doubled on the way into the shared loop: the count equals the parent commit's."""
    monkeypatch.chdir(tmp_path)
    out = run_case(case, False, 2, tmp_path / "ck")
    try:
        print(f"{case}: {out['calls']} dlip_* calls in two eager epochs, losses {out['losses']!r}, mode {out['mode']}")
        assert out["mode"] == "eager" and all(np.isfinite(l) for l in out["losses"])
        assert out["calls"][1] == PARENT_DLIP_CALLS[case]
        assert out["calls"][0] - PARENT_DLIP_CALLS[case] - TRAINER_SETUP_CALLS[CASES[case][0]] in (0, PROCESS_SETUP_CALLS)
    finally:
        if hasattr(out["owner"], "close"):
            out["owner"].close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_recorded_default_records_every_shape_it_meets(case, tmp_path, monkeypatch):
    """Two epochs of the Trainers: a shape records the second time it is met, and the ring's second batch is met once per epoch."""
    monkeypatch.chdir(tmp_path)
    out = run_case(case, True, 2, tmp_path / "ck")
    try:
        print(f"{case}: mode {out['mode']}, recorded steps {out['summary']}, losses {out['losses']!r}")
        assert out["mode"] == "graph"
        assert out["summary"]["recorded"] == out["summary"]["shapes"] >= 1 and out["summary"]["eager_only"] == []
        assert all(np.isfinite(l) for l in out["losses"])
    finally:
        if hasattr(out["owner"], "close"):
            out["owner"].close()
