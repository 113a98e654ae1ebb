#!/usr/bin/env python3
"""The criteria side by side at the shipped batch: forward + backward of one criterion call on B = 256 embeddings of E = 512 features --
ASoftmax beside LMCL over K = 1211 classes, Contrastive (both selectors) beside OnlineTriplet(hardest) over 57 speakers -- eager
(launches issued from Python) and inside a recorded plan (torch.cuda.CUDAGraph replay, what a recorded training step does), in us per
call.  ``--big`` adds the pair / triplet criteria at B = 1024 (the hard-negative selection counts ranks: O(B^2) compares per row).
``--trainer`` adds train_audio's recorded step (shipped config, one crop length, cached batches) per criterion: ms per step from the
second epoch's utt/s.

    python tools/bench_criteria.py [--iters 100] [--big] [--trainer]

Engine only, one process; prints one line per measurement and one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeplip_amd import pairs as pr, triplet as tp, weightgen as wg  # noqa: E402
from deeplip_amd.loss import ASoftmax, Contrastive, LMCL, OnlineTriplet  # noqa: E402


def inputs(B, E, S):
    labels = np.minimum((wg.gen("bench_criteria.labels", (B,), kind="uniform") * S).astype(np.int64), S - 1)
    x = 0.1 * (0.2 * wg.gen("bench_criteria.centres", (S, E))[labels] + wg.gen("bench_criteria.noise", (B, E)))
    return torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(labels).cuda()


REPEATS = 5


def timed(fn, iters):
    """us per call between two events on the current stream: REPEATS windows of ``iters`` calls after 3 warm-up calls ->
    [median, min, max] over the windows."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    got = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        got.append(e0.elapsed_time(e1) / iters * 1e3)
    got.sort()
    return [round(got[len(got) // 2], 1), round(got[0], 1), round(got[-1], 1)]


def show(name, B, r):
    e, g = r["eager_us"], r["replay_us"]
    print(f"{name:34s} B {B}: eager {e[0]:8.1f} ({e[1]:.1f} - {e[2]:.1f}) us, recorded {g[0]:8.1f} ({g[1]:.1f} - {g[2]:.1f}) us per forward + backward")


def measure(crit, x, lab, iters, stream):
    with torch.cuda.stream(stream):          # (the leaf's gradient accumulator belongs to the stream that captures)
        xg = x.clone().requires_grad_()

    def step():
        xg.grad = None
        for p in crit.parameters():
            p.grad = None
        loss, _ = crit(xg, lab)
        loss.backward()
        return loss

    with torch.cuda.stream(stream):
        eager = timed(step, iters)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            step()
        replay = timed(g.replay, iters)
    return {"eager_us": eager, "replay_us": replay}


def trainer_step_ms(loss, extra=None):
    import train_audio
    ov = {"train.loss": loss, "train.crop_frames": None, "train.steps_per_epoch": 40, "train.epoch": 2, "train.data_cache": 4, **(extra or {})}
    tr = train_audio.Trainer(overrides=ov)
    tr.save = lambda *a, **k: None           # a measurement: no checkpoints
    tr._train()
    st = tr.last_epoch_stats
    return {"ms_per_step": round(st["bs"] / st["utt_per_s"] * 1e3, 3), "utt_per_s": round(st["utt_per_s"], 1), "step_mode": st["step_mode"], "bs": st["bs"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--trainer", action="store_true")
    a = ap.parse_args()
    out = {"iters": a.iters, "device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()
    B, E = 256, 512
    x, lab = inputs(B, E, 1211)
    torch.manual_seed(0)
    for name, crit in (("LMCL K=1211", LMCL(E, 1211, 30.0, 0.2)), ("ASoftmax K=1211 m=4", ASoftmax(E, 1211))):
        out[name] = measure(crit.cuda(), x, lab, a.iters, stream)
        show(name, B, out[name])
    for B in (256, 1024) if a.big else (256,):
        x, lab = inputs(B, E, 57)
        for name, crit in (("OnlineTriplet hardest", OnlineTriplet(0.2, tp.make_selector("hardest", 0.2))),
                           ("Contrastive hard_negative", Contrastive(0.5, pr.make_pair_selector("hard_negative"))),
                           ("Contrastive all", Contrastive(0.5, pr.make_pair_selector("all")))):
            key = f"{name} B={B}"
            out[key] = measure(crit, x, lab, a.iters, stream)
            show(name, B, out[key])
    if a.trainer:
        runs = (("LMCL", None), ("ASoftmax", None), ("Triplet", None), ("OnlineContrastive", {"train.contrastive": {"selector": "hard_negative"}}),
                ("OnlineContrastive", {"train.contrastive": {"selector": "all"}}))
        for loss, extra in runs:
            key = "train_audio " + loss + ("" if not extra else " " + extra["train.contrastive"]["selector"])
            out[key] = trainer_step_ms(loss, extra)
            print(f"{key:40s} {out[key]['ms_per_step']:8.3f} ms per step ({out[key]['utt_per_s']:.0f} utt/s, {out[key]['step_mode']}, bs {out[key]['bs']})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
