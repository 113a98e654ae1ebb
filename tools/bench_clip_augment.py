#!/usr/bin/env python3
"""Lip-clip augmentation on the device (deeplip_amd/clip_augment.py; EXPERIMENTS.md R24.1), microseconds per call:

  kernel         ClipAugment on 64 clips of 29 frames -- uint8 RGB 96 x 96 -> 88 (per-clip crop origins, flips, ragged lengths) and
                 the float source [64, 1, 29, 88, 88] -- with masks only (2 time masks, 2 cutouts; fill zero and fill mean) and with
                 everything on (mean fill + mixup)
  ingest         dlip_crop_normalize_u8 (VideoFrontend) on the same frames, clip_params and lengths: the launch the stage replaces
  torch          a plain-torch formulation of the same definition on the same tensors, from index vectors and masks ALREADY RESOLVED
                 on the host and resident on the device (the kernel resolves them from the draws itself): a yardstick, not a product path
  bytes          what the stage must move: per valid output pixel the source bytes of each operand it reads (3 for RGB, 4 for float; twice
                 with a partner; once more for the mean pass) and 4 written; per padded pixel 4 written.  Share = bytes / time over the HBM
                 peak (8.0 TB/s).  The tensors of one call (51 MB of frames, 57 MB of output) fit the 256 MiB Infinity Cache: the rates
                 are rates of a cache-resident working set, not of HBM alone

One process; every call is warmed `--warmup` times, then `--rounds` timed windows of `--calls` calls each alternate over the
measurements of a workload; each window lies between two HIP events on an idle device.  Medians over the windows.

  --trainer      also train_video.main() at batch 32 x 29 frames with and without the stage (masks; everything), --rgb and float: ms per
                 recorded step from the trainer's own clock, each variant run `--trainer-runs` times, variants alternating

    python tools/bench_clip_augment.py [--rounds 20] [--calls 10] [--warmup 5] [--trainer]

Prints one line per measurement and one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import clip_augment_ref as ref  # noqa: E402
from deeplip_amd.clip_augment import ClipAugment  # noqa: E402

HBM_PEAK = 8.0e12
B, T, S, CROP = 64, 29, 96, 88
MASKS = dict(time_masks=2, time_width=5, time_ratio=0.4, cutouts=2, cut_size=30)


def window(fn, calls) -> float:
    """Microseconds per call: `calls` calls between two HIP events, the device idle on both sides."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1)) * 1e3 / calls


def measure(runs, a):
    with torch.no_grad():
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(window(fn, a.calls))
    return {k: {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1), "max_us": round(float(np.max(v)), 1)}
            for k, v in t.items()}


def resolved(ca, draws, lens, cp, OH):
    """What the torch formulation starts from, on the device: source rows / columns per clip (the flip baked in), valid frames, the
    time-mask and cutout masks."""
    iy = np.zeros((B, OH), dtype=np.int64)
    ix = np.zeros((B, OH), dtype=np.int64)
    valid = np.arange(T)[None, :] < np.asarray(lens)[:, None]
    tm = np.zeros((B, T), dtype=bool)
    cm = np.zeros((B, OH, OH), dtype=bool)
    for b in range(B):
        row = [int(v) for v in draws[b]]
        if cp is not None:
            iy[b] = cp[b, 0] + np.arange(OH)
            ix[b] = cp[b, 1] + (np.arange(OH)[::-1] if cp[b, 2] else np.arange(OH))
        for t0, w in ref.time_masks(int(lens[b]), row, ca.time_masks, ca.time_width, ca.time_ratio):
            tm[b, t0:t0 + w] = True
        for y0, x0, h, w in ref.cutouts(OH, OH, row, ca.cutouts, ca.cut_size):
            cm[b, y0:y0 + h, x0:x0 + w] = True
    return [torch.from_numpy(v).cuda() for v in (iy, ix, valid, tm, cm)]


def torch_clip_augment(src, iy, ix, valid, tm, cm, count, mean_fill, perm, lam):
    if src.dtype == torch.uint8:
        bi = torch.arange(B, device=src.device)[:, None, None, None]
        ti = torch.arange(T, device=src.device)[None, :, None, None]
        r, g, b = (src[bi, ti, c, iy[:, None, :, None], ix[:, None, None, :]].float() for c in range(3))
        a = (((0.299 * r + 0.587 * g) + 0.114 * b) / 255.0 - 0.421) / 0.165
    else:
        a = src[:, 0]
    v = valid[:, :, None, None]
    a = torch.where(v, a, 0.0)
    f = (a.double().sum(dim=(1, 2, 3)) / count).float()[:, None, None, None] if mean_fill else 0.0
    a = torch.where((tm[:, :, None, None] | cm[:, None]) & v, f, a)
    if perm is not None:
        a = torch.where(v, lam * a + (1.0 - lam) * a[perm], 0.0)
    return a[:, None]


def stage_bytes(lens, OH, src_bytes, partners, mean_fill):
    """Bytes the stage must move (see the module docstring); `partners`: frames in which a row reads a partner's pixels."""
    px = OH * OH
    own = int(np.sum(lens)) * px
    return own * src_bytes * (2 if mean_fill else 1) + partners * px * src_bytes + B * T * px * 4


def trainer_steps(runs):
    """train_video.main at batch 32 x 29 frames, 40 steps over a cache of 4 batches: ms per step (the trainer's clock, from the 4th step
    on: recorded steps) with and without the stage."""
    import tempfile
    import train_video
    aug = ["--time-masks", "2", "--time-mask-width", "5", "--time-mask-ratio", "0.4", "--cutouts", "2", "--cutout-size", "30"]
    variants = {"none": [], "masks": aug, "masks + mixup": aug + ["--mixup-alpha", "0.4"]}
    res = {}
    for src, extra in (("rgb", ["--rgb"]), ("float", [])):
        out = {k: [] for k in variants}
        for _ in range(runs):
            for k, flags in variants.items():
                train_video.main(["--save-path", tempfile.mkdtemp(), "--batch-size", "32", "--frames", "29", "--steps", "40", "--data-cache", "4",
                                  "--display", "1000"] + extra + flags)
                st = train_video.train.last_stats
                assert st["step_mode"] == "graph", st
                out[k].append(round(st["ms_per_step"], 3))
        for k, v in out.items():
            res[f"{src}, {k}"] = {"ms_per_step": v, "median": round(float(np.median(v)), 3)}
            print(f"train_video 32 x 29 {src}, {k}: ms per step {v}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer", action="store_true", help="also time train_video's step with and without the stage")
    ap.add_argument("--trainer-runs", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20271)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_augment: no GPU")
    r = np.random.Generator(np.random.PCG64(a.seed))
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_window": a.calls, "warmup": a.warmup, "workloads": {}}
    lens = np.concatenate([[T], r.integers(T // 3, T + 1, size=B - 1)]).astype(np.int32)
    cp = np.stack([r.integers(0, S - CROP + 1, size=B), r.integers(0, S - CROP + 1, size=B), r.integers(0, 2, size=B), np.zeros(B)], 1).astype(np.int32)
    frames = torch.from_numpy(r.integers(0, 256, size=(B, T, 3, S, S), dtype=np.int64).astype(np.uint8)).cuda()
    clip = torch.from_numpy(r.standard_normal((B, 1, T, CROP, CROP)).astype(np.float32)).cuda()
    lens_d, cp_d = torch.from_numpy(lens).cuda(), torch.from_numpy(cp).cuda()
    from deeplip_amd.frontend import VideoFrontend
    vf = VideoFrontend(CROP)
    slower = []
    for src_name, src, cps, src_bytes in (("rgb 96 -> 88", frames, cp, 3), ("float 88", clip, None, 4)):
        res = {}
        for name, kw in (("masks, fill zero", dict(MASKS, fill="zero")), ("masks, fill mean", dict(MASKS, fill="mean")),
                         ("masks, fill mean, mixup", dict(MASKS, fill="mean", mixup_alpha=0.4))):
            ca = ClipAugment(**kw)
            host = ca.draw(B, r)
            p = ca.to_device(host, "cuda")
            perm = host.get("perm")
            partners = 0 if perm is None else int(sum(min(lens[b], lens[perm[b]]) for b in range(B) if perm[b] != b))
            nbytes = stage_bytes(lens, CROP, src_bytes, partners, ca.fill == "mean")
            call = (lambda ca=ca, p=p: ca(src, clip_params=cp_d, lengths=lens_d, params=p)) if cps is not None else \
                (lambda ca=ca, p=p: ca(src, lengths=lens_d, params=p))
            pre = resolved(ca, host["draws"], lens, cps, CROP)
            count = torch.from_numpy(lens.astype(np.float64) * CROP * CROP).cuda()
            targs = (src, *pre, count, ca.fill == "mean", None if perm is None else torch.from_numpy(perm).long().cuda(),
                     None if perm is None else float(host["lam"][0]))
            err = float((call() - torch_clip_augment(*targs)).abs().max())
            assert err < 1e-5, (src_name, name, err)                # the yardstick computes the same thing
            runs = {"kernel": call, "torch": lambda targs=targs: torch_clip_augment(*targs)}
            if cps is not None and name == "masks, fill zero":
                runs["ingest"] = lambda: vf(frames, clip_params=cp_d, lengths=lens_d)
            m = measure(runs, a)
            k_s = m["kernel"]["median_us"] * 1e-6
            m.update(bytes=nbytes, hbm_floor_us=round(nbytes / HBM_PEAK * 1e6, 1), kernel_GBps=round(nbytes / k_s / 1e9, 1),
                     kernel_share_of_hbm_peak=round(nbytes / k_s / HBM_PEAK, 4), torch_over_kernel=round(m["torch"]["median_us"] / m["kernel"]["median_us"], 2))
            if m["torch_over_kernel"] < 1.0:
                slower.append((src_name, name))
            res[name] = m
            print(f"[{src_name}] {name:26s} kernel {m['kernel']['median_us']:8.1f} us ({nbytes / 1e6:.1f} MB, hbm floor {m['hbm_floor_us']} us, "
                  f"{m['kernel_GBps']} GB/s)   torch {m['torch']['median_us']:8.1f} us"
                  + (f"   ingest {m['ingest']['median_us']:8.1f} us" if "ingest" in m else ""), flush=True)
        out["workloads"][src_name] = res
    out["kernel_slower_than_torch_at"] = slower
    if a.trainer:
        out["train_video"] = trainer_steps(a.trainer_runs)
    print(json.dumps(out))
    if slower:
        raise SystemExit(f"bench_clip_augment: the kernel is slower than the torch formulation at {slower}")


if __name__ == "__main__":
    main()
