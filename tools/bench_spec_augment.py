#!/usr/bin/env python3
"""SpecAugment on the device (deeplip_amd/spec_augment.py; EXPERIMENTS.md R19.1), microseconds per call:

  kernel         dlip_spec_augment_f32 through SpecAugment on [256, 24, 300] (MFCC crops), [256, 80, 3000] (fbank utterances) and
                 [64, 257, 302] (stft crops; 302 frames: no row is 16-byte aligned), masks only (2 + 2, fill zero) and with the warp
                 (W = 5) in front of them; `mean fill` adds the row-mean launch
  hbm floor      one read and one write of the tensor over the HBM peak (8.0 TB/s)
  torch          a plain-torch formulation on the same tensors: arange comparisons + where for the masks, a gather + lerp for the warp,
                 from the mask bounds and the per-frame (index, fraction) ALREADY RESOLVED on the host and resident on the device (the
                 kernel resolves them from the draws itself) -- a yardstick, not a product path: no such stage existed before

One process; every call is warmed `--warmup` times, then `--rounds` timed windows of `--calls` calls each alternate over the
measurements of a workload; each window lies between two HIP events on an idle device.  Medians over the windows.

  --trainer      also train_audio.Trainer._train_epoch() at bs 256, one crop length, with and without data.spec_augment, on the
                 feature-fed path and from waves: per path two trainers whose epochs alternate, utt/s of epochs 2 and 3

    python tools/bench_spec_augment.py [--rounds 20] [--calls 10] [--warmup 5] [--trainer]

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

import spec_augment_ref as ref  # noqa: E402
from deeplip_amd.spec_augment import SpecAugment  # noqa: E402

HBM_PEAK = 8.0e12
SHAPES = ((256, 24, 300), (256, 80, 3000), (64, 257, 302))
MASKS = dict(freq_masks=2, freq_width=4, time_masks=2, time_width=20, time_ratio=0.2)
SECTION = dict(MASKS, time_warp=5, fill="zero")


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


def resolved(sa, draws, B, C, NF):
    """What the torch formulation starts from, on the device: mask bounds [B, n] per axis and the warp's (index, fraction) [B, NF]."""
    f0, f1, t0, t1 = (np.zeros((B, max(n, 1)), dtype=np.int64) for n in (sa.freq_masks, sa.freq_masks, sa.time_masks, sa.time_masks))
    idx = np.tile(np.minimum(np.arange(NF), NF - 2), (B, 1))
    frac = np.tile((np.arange(NF) == NF - 1).astype(np.float32), (B, 1))
    for b in range(B):
        row = [int(v) for v in draws[b]]
        for j, (s, w) in enumerate(ref.freq_masks(C, row, sa.freq_masks, sa.freq_width)):
            f0[b, j], f1[b, j] = s, s + w
        for j, (s, w) in enumerate(ref.time_masks(NF, row, sa.time_masks, sa.time_width, sa.time_ratio)):
            t0[b, j], t1[b, j] = s, s + w
        wp = ref.warp_params(NF, sa.time_warp, row[0], row[1])
        if wp is not None and wp[0] != wp[1]:
            s = ref.warp_positions(NF, *wp)
            idx[b] = np.minimum(np.floor(s).astype(np.int64), NF - 2)
            frac[b] = (s - idx[b]).astype(np.float32)
    return [torch.from_numpy(v).cuda() for v in (f0, f1, t0, t1, idx, frac)]


def torch_spec_augment(x, f0, f1, t0, t1, idx, frac, warp):
    B, C, NF = x.shape
    if warp:
        i = idx[:, None, :].expand(B, C, NF)
        x = torch.lerp(torch.gather(x, 2, i), torch.gather(x, 2, i + 1), frac[:, None, :])
    af, at = torch.arange(C, device=x.device), torch.arange(NF, device=x.device)
    fm = ((af[None, None, :] >= f0[:, :, None]) & (af[None, None, :] < f1[:, :, None])).any(dim=1)
    tm = ((at[None, None, :] >= t0[:, :, None]) & (at[None, None, :] < t1[:, :, None])).any(dim=1)
    return torch.where(fm[:, :, None] | tm[:, None, :], 0.0, x)


def trainer_epochs(bs, steps, epochs):
    """train_audio.Trainer._train_epoch() at one crop length (300 frames), with and without data.spec_augment, on the feature-fed path
    and from waves: per path two trainers in one process, their epochs ALTERNATING (a drift of the box hits both), over a cache of 4
    pre-generated batches.  utt/s per epoch; epoch 1 generates the batches and records the step."""
    import tempfile
    os.chdir(tempfile.mkdtemp())                                  # the trainers' run directory
    import train_audio
    base = {"train.bs": bs, "train.steps_per_epoch": steps, "train.data_cache": 4, "train.crop_frames": [300, 300]}
    res = {}
    for path, extra in (("features", {}), ("from waves", {"data.train_from_waves": True})):
        settings = {path: extra, path + " + spec_augment": dict(extra, **{"data.spec_augment": dict(SECTION)})}
        trainers = {k: train_audio.Trainer("conf/audio_config.yaml", overrides=dict(base, **v)) for k, v in settings.items()}
        out = {k: [] for k in settings}
        for epoch in range(1, epochs + 1):
            for k, tr in trainers.items():
                tr.current_epoch = epoch
                tr._adjust_margin()
                tr._train_epoch()
                out[k].append(round(tr.last_epoch_stats["utt_per_s"], 1))
        for tr in trainers.values():
            tr.close()
        for k, v in out.items():
            res[k] = {"utt_per_s": v, "ms_per_step": round(1e3 * bs / float(np.median(v[1:])), 3)}
            print(f"train_audio bs {bs}, {k}: utt/s per epoch {v}, {res[k]['ms_per_step']} ms per step (epochs 2 ..)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer", action="store_true", help="also time train_audio's step with and without data.spec_augment, both paths")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20264)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spec_augment: no GPU")
    r = np.random.Generator(np.random.PCG64(a.seed))
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_window": a.calls, "warmup": a.warmup, "workloads": {}}
    slower = []
    for B, C, NF in SHAPES:
        x = torch.from_numpy(r.standard_normal((B, C, NF)).astype(np.float32)).cuda()
        nbytes = 2 * 4 * B * C * NF
        res = {"shape": [B, C, NF], "bytes": nbytes, "hbm_floor_us": round(nbytes / HBM_PEAK * 1e6, 1)}
        for name, kw in (("masks", dict(MASKS)), ("warp + masks", dict(MASKS, time_warp=5)), ("masks, mean fill", dict(MASKS, fill="mean"))):
            sa = SpecAugment(**kw)
            draws = sa.draw(B, r)["draws"]
            p = {"draws": torch.from_numpy(draws).cuda()}
            runs = {"kernel": lambda: sa(x, params=p)}
            if sa.fill == "zero":
                pre = resolved(sa, draws, B, C, NF)
                got, want = sa(x, params=p), torch_spec_augment(x, *pre, sa.time_warp > 0)
                err = float((got - want).abs().max())
                assert err < 1e-5, (name, err)                     # the yardstick computes the same thing
                runs["torch"] = lambda: torch_spec_augment(x, *pre, sa.time_warp > 0)
            m = measure(runs, a)
            k_s = m["kernel"]["median_us"] * 1e-6
            m.update(kernel_GBps=round(nbytes / k_s / 1e9, 1), kernel_share_of_hbm_peak=round(nbytes / k_s / HBM_PEAK, 4))
            if "torch" in m:
                m["torch_over_kernel"] = round(m["torch"]["median_us"] / m["kernel"]["median_us"], 2)
                if m["torch_over_kernel"] < 1.0:
                    slower.append((B, C, NF, name))
            res[name] = m
            print(f"[{B}, {C}, {NF}] {name:18s} kernel {m['kernel']['median_us']:8.1f} us (hbm floor {res['hbm_floor_us']}; "
                  f"{m['kernel_GBps']} GB/s)" + (f"   torch {m['torch']['median_us']:8.1f} us" if "torch" in m else ""), flush=True)
        out["workloads"][f"{B}x{C}x{NF}"] = res
    out["kernel_slower_than_torch_at"] = slower
    if a.trainer:
        out["train_audio"] = trainer_epochs(256, 24, 3)
    print(json.dumps(out))
    if slower:
        raise SystemExit(f"bench_spec_augment: the kernel is slower than the torch formulation at {slower}")


if __name__ == "__main__":
    main()
