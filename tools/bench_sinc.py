#!/usr/bin/env python3
"""The sinc filter bank of `arch: sincnet` (deeplip_amd/sincnet.py; EXPERIMENTS.md R23.1), milliseconds per call:

  kernel         SincConv.features on wave [B, S] (256 x 48 000 by default), F = 24 filters, L = 31 / 251 / 1023 taps: forward
                 (dlip_sinc_taps_f32 + dlip_sinc_features_f32) and backward (dlip_sinc_features_bwd_f32 + dlip_sinc_taps_bwd_f32)
  torch          a plain-torch formulation of the same definition on the same tensors (tests/sinc_ref.py's features_conv1d in fp32:
                 conv1d, square, unfold-framing, log; autograd for the backward) -- the yardstick, not the code under test
  share of peak  the FOLDED multiply-add count -- (L + 1) / 2 per filter and position, once forward, twice backward (z recomputed, the
                 tap gradient accumulated) -- over the fp32 peak of 157.3 TFLOP/s
  peak memory    the rise of torch.cuda.max_memory_allocated across one forward + backward of each formulation

One process; every call is warmed, then `--rounds` timed windows of `--calls` calls each ALTERNATE between the two formulations; each
window lies between two HIP events on an idle device.  Medians over the windows.

  --trainer      also train_audio.Trainer._train_epoch() at bs 256, 300 frames: `arch: sincnet` beside `arch: tdnn` from waves with
                 mfcc (two trainers whose epochs alternate, utt/s of epochs 2 ..)

    python tools/bench_sinc.py [--batch 256] [--samples 48000] [--rounds 5] [--calls 2] [--trainer]

Prints one line per measurement and one JSON line; says so where the kernel is slower than the torch formulation."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sinc_ref as ref  # noqa: E402
from deeplip_amd.sincnet import SincConv  # noqa: E402

FP32_PEAK = 157.3e12
TAPS = (31, 251, 1023)


def window(fn, calls) -> float:
    """Milliseconds per call: `calls` calls between two HIP events, the device idle on both sides."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1)) / calls


def peak_rise(fn) -> int:
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def trainer_epochs(bs, steps, epochs):
    """train_audio.Trainer._train_epoch() at one crop length (300 frames) from waves: `arch: sincnet` (the layer inside the recorded step)
    beside `arch: tdnn` with the mfcc front-end in front of the step; two trainers in one process, their epochs alternating, over a
    cache of 4 pre-generated batches.  Epoch 1 generates the batches and records the step."""
    import tempfile
    os.chdir(tempfile.mkdtemp())
    import train_audio
    base = {"train.bs": bs, "train.steps_per_epoch": steps, "train.data_cache": 4, "train.crop_frames": [300, 300], "data.train_from_waves": True}
    settings = {"sincnet": dict(base, **{"model.arch": "sincnet"}), "tdnn + mfcc": dict(base, **{"model.arch": "tdnn"})}
    trainers = {k: train_audio.Trainer("conf/audio_config.yaml", overrides=v) for k, v in settings.items()}
    out = {k: [] for k in settings}
    for epoch in range(1, epochs + 1):
        for k, tr in trainers.items():
            tr.current_epoch = epoch
            tr._adjust_margin()
            tr._train_epoch()
            out[k].append(round(tr.last_epoch_stats["utt_per_s"], 1))
    res = {}
    for k, tr in trainers.items():
        res[k] = {"utt_per_s": out[k], "ms_per_step": round(1e3 * bs / float(np.median(out[k][1:])), 3), "step_mode": tr.last_epoch_stats["step_mode"]}
        print(f"train_audio bs {bs}, {k}: utt/s per epoch {out[k]}, {res[k]['ms_per_step']} ms per step (epochs 2 ..)", flush=True)
        tr.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--filters", type=int, default=24)
    ap.add_argument("--taps", type=int, nargs="+", default=list(TAPS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--trainer", action="store_true", help="also time train_audio's recorded step: arch sincnet beside tdnn + mfcc from waves")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinc: no GPU")
    B, S, F_ = a.batch, a.samples, a.filters
    x = ref.white_noise(B, S, seed=1).float().cuda()
    out = {"device": torch.cuda.get_device_name(0), "shape": [B, S, F_], "rounds": a.rounds, "calls_per_window": a.calls, "workloads": {}}
    slower = []
    for L in a.taps:
        sinc = SincConv(F_, kernel_size=L).cuda()
        flen, step = sinc.frame_len, sinc.frame_step
        low = sinc.low_hz_.detach().clone().requires_grad_()
        band = sinc.band_hz_.detach().clone().requires_grad_()

        def k_fwd():
            return sinc.features(x, None)[0]

        def t_fwd():
            g = ref.taps(low.double(), band.double(), L, sinc.rate, sinc.min_low_hz, sinc.min_band_hz).float()
            return ref.features_conv1d(x, g, flen, step, sinc.eps)

        yk, yt = k_fwd(), t_fwd()
        dy = torch.randn_like(yk)
        err = float((yk - yt).abs().max() / yt.abs().max())
        assert err < 1e-4, (L, err)                                   # the yardstick computes the same thing (both in fp32)
        runs = {"kernel fwd": lambda: k_fwd(), "torch fwd": lambda: t_fwd(),
                "kernel fwd+bwd": lambda: k_fwd().backward(dy), "torch fwd+bwd": lambda: t_fwd().backward(dy)}
        mem = {"kernel": peak_rise(runs["kernel fwd+bwd"]), "torch": peak_rise(runs["torch fwd+bwd"])}
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(window(fn, a.calls))
        med = {k: float(np.median(v)) for k, v in t.items()}
        folded = 2.0 * B * S * F_ * (L + 1) / 2                      # FLOP of the folded forward
        res = {"taps": L, "ms": {k: round(v, 3) for k, v in med.items()},
               "kernel_bwd_ms": round(med["kernel fwd+bwd"] - med["kernel fwd"], 3), "torch_bwd_ms": round(med["torch fwd+bwd"] - med["torch fwd"], 3),
               "fwd_share_of_fp32_peak": round(folded / (med["kernel fwd"] * 1e-3) / FP32_PEAK, 4),
               "bwd_share_of_fp32_peak": round(2 * folded / (max(med["kernel fwd+bwd"] - med["kernel fwd"], 1e-9) * 1e-3) / FP32_PEAK, 4),
               "peak_bytes": mem, "torch_over_kernel_fwd": round(med["torch fwd"] / med["kernel fwd"], 2),
               "torch_over_kernel_fwd_bwd": round(med["torch fwd+bwd"] / med["kernel fwd+bwd"], 2), "max_rel_diff_vs_torch": err}
        if res["torch_over_kernel_fwd"] < 1.0:
            slower.append((L, "forward"))
        if res["torch_over_kernel_fwd_bwd"] < 1.0:
            slower.append((L, "forward + backward"))
        out["workloads"][f"L{L}"] = res
        print(f"L {L:5d}: kernel fwd {med['kernel fwd']:8.3f} ms ({res['fwd_share_of_fp32_peak']:.3f} of the fp32 peak), bwd "
              f"{res['kernel_bwd_ms']:8.3f} ms ({res['bwd_share_of_fp32_peak']:.3f});  torch fwd {med['torch fwd']:8.3f} ms, bwd "
              f"{res['torch_bwd_ms']:8.3f} ms;  peak bytes kernel {mem['kernel']:,} torch {mem['torch']:,}", flush=True)
        del sinc, yk, yt, dy
        torch.cuda.empty_cache()
    out["kernel_slower_than_torch_at"] = slower
    if slower:
        print(f"the kernel is slower than the torch formulation at {slower}", flush=True)
    if a.trainer:
        out["train_audio"] = trainer_epochs(256, 12, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
