#!/usr/bin/env python3
"""Waveform resampling on the device (deeplip_amd/resample.py; EXPERIMENTS.md R13.1), microseconds per call:

  kernel         dlip_wave_resample_f32 through Resample / SpeedPerturb on
                   256 x 48 000 samples at 10/9, at 10/11 and as a mixed bank (speeds 0.9 / 1.0 / 1.1 drawn per row),
                   256 x 144 000 samples at 1/3 (48 kHz -> 16 kHz),  64 x 132 300 samples at 160/441 (44.1 kHz -> 16 kHz)
  hbm floor      the bytes the kernel must move (every input sample read once, every output written once) over the HBM peak (8.0 TB/s)
  fma floor      its fmaf count (outputs x K taps per phase) over the fp32 vector peak (157.3 TFLOP/s = 78.6e12 fmaf/s)
  torch          a polyphase formulation in torch on the device, one strided conv1d per output phase -- a yardstick, not a product
                 path; ratios with up > --yardstick-max-up are skipped (one conv1d launch per phase: 160 of them at 160/441)
  in context     the stage in front of the front-end: SpeedPerturb + AudioFrontend("mfcc") against the front-end alone on a training
                 batch of 64 crops, and Resample(48 kHz -> 16 kHz) + front-end against the front-end alone on an extraction batch

One process; every call is warmed `--warmup` times, then `--rounds` timed windows of `--calls` calls each alternate over the
measurements of a workload; each window lies between two HIP events on an idle device.  Medians over the windows.

  --trainer      also train_audio.Trainer._train_epoch() from waveforms at bs 256, one crop length, with and without
                 data.speed_perturb: two trainers whose epochs alternate, utt/s of epochs 2 and 3

    python tools/bench_resample.py [--rounds 20] [--calls 10] [--warmup 5] [--yardstick-max-up 10] [--trainer]

Prints one line per measurement and one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeplip_amd.frontend import AudioFrontend  # noqa: E402
from deeplip_amd.resample import Resample, SpeedPerturb, design, out_len, pack_table  # noqa: E402

HBM_PEAK = 8.0e12
FMA_PEAK = 157.3e12 / 2


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


def torch_polyphase(x, up, down, h):
    """y = resample of x [B, S] in torch: outputs m = m_r + k up share the phase of m_r and step `down` through the input -- one
    conv1d of stride `down` per m_r < up, interleaved into y."""
    B, S = x.shape
    tab, K = pack_table(h, up)
    c = (len(h) - 1) // 2
    n_out = out_len(S, up, down)
    xp = torch.nn.functional.pad(x, (K - 1, K + down))[:, None, :]
    y = torch.empty((B, n_out), device=x.device)
    w = torch.from_numpy(np.ascontiguousarray(tab[:, :K][:, ::-1])).to(x.device)         # cross-correlation: taps reversed
    for m_r in range(min(up, n_out)):
        q = c + m_r * down
        cnt = (n_out - m_r + up - 1) // up
        seg = xp[:, :, q // up: q // up + (cnt - 1) * down + K]
        y[:, m_r::up] = torch.nn.functional.conv1d(seg, w[q % up][None, None, :], stride=down)[:, 0, :cnt]
    return y


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


def trainer_epochs(bs, steps, epochs):
    """train_audio.Trainer._train_epoch() from waveforms at one crop length (300 frames), with and without data.speed_perturb: two
    trainers in one process, their epochs ALTERNATING (a drift of the box hits both), over a cache of 4 pre-generated batches (the
    synthetic source's numpy is not what is measured).  utt/s per epoch; epoch 1 generates the batches and records the step."""
    import tempfile
    os.chdir(tempfile.mkdtemp())                                  # the trainers' run directory
    import train_audio
    base = {"train.bs": bs, "train.steps_per_epoch": steps, "train.data_cache": 4, "train.crop_frames": [300, 300], "data.train_from_waves": True}
    settings = {"from waves": {}, "from waves + speed_perturb": {"data.speed_perturb": {"speeds": [0.9, 1.0, 1.1]}}}
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
    res = {k: {"utt_per_s": v, "ms_per_step": round(1e3 * bs / float(np.median(v[1:])), 3)} for k, v in out.items()}
    for k, v in res.items():
        print(f"train_audio bs {bs}, {k}: utt/s per epoch {v['utt_per_s']}, {v['ms_per_step']} ms per step (epochs 2 ..)", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trainer", action="store_true", help="also time train_audio's from-waves step with and without data.speed_perturb")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--yardstick-max-up", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20263)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: no GPU")
    r = np.random.Generator(np.random.PCG64(a.seed))
    out = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "calls_per_window": a.calls, "warmup": a.warmup, "workloads": {}}

    def wave(B, S):
        return torch.from_numpy((0.1 * r.standard_normal((B, S))).astype(np.float32)).cuda()

    for name, B, S, up, down in (("10/9", 256, 48000, 10, 9), ("10/11", 256, 48000, 10, 11), ("1/3", 256, 144000, 1, 3),
                                 ("160/441", 64, 132300, 160, 441)):
        x = wave(B, S)
        rs = Resample(down, up)
        runs = {"kernel": lambda: rs(x)}
        if up <= a.yardstick_max_up:
            got, want = rs(x)[0], torch_polyphase(x, up, down, rs.h)
            err = float((got - want).abs().max())
            assert err < 1e-4, (name, err)                       # the yardstick computes the same thing
            runs["torch"] = lambda: torch_polyphase(x, up, down, rs.h)
        res = measure(runs, a)
        n_out, K = out_len(S, up, down), -(-rs.h.size // up)
        nbytes, fmas = 4 * B * (S + n_out), B * n_out * K
        k_s = res["kernel"]["median_us"] * 1e-6
        res.update(shape=[B, S], out_samples=n_out, taps_per_output=K, tile=rs.tile, bytes=nbytes, fmaf=fmas,
                   hbm_floor_us=round(nbytes / HBM_PEAK * 1e6, 1), fma_floor_us=round(fmas / FMA_PEAK * 1e6, 1),
                   kernel_GBps=round(nbytes / k_s / 1e9, 1), kernel_share_of_hbm_peak=round(nbytes / k_s / HBM_PEAK, 4),
                   kernel_Gfmaps=round(fmas / k_s / 1e9, 1))
        if "torch" in res:
            res["torch_over_kernel"] = round(res["torch"]["median_us"] / res["kernel"]["median_us"], 2)
        out["workloads"][name] = res
        print(f"{name:8s} [{B} x {S}] kernel {res['kernel']['median_us']:9.1f} us (hbm floor {res['hbm_floor_us']}, fma floor "
              f"{res['fma_floor_us']}; {res['kernel_GBps']} GB/s)" + (f"   torch {res['torch']['median_us']:9.1f} us" if "torch" in res else ""),
              flush=True)

    # the mixed bank: speeds drawn per row, every row cut to the input's width
    x = wave(256, 48000)
    sp = SpeedPerturb((0.9, 1.0, 1.1))
    idx = torch.from_numpy(sp.draw(256, r)["speed_idx"]).cuda()
    res = measure({"kernel": lambda: sp(x, params={"speed_idx": idx}, out_samples=48000)}, a)
    out["workloads"]["mixed 0.9/1.0/1.1"] = dict(res, shape=[256, 48000], out_samples=48000)
    print(f"mixed    [256 x 48000] kernel {res['kernel']['median_us']:9.1f} us", flush=True)

    # in context: in front of the MFCC front-end
    fe = AudioFrontend("mfcc")
    Sb = fe.samples_for_frames(300)                                # a 300-frame crop, the middle of the trainers' 200 .. 400
    xin = wave(64, sp.in_samples(Sb))
    xb = xin[:, :Sb].contiguous()
    idx = torch.from_numpy(sp.draw(64, r)["speed_idx"]).cuda()
    res = measure({"frontend": lambda: fe(xb), "speed + frontend": lambda: fe(sp(xin, params={"speed_idx": idx}, out_samples=Sb)[0])}, a)
    res["stage_share"] = round(1.0 - res["frontend"]["median_us"] / res["speed + frontend"]["median_us"], 3)
    out["train_step_features"] = dict(res, shape=[64, Sb])
    rs = Resample(48000, 16000)
    S16 = fe.samples_for_frames(400)
    x48 = wave(64, 3 * S16)
    lens48 = torch.from_numpy(r.integers(3 * S16 // 2, 3 * S16 + 1, size=64).astype(np.int32)).cuda()
    x16, lens16 = rs(x48, lens48)
    res = measure({"frontend": lambda: fe(x16, lens16), "resample + frontend": lambda: fe(*rs(x48, lens48))}, a)
    res["stage_share"] = round(1.0 - res["frontend"]["median_us"] / res["resample + frontend"]["median_us"], 3)
    out["extraction_features"] = dict(res, shape=[64, 3 * S16])
    for k in ("train_step_features", "extraction_features"):
        print(f"{k}: " + ", ".join(f"{n} {v['median_us']} us" for n, v in out[k].items() if isinstance(v, dict)) +
              f"; the stage's share {out[k]['stage_share']}", flush=True)
    if a.trainer:
        out["train_audio"] = trainer_epochs(256, 24, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
