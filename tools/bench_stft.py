#!/usr/bin/env python3
"""The `stft` front-end (log-magnitude spectrograms) on [256, 48000] waveforms at (n_fft 512, hop 160,
window 400), in microseconds per call:

  stft rect      AudioFrontend("stft")(wave): spectrogram kernel + CMVN
  stft ragged    the same with a device length vector (rows of 24000 .. 48000 samples): + the frame-length kernel
  stft kernel    dlip_stft_logmag_wave_f32 alone: its share of the rectangular call, and its output bytes per second against the
                 HBM peak (8.0 TB/s; the kernel writes 301 x 260 floats per row and reads 48000)
  logfbank-60    AudioFrontend("logfbank", num_bin=60)(wave): the yardstick -- the same FFT size, plus a mel GEMM the spectrogram
                 does not have, writing 60 bands per frame where the spectrogram writes 257 bins

One process; every call is warmed `--warmup` times, then `--rounds` timed windows of `--calls` calls each ALTERNATE over the four
(the host is shared: a drift hits all of them); each window lies between two HIP events on an idle device.  Medians over the windows.

    python tools/bench_stft.py [--rows 256] [--samples 48000] [--rounds 20] [--calls 10] [--warmup 5]

Prints one line per measurement and one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeplip_amd import ops  # noqa: E402
from deeplip_amd._lib import call  # noqa: E402
from deeplip_amd.frontend import AudioFrontend  # noqa: E402

HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stft: no GPU")
    B, S = a.rows, a.samples
    r = np.random.Generator(np.random.PCG64(a.seed))
    x = torch.from_numpy((0.1 * r.standard_normal((B, S))).astype(np.float32)).cuda()
    lens = torch.from_numpy(r.integers(S // 2, S + 1, size=B).astype(np.int32)).cuda()
    fe = AudioFrontend("stft")                                     # 16 kHz: hop 160, window 400, n_fft 512 -> 257 bins
    mel = AudioFrontend("logfbank", num_bin=60)
    NF = fe.frames_for_samples(S)
    rows = ops._empty((B * NF, fe.nbp), x.device)

    def kernel():
        call("dlip_stft_logmag_wave_f32", x, rows, B, S, NF, fe.win_length, fe.hop, fe.nfft, fe.nb, fe.nbp)

    runs = {"stft rect": lambda: fe(x), "stft ragged": lambda: fe(x, lens), "stft kernel": kernel, "logfbank-60": lambda: mel(x)}
    with torch.no_grad():
        for fn in runs.values():
            for _ in range(a.warmup):
                fn()
        t = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(window(fn, a.calls))
    out = {"device": torch.cuda.get_device_name(0), "shape": [B, S], "geometry": [fe.nfft, fe.hop, fe.win_length], "frames": NF,
           "rounds": a.rounds, "calls_per_window": a.calls, "warmup": a.warmup}
    for k, v in t.items():
        out[k] = {"median_us": round(float(np.median(v)), 1), "min_us": round(float(np.min(v)), 1), "max_us": round(float(np.max(v)), 1)}
        print(f"{k:12s} median {out[k]['median_us']:10.1f} us   min {out[k]['min_us']:10.1f}   max {out[k]['max_us']:10.1f}", flush=True)
    k_s = out["stft kernel"]["median_us"] * 1e-6
    out_bytes, in_bytes = B * NF * fe.nbp * 4, B * S * 4
    out["kernel_share_of_rect"] = round(out["stft kernel"]["median_us"] / out["stft rect"]["median_us"], 3)
    out["kernel_output_bytes"] = out_bytes
    out["kernel_output_GBps"] = round(out_bytes / k_s / 1e9, 1)
    out["kernel_output_share_of_hbm_peak"] = round(out_bytes / k_s / HBM_PEAK, 4)
    out["kernel_input_GBps"] = round(in_bytes / k_s / 1e9, 1)
    out["stft_rect_over_logfbank60"] = round(out["stft rect"]["median_us"] / out["logfbank-60"]["median_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
