#!/usr/bin/env python3
"""What waveform augmentation costs (EXPERIMENTS.md R6.28): needs an MI355X.

  (b) the FIR kernel alone -- dlip_wave_reverb_f32 without keep_power on 256 rows x 48 000 samples (a 3 s crop at 16 kHz) for room
      responses of 512, 2048 and 8192 taps, every row reverberated: device-event time per call, achieved FMA/s = rows * samples *
      taps over it, and that as a share of the fp32 vector peak (256 CUs x 4 SIMDs x 32 FMA/clk x 2.4 GHz = 78.6 T FMA/s).  Beside
      it, AS A YARDSTICK ONLY, the same convolution through torch.fft (rfft of rows and response at the next power of two above
      samples + taps, product, irfft) on the same GPU, and the largest difference between the two results.
  (a) train_audio.Trainer._train_epoch() at bs 256 on the shipped E-TDNN config in three settings -- the feature path, waveforms
      through the front-end (data.train_from_waves) and waveforms with the default augment section -- utt/s of the second epoch
      over a cache of pre-generated batches (train.data_cache: the synthetic source's numpy is not what is measured).

    python tools/probes/wave_augment_time.py [--steps 24] [--reps 20] [--skip-trainer]      -> one JSON line
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

PEAK_FMA = 256 * 4 * 32 * 2.4e9          # fp32 vector FMA/s (v_pk_fma_f32: 64 FLOP/clk/SIMD)


def _time(fn, reps):
    """Median device-event milliseconds of fn() over ``reps`` calls after 3 warm-up calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def fir_alone(reps, rows=256, samples=48000):
    from deeplip_amd import weightgen as wg
    from deeplip_amd.augment import WaveAugment
    x = torch.from_numpy(wg.gen("probe.wa.x", (rows, samples))).cuda()
    out = []
    for taps in (512, 2048, 8192):
        h = (0.05 * wg.gen(f"probe.wa.h{taps}", (taps,))).astype(np.float32)
        h[0] = 1.0
        aug = WaveAugment(rirs=[h], p_reverb=1.0, keep_power=False)
        ridx = torch.zeros(rows, dtype=torch.int32, device="cuda")
        y = aug(x, params={"rir_idx": ridx})
        med, lo, hi = _time(lambda: aug(x, params={"rir_idx": ridx}), reps)
        n = 1 << int(np.ceil(np.log2(samples + taps)))
        hd = torch.from_numpy(h).cuda()

        def fft_route():
            return torch.fft.irfft(torch.fft.rfft(x, n=n) * torch.fft.rfft(hd, n=n)[None, :], n=n)[:, :samples]
        yf = fft_route()
        diff = float((yf - y).abs().max() / y.abs().max())
        fmed, flo, fhi = _time(fft_route, reps)
        fma = rows * samples * taps
        out.append({"taps": taps, "fir_ms": round(med, 3), "fir_ms_min_max": [round(lo, 3), round(hi, 3)],
                    "fir_tfma_s": round(fma / (med * 1e-3) / 1e12, 2), "share_of_fp32_vector_peak": round(fma / (med * 1e-3) / PEAK_FMA, 3),
                    "torch_fft_ms": round(fmed, 3), "torch_fft_ms_min_max": [round(flo, 3), round(fhi, 3)], "fft_vs_fir_rel_diff": diff})
    return out


def trainer(steps):
    import train_audio
    settings = {"features": {}, "waves": {"data.train_from_waves": True},
                "waves+augment": {"data.train_from_waves": True,
                                  "data.augment": {"snr_levels": [-5, 0, 5, 10, 15, 20, 9999], "p_reverb": 0.25, "keep_power": True,
                                                   "normalize": False, "max_taps": 8192}}}
    out = {}
    for name, ov in settings.items():
        tr = train_audio.Trainer(overrides=dict({"train.bs": 256, "train.steps_per_epoch": steps, "train.data_cache": 4}, **ov))
        try:
            rates = []
            for epoch in (1, 2, 3):                  # epoch 1 fills the batch cache and records the steps
                tr.current_epoch = epoch
                tr._adjust_margin()
                tr._train_epoch()
                rates.append(round(tr.last_epoch_stats["utt_per_s"], 1))
            out[name] = {"utt_per_s_epochs": rates, "step_mode": tr.last_epoch_stats["step_mode"],
                         "ms_per_step": round(256e3 / rates[-1], 3)}
        finally:
            tr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-trainer", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("wave_augment_time.py measures on the GPU: no ROCm device found")
    from deeplip_amd import build
    res = {"box": build.box_id(), "fir_alone": fir_alone(a.reps)}
    if not a.skip_trainer:
        res["trainer_bs256_etdnn"] = trainer(a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
