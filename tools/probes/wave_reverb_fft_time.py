#!/usr/bin/env python3
"""What the two reverberation routes cost (EXPERIMENTS.md R15.1; the protocol of R10.1): needs an MI355X.

  (1) the reverberation alone, keep_power off, on 256 rows x 48 000 samples (a 3 s crop at 16 kHz), every row reverberated, in ONE
      process: the transform route (WaveAugment(reverb="fft"), dlip_wave_reverb_fft_f32) at 512, 2048, 8192, 16 384 and 65 536 taps;
      beside it the direct FIR kernel (reverb="fir", dlip_wave_reverb_f32) at the lengths it takes (512 .. 8192) and, AS A YARDSTICK
      ONLY, the same convolution through torch.fft (rfft at the next power of two above samples + taps, product, irfft).
      Device-event milliseconds per call: median of ``--reps`` after 3 warm-ups, with min and max; and the largest difference
      between the routes' results relative to the largest output.
  (2) train_audio.Trainer._train_epoch() at bs 256 on the shipped E-TDNN config from waveforms with the default augment section,
      ``reverb: fir`` against ``reverb: fft`` -- utt/s of the later epochs over a cache of pre-generated batches.

    python tools/probes/wave_reverb_fft_time.py [--steps 24] [--reps 20] [--skip-trainer]      -> one JSON line
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from wave_augment_time import _time      # noqa: E402  (the same clock as R10.1)

TAPS = (512, 2048, 8192, 16384, 65536)


def reverb_alone(reps, rows=256, samples=48000):
    from deeplip_amd import _lib, weightgen as wg
    from deeplip_amd.augment import WaveAugment
    x = torch.from_numpy(wg.gen("probe.wa.x", (rows, samples))).cuda()
    ridx = torch.zeros(rows, dtype=torch.int32, device="cuda")
    out = []
    for taps in TAPS:
        h = (0.05 * wg.gen(f"probe.wa.h{taps}", (taps,))).astype(np.float32)
        h[0] = 1.0
        row = {"taps": taps}
        fft = WaveAugment(rirs=[h], p_reverb=1.0, keep_power=False, reverb="fft")
        y = fft(x, params={"rir_idx": ridx})
        med, lo, hi = _time(lambda: fft(x, params={"rir_idx": ridx}), reps)
        row.update(fft_route_ms=round(med, 3), fft_route_ms_min_max=[round(lo, 3), round(hi, 3)])
        if taps <= _lib.DLIP_FIR_MAX_TAPS:
            fir = WaveAugment(rirs=[h], p_reverb=1.0, keep_power=False, reverb="fir")
            yd = fir(x, params={"rir_idx": ridx})
            med, lo, hi = _time(lambda: fir(x, params={"rir_idx": ridx}), reps)
            row.update(fir_ms=round(med, 3), fir_ms_min_max=[round(lo, 3), round(hi, 3)],
                       fft_route_vs_fir_rel_diff=float((y - yd).abs().max() / yd.abs().max()))
        n = 1 << int(np.ceil(np.log2(samples + taps)))
        hd = torch.from_numpy(h).cuda()

        def torch_fft():
            return torch.fft.irfft(torch.fft.rfft(x, n=n) * torch.fft.rfft(hd, n=n)[None, :], n=n)[:, :samples]
        yt = torch_fft()
        med, lo, hi = _time(torch_fft, reps)
        row.update(torch_fft_ms=round(med, 3), torch_fft_ms_min_max=[round(lo, 3), round(hi, 3)],
                   fft_route_vs_torch_fft_rel_diff=float((y - yt).abs().max() / yt.abs().max()))
        out.append(row)
    return out


def trainer(steps):
    import train_audio
    section = {"snr_levels": [-5, 0, 5, 10, 15, 20, 9999], "p_reverb": 0.25, "keep_power": True, "normalize": False}
    out = {}
    for route in ("fir", "fft"):
        ov = {"train.bs": 256, "train.steps_per_epoch": steps, "train.data_cache": 4, "data.train_from_waves": True,
              "data.augment": dict(section, reverb=route)}
        tr = train_audio.Trainer(overrides=ov)
        try:
            rates = []
            for epoch in (1, 2, 3):                  # epoch 1 fills the batch cache and records the steps
                tr.current_epoch = epoch
                tr._adjust_margin()
                tr._train_epoch()
                rates.append(round(tr.last_epoch_stats["utt_per_s"], 1))
            out[route] = {"utt_per_s_epochs": rates, "step_mode": tr.last_epoch_stats["step_mode"], "ms_per_step": round(256e3 / rates[-1], 3),
                          "longest_response_taps": int(tr._augment.rir.shape[1]), "truncated": list(tr._augment.truncated)}
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
        raise SystemExit("wave_reverb_fft_time.py measures on the GPU: no ROCm device found")
    from deeplip_amd import _lib, build
    res = {"box": build.box_id(), "ols_block": _lib.DLIP_OLS_BLOCK, "reverb_alone": reverb_alone(a.reps)}
    if not a.skip_trainer:
        res["trainer_bs256_etdnn_from_waves"] = trainer(a.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
