#!/usr/bin/env python3
"""What sliding-window CMN + VAD frame selection costs (EXPERIMENTS.md R12.1): needs an MI355X.

On 256 rows x 24 features x 3000 frames (30 s utterances, ragged lengths 1500 .. 3000), window 300 centred, the recipe's VAD:

  (a) the stage -- deeplip_amd.voiced_frames.VoicedFrames (dlip_vad_energy_select_i32 + dlip_cmn_sliding_select_f32): device-event
      time per eager call and per replay of a recorded plan (how extraction runs it: no host between the launches), the bytes the algorithm reads and writes over it (x's valid frames once, y once, the energy row, pos written and
      read once) and that rate as a share of the HBM rate.  The calls rotate over four input / output sets (0.6 GB together) so
      that the 256 MiB Infinity Cache does not serve the reads;
  (b) AS A YARDSTICK ONLY, never a product path: the same computation composed from torch ops on the same GPU -- fp64 cumsum,
      window differences by gather, the vote by cumsum of the decisions -- with the compaction done two ways: per-row boolean
      indexing (a host round trip per row) and one scatter over the batch; and the largest difference between its result and (a)'s;
  (c) the stage beside the step it sits in: front-end (MFCC-24, fft64) -> stage -> E-TDNN extraction on the same batch of waveforms,
      each part timed alone and the step as a whole.  At --step-rows rows (default 64): the encoder's widest layer holds a batch
      in one 2 GiB addressing window per launch, and 256 rows of 3000 frames do not fit it (DLIP_ERANGE).

    python tools/probes/voiced_frames_time.py [--reps 20] [--rows 256] [--frames 3000] [--step-rows 64] [--skip-step]
    -> one JSON line per part
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12          # bytes/s: the data sheet's rate, and what a float4 copy kernel reaches on this part
WINDOW = 300
VAD = {"energy_threshold": -0.25, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12}


def _time(fn, reps):
    """Median / min / max device-event milliseconds of fn(i) over ``reps`` calls after 4 warm-up calls."""
    for i in range(4):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(float(np.median(ms)), 4), round(float(min(ms)), 4), round(float(max(ms)), 4)]


def torch_stage(x, lens, compaction):
    """The stage's definition in torch ops (window 300 centred, norm_vars off, the VAD of ``VAD``, min_keep 1)."""
    B, C, NF = x.shape
    t = torch.arange(NF, device=x.device)[None, :]
    n = lens[:, None].long()
    valid = t < n
    x64 = torch.where(valid[:, None, :], x, torch.zeros((), device=x.device)).double()
    cs = torch.nn.functional.pad(torch.cumsum(x64, dim=2), (1, 0))
    b = t - WINDOW // 2
    e = b + WINDOW
    shift = (-b).clamp(min=0)
    b, e = b + shift, e + shift
    over = (e - n).clamp(min=0)
    b, e = (b - over).clamp(min=0), torch.minimum(e, n).clamp(min=1)
    b = torch.minimum(b, e - 1)                                         # (columns behind the row: any in-range pair, masked below)
    win = torch.gather(cs, 2, e[:, None, :].expand(B, C, NF)) - torch.gather(cs, 2, b[:, None, :].expand(B, C, NF))
    y = torch.where(valid[:, None, :], (x64 - win / (e - b)[:, None, :]).float(), torch.zeros((), device=x.device))
    e0 = x[:, 0, :]
    thr = (VAD["energy_threshold"] + VAD["energy_mean_scale"] * torch.where(valid, e0, torch.zeros((), device=x.device)).double().sum(1) / lens).float()
    above = ((e0 > thr[:, None]) & valid).int()
    ca = torch.nn.functional.pad(torch.cumsum(above, dim=1), (1, 0))
    ctx = VAD["frames_context"]
    lo, hi = (t - ctx).clamp(min=0), torch.minimum(t + ctx, n - 1).clamp(min=0)
    num = torch.gather(ca, 1, hi + 1) - torch.gather(ca, 1, lo.expand(B, NF))
    den = hi - lo + 1
    voiced = (num.float() >= den.float() * np.float32(VAD["proportion_threshold"])) & valid
    count = voiced.sum(1)
    voiced = torch.where((count < 1)[:, None], valid, voiced)          # the fallback: a row without voiced frames keeps all
    out = torch.zeros_like(y)
    if compaction == "rows":
        for r in range(B):
            kept = y[r][:, voiced[r]]                                   # a boolean index: the host waits for the count
            out[r, :, :kept.shape[1]] = kept
    else:
        pos = torch.cumsum(voiced.int(), dim=1) - 1
        pos = torch.where(voiced, pos, torch.full_like(pos, NF)).long()      # dropped frames go to a column behind the row
        wide = torch.zeros((B, C, NF + 1), device=x.device)
        wide.scatter_(2, pos[:, None, :].expand(B, C, NF), y)
        out = wide[:, :, :NF].contiguous()
    return out, voiced.sum(1).int()


def stage_alone(reps, B, C, NF):
    from deeplip_amd import weightgen as wg
    from deeplip_amd.voiced_frames import VoicedFrames
    r = np.random.Generator(np.random.PCG64(12))
    lens_h = r.integers(NF // 2, NF + 1, size=B)
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    xs = [torch.from_numpy(wg.gen(f"probe.vf.x{k}", (B, C, NF))).cuda() for k in range(4)]      # four sets: past the Infinity Cache
    st = VoicedFrames(cmn_window=WINDOW, vad=VAD)
    cmn_only = VoicedFrames(cmn_window=WINDOW, vad=None)
    sel_only = VoicedFrames(cmn_window=None, vad=VAD)
    from deeplip_amd.plan import Arena, StepPlan
    from deeplip_amd import ops
    arenas = [Arena() for _ in xs]                                      # one set of output buffers per input set, allocated once

    def run(stage):
        def fn(i):
            a = arenas[i % 4]
            a.mode, a.cursor = ("collect" if not a.bufs else "replay"), 0
            ops.ARENA = a
            try:
                return stage(xs[i % 4], lens)
            finally:
                ops.ARENA = None
        return fn
    y, ol = st(xs[0], lens)
    kept = int(ol.sum().item())
    valid = int(lens_h.sum())
    out = {"rows": B, "features": C, "frames": NF, "valid_frames": valid, "kept_frames": kept,
           "fallback_rows": int(st.last_fallback.sum().item())}
    # what the algorithm moves: x's valid frames read once, every column of y written once, the energy row read once, pos written
    # by the VAD kernel and read once by the CMN kernel
    nbytes = {"stage": 4 * (C * valid + C * B * NF + valid + 2 * B * NF), "cmn_only": 4 * (C * valid + C * B * NF),
              "select_only": 4 * (C * valid + C * B * NF + valid + 2 * B * NF)}
    for name, s in (("stage", st), ("cmn_only", cmn_only), ("select_only", sel_only)):
        for a in arenas:
            a.bufs.clear()
        ms = _time(run(s), reps)
        rate = nbytes[name] / (ms[0] * 1e-3)
        out[name] = {"eager_ms_median_min_max": ms, "algorithm_bytes": nbytes[name], "eager_tb_per_s": round(rate / 1e12, 3)}
        # ... and as the product runs it, inside a recorded plan: eight replays per timing window (four plans, one per input set), so
        # the device is never waiting for the host between two launches -- the kernels' own time
        plans = [StepPlan(lambda x, l, s=s: s(x, l), xk, lens) for xk in xs]

        def replays(i):
            for k in range(8):
                plans[k % 4].run()
        ms = [round(v / 8, 4) for v in _time(replays, reps)]
        for pl in plans:
            pl.close()
        rate = nbytes[name] / (ms[0] * 1e-3)
        out[name].update({"plan_ms_median_min_max": ms, "tb_per_s": round(rate / 1e12, 3), "share_of_hbm_spec": round(rate / HBM_SPEC, 3),
                          "share_of_hbm_copy_rate": round(rate / HBM_COPY, 3)})
    for comp in ("rows", "scatter"):
        yt, lt = torch_stage(xs[0], lens, comp)
        out[f"torch_{comp}"] = {"ms_median_min_max": _time(lambda i: torch_stage(xs[i % 4], lens, comp), max(3, reps // 4)),
                                "lengths_equal": bool(torch.equal(lt, ol)),
                                "rel_diff_vs_stage": float((yt - y).abs().max() / y.abs().max()) if torch.equal(lt, ol) else None}
    return out


def step(reps, B, NF):
    import yaml
    from deeplip_amd import packing, weightgen as wg
    from deeplip_amd.frontend import AudioFrontend
    from deeplip_amd.trainer_common import encoder_min_frames
    from deeplip_amd.voiced_frames import VoicedFrames
    from models.audio_models.tdnn import SpeakerEmbNet
    with open(os.path.join(ROOT, "conf", "fusion_config.yaml")) as f:
        acfg = yaml.safe_load(f)["model"]["audio_config"]
    packing.set_precision("f16x3")
    net = SpeakerEmbNet(dict(acfg, arch="etdnn"))
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="audio.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.cuda().eval()
    fe = AudioFrontend("mfcc", normalize=False)
    S = fe.frame_len + (NF - 1) * fe.frame_step
    r = np.random.Generator(np.random.PCG64(13))
    slen = torch.tensor(r.integers(S // 2, S + 1, size=B), dtype=torch.int32, device="cuda")
    t = torch.arange(S, device="cuda", dtype=torch.float32)
    wave = 0.4 * torch.sin(t[None, :] * torch.linspace(0.02, 0.6, B, device="cuda")[:, None]) + 0.05 * torch.randn((B, S), device="cuda")
    gate = (torch.rand((B, S // 4000 + 1), device="cuda") > 0.3).float().repeat_interleave(4000, dim=1)[:, :S]      # pauses of 0.25 s
    wave = (wave * gate).contiguous()
    # float waveforms around 1 put the log-energy near 4 where 16-bit samples put it near 18: the threshold moves with them
    st = VoicedFrames(cmn_window=WINDOW, vad=dict(VAD, energy_threshold=-5.0), min_keep=encoder_min_frames(net))
    with torch.no_grad():
        feats, nf = fe(wave, slen)
        y, ol = st(feats, nf)
        out = {"rows": B, "frames": NF, "valid_frames": int(nf.sum().item()), "kept_frames": int(ol.sum().item()),
               "frontend_ms": _time(lambda i: fe(wave, slen), reps),
               "stage_ms": _time(lambda i: st(feats, nf), reps),
               "encoder_on_kept_ms": _time(lambda i: net.extract_embedding(y, lengths=ol), reps),
               "encoder_on_all_ms": _time(lambda i: net.extract_embedding(feats, lengths=nf), reps)}

        def whole(i):
            f, n = fe(wave, slen)
            f, n = st(f, n)
            return net.extract_embedding(f, lengths=n)
        out["step_ms"] = _time(whole, reps)
    out["stage_share_of_step"] = round(out["stage_ms"][0] / out["step_ms"][0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--step-rows", type=int, default=64)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("voiced_frames_time.py measures on the GPU: no ROCm device found")
    from deeplip_amd import build
    print(json.dumps({"box": build.box_id(), "stage_alone": stage_alone(a.reps, a.rows, 24, a.frames)}), flush=True)
    if not a.skip_step:
        print(json.dumps({"box": build.box_id(), "step": step(max(5, a.reps // 2), a.step_rows, a.frames)}), flush=True)


if __name__ == "__main__":
    main()
