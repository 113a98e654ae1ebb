#!/usr/bin/env python3
"""Speech embeddings of a test list FROM WAVEFORMS: MFCC-24 front-end + the shipped E-TDNN over a seeded list of utterances whose
durations frame into 137 .. 412 frames (the spread of the test lists), in utterances/s and ms per pass:

  (a) loop      front-end and encoder on one utterance at a time at its own length, the waveform already on the device -- the
                reference's loop (train_fusion.py:334-349) and the only way before the front-end took length vectors
  (b) ragged    RaggedExtractor.run(waves=True) at batch 32: length-bucketed zero-padded waveform batches + int32 sample counts
                through ONE recorded plan (front-end + encoder) per padded shape, host batches pinned and cached
  (c) features  the feature-fed ragged extraction (RaggedExtractor.run on ready-made [B,24,T] features): the ceiling, no front-end

One process: a first pass of each warms every shape (and records the plans), then `--rounds` timed passes alternate (a), (b), (c);
every window lies between two HIP events on the idle device (synchronised on both sides); medians are reported.

    python tools/bench_frontend_ragged.py [--utts 512] [--rounds 3] [--batch 32]
    python tools/bench_frontend_ragged.py --rect 50     only the RECTANGULAR front-end call (lengths=None) on [32, 48000] waveforms,
                                                        50 timed calls per power-spectrum route: the figure to hold against the
                                                        same call of an older build on the same box

Engine only; prints one line per measurement and one JSON line."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from deeplip_amd import _lib, arith, weightgen as wg  # noqa: E402
from deeplip_amd.frontend import AudioFrontend  # noqa: E402
from deeplip_amd.trainer_common import encoder_min_frames  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model():
    from models.audio_models.tdnn import SpeakerEmbNet
    with open(os.path.join(ROOT, "conf", "fusion_config.yaml")) as f:
        acfg = yaml.safe_load(f)["model"]["audio_config"]
    net = SpeakerEmbNet(dict(acfg, arch="etdnn"))
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="audio.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda().eval()


def window(fn) -> float:
    """Milliseconds between two HIP events around fn(), the device idle on both sides."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    torch.cuda.synchronize()
    e1.record()
    e1.synchronize()
    return float(e0.elapsed_time(e1))


def extraction(a):
    from deeplip_amd.extract import RaggedExtractor
    from deeplip_amd.synthetic import SyntheticAVSet
    ds = SyntheticAVSet(a.utts // 8, 8, 0, audio_dim=24, key="bench.fe.ragged", seed=a.seed, ragged=True, audio_range=(137, 412))
    n, dev = len(ds), torch.device("cuda")
    arith.configure(a.arith)
    out = {"device": torch.cuda.get_device_name(0), "utts": n, "batch": a.batch, "rounds": a.rounds, "arith": a.arith,
           "frames": int(ds.audio_len.sum())}
    with torch.no_grad():
        net, fe = model(), AudioFrontend("mfcc")
        D = net.embedding_dim
        waves = [torch.from_numpy(ds.wave_item(i)[None]).to(dev) for i in range(n)]           # [1, S_i], resident
        rows = torch.empty((n, D), device=dev)

        def wave_step(w, l):
            feats, nf = fe(w, l)
            return net.extract_embedding(feats, lengths=nf)[0]

        kw = dict(batch=a.batch, audio_min_frames=encoder_min_frames(net))
        ex_w = RaggedExtractor(wave_step, None, dev, wave_geometry=(fe.frame_len, fe.frame_step), **kw)
        ex_f = RaggedExtractor(lambda x, l: net.extract_embedding(x, lengths=l)[0], None, dev, **kw)
        cw, cf = {}, {}

        def loop():
            for i, w in enumerate(waves):
                rows[i] = net.extract_embedding(fe(w))[0][0]

        ragged = lambda: ex_w.run(ds, 0, n, D, host_cache=cw, waves=True)[0]
        feats = lambda: ex_f.run(ds, 0, n, D, host_cache=cf)[0]
        window(loop)                                                   # every length once
        table = ragged()                                               # every padded shape once: its plan recorded
        feats()
        _lib.check_range(sync=True)
        out["rows_vs_loop_rel_err"] = float((table - rows).abs().max() / rows.abs().max())
        t = {"loop": [], "ragged": [], "features": []}
        for _ in range(a.rounds):
            t["loop"].append(window(loop))
            t["ragged"].append(window(ragged))
            t["features"].append(window(feats))
        st = dict(ex_w.stats)
        ex_w.close(); ex_f.close()
    for k, v in t.items():
        ms = float(np.median(v))
        out[k] = {"ms": round(ms, 2), "utt_per_s": round(n / ms * 1e3, 1), "passes_ms": [round(x, 2) for x in v]}
        print(f"{k:9s} {ms:10.2f} ms / pass   {n / ms * 1e3:10.1f} utt/s", flush=True)
    out["ragged_over_loop"] = round(out["ragged"]["utt_per_s"] / out["loop"]["utt_per_s"], 3)
    out.update(padding_overhead=st["audio_padding_overhead"], batches=st["audio_batches"], shapes=st["audio_shapes"],
               plans_recorded=st["plans_recorded"], f32_reruns=st["f32_reruns"])
    print(json.dumps(out))


def rectangular(a):
    """The call that predates the length vector: AudioFrontend(...)(wave) on [32, 48000], per route, in microseconds per call."""
    r = np.random.Generator(np.random.PCG64(a.seed))
    x = torch.from_numpy((0.1 * r.standard_normal((32, 48000))).astype(np.float32)).cuda()
    out = {"device": torch.cuda.get_device_name(0), "calls": a.rect, "shape": [32, 48000]}
    for route in ("fft64", "gemm32", "direct64"):
        fe = AudioFrontend("mfcc", delta=True, dft=route)
        for _ in range(5):
            fe(x)
        ms = [window(lambda: fe(x)) for _ in range(a.rect)]
        out[route] = {"median_us": round(float(np.median(ms)) * 1e3, 1), "min_us": round(float(np.min(ms)) * 1e3, 1)}
        print(f"rectangular {route:9s} median {out[route]['median_us']:9.1f} us   min {out[route]['min_us']:9.1f} us", flush=True)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seed", type=int, default=20261)
    ap.add_argument("--arith", default="auto", choices=["auto", "f32", "f16x3"])
    ap.add_argument("--rect", type=int, default=0)
    a = ap.parse_args()
    rectangular(a) if a.rect else extraction(a)


if __name__ == "__main__":
    main()
