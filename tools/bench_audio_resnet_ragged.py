#!/usr/bin/env python3
"""Extracting a test list through the ResNet speech encoder (`arch: resnet`, shipped config: hidden [64,128,256], layers [3,3,3],
F = 40): a seeded list of utterances with lengths uniform in 137 .. 412 frames, in utterances/s, per arithmetic mode (f32, f16x3):

  (a) loop     extract_embedding on one utterance at a time at its own length, the features already on the device -- the
               reference's test loop (train_audio.py:343-373) and the only path the encoder had before it took length vectors
  (b) ragged   deeplip_amd.extract.RaggedExtractor at batch 64: length-bucketed zero-padded batches + int32 length vectors through
               one recorded plan per padded shape, host batches pinned and cached (the GPU is timed, not numpy)

Both in ONE process: a first pass of each warms every shape (and records (b)'s plans), then `--rounds` timed passes alternate
(a), (b), (a), (b), ... with a device synchronisation on both sides of every timed window; the medians are reported with the ratio
(b) / (a) and ragged.padding_overhead of (b)'s batches.  Numbers of different boxes of the pool differ by several percent: compare
within one call only.

    python tools/bench_audio_resnet_ragged.py [--utts 2048] [--rounds 3] [--batch 64]
    python tools/bench_audio_resnet_ragged.py --forwards 20     only that many eager batched forwards per mode (B = 64, T = 300,
                                                                lengths 273 .. 300): run it under rocprofv3 --kernel-trace --stats
                                                                for the share of time_tail_zero_kernel / avgpool_time_ragged_kernel

Engine only; prints one line per measurement and one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import yaml  # noqa: E402

from deeplip_amd import _lib, arith, weightgen as wg  # noqa: E402
from deeplip_amd.extract import RaggedExtractor  # noqa: E402
from deeplip_amd.ragged import pad_stack  # noqa: E402
from deeplip_amd.trainer_common import encoder_min_frames  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, LMIN, LMAX = 40, 137, 412


class RaggedList:
    """The list interface RaggedExtractor walks (deeplip_amd.synthetic.SyntheticAVSet's), audio only: utterance i is one of 16
    seeded [F, 412] feature matrices cut to its own length."""

    def __init__(self, n: int, seed: int):
        r = np.random.Generator(np.random.PCG64(seed))
        self.audio_len = r.integers(LMIN, LMAX + 1, size=n).astype(np.int64)
        self.clip_ptr = np.zeros((n + 1,), dtype=np.int32)
        self.clip_len = np.zeros((0,), dtype=np.int64)
        self.bank = wg.audio_input(16, F, LMAX, key="bench.aresnet.x", speakers=list(range(16)))

    def __len__(self):
        return len(self.audio_len)

    def audio_item(self, i: int) -> np.ndarray:
        return np.ascontiguousarray(self.bank[i % 16][:, :int(self.audio_len[i])])

    def audio_padded(self, idx, T=None, rows=None):
        items = [self.audio_item(i) for i in idx]
        L = np.array([it.shape[1] for it in items], dtype=np.int32)
        return pad_stack(items, int(T or L.max()), axis=1, rows=rows), L


def model():
    from models.resnet import SpeakerEmbNet
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        opts = yaml.safe_load(f)["model"]
    net = SpeakerEmbNet(dict(opts, arch="resnet"))
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="aresnet.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda().eval()


def window(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def extraction(a):
    ds = RaggedList(a.utts, a.seed)
    n = len(ds)
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "utts": n, "batch": a.batch, "rounds": a.rounds, "frames": int(ds.audio_len.sum()), "modes": {}}
    with torch.no_grad():
        net = model()
        items = [torch.from_numpy(ds.audio_item(i)[None, None]).to(dev) for i in range(n)]       # [1,1,F,L_i], resident
        for mode in ("f32", "f16x3"):
            arith.configure(mode)
            D = net.embedding_dim
            ex = RaggedExtractor(lambda x, l: net.extract_embedding(x, lengths=l)[0], None, dev, batch=a.batch, audio_min_frames=encoder_min_frames(net))
            cache: dict = {}
            rows = torch.empty((n, D), device=dev)

            def loop():
                for i, it in enumerate(items):
                    rows[i] = net.extract_embedding(it)[0][0]

            def ragged():
                return ex.run(ds, 0, n, D, host_cache=cache)[0]

            window(loop)                                           # every length once: kernels, workspaces
            table = ragged()                                       # every padded shape once: its plan recorded
            torch.cuda.synchronize()
            _lib.check_range(sync=True)
            err = float((table - rows).abs().max() / rows.abs().max())
            ta, tb = [], []
            for _ in range(a.rounds):
                ta.append(window(loop))
                tb.append(window(ragged))
            st = dict(ex.stats)
            ex.close()
            la, lb = n / float(np.median(ta)), n / float(np.median(tb))
            out["modes"][mode] = {"loop_utt_per_s": round(la, 1), "ragged_utt_per_s": round(lb, 1), "ratio": round(lb / la, 3),
                                  "loop_s": [round(t, 4) for t in ta], "ragged_s": [round(t, 4) for t in tb],
                                  "padding_overhead": st["audio_padding_overhead"], "batches": st["audio_batches"],
                                  "shapes": st["audio_shapes"], "plans_recorded": st["plans_recorded"], "f32_reruns": st["f32_reruns"],
                                  "rows_vs_loop_rel_err": err}
            print(f"{mode:6s} loop {la:9.1f} utt/s   ragged (batch {a.batch}) {lb:9.1f} utt/s   x{lb / la:6.2f}   padding overhead "
                  f"{st['audio_padding_overhead']:.4f}, {st['audio_batches']} batches of {st['audio_shapes']} shapes, rows vs loop {err:.2e}",
                  flush=True)
    print(json.dumps(out))


def forwards(a):
    r = np.random.Generator(np.random.PCG64(a.seed))
    T = 300
    lens = r.integers(273, T + 1, size=a.batch).astype(np.int32)      # one rung of the 10 % ladder
    lens[-1] = T
    x = torch.from_numpy(wg.audio_input(a.batch, F, T, key="bench.aresnet.fw")).cuda()
    l = torch.from_numpy(lens).cuda()
    with torch.no_grad():
        net = model()
        for mode in ("f32", "f16x3"):
            arith.configure(mode)
            for _ in range(a.forwards):
                net.extract_embedding(x, lengths=l)
            torch.cuda.synchronize()
            _lib.check_range(sync=True)
    print(json.dumps({"forwards_per_mode": a.forwards, "batch": a.batch, "T": T, "padding_share": round(1.0 - float(lens.sum()) / (a.batch * T), 4)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seed", type=int, default=20260)
    ap.add_argument("--forwards", type=int, default=0)
    a = ap.parse_args()
    forwards(a) if a.forwards else extraction(a)


if __name__ == "__main__":
    main()
