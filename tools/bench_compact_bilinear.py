#!/usr/bin/env python3
"""CompactBilinearPooling / BNCompactBilinear at the shipped sizes (d1 = d2 = 512, D = 512) at B = 60 (conf/fusion_config.yaml: bs)
and B = 256.  Per batch size, each inside a recorded graph (torch.cuda.CUDAGraph replay, what a recorded training step does), in
us per call:

  bare launch                 the same entry point at B = 1, d = 4, D = 4: what one replayed launch costs with nothing to do
  forward                     the layer, sketches not kept (frozen inputs, as in train_fusion)
  forward, sketches kept      the same launch writing psi1, psi2
  backward                    both input gradients (not on the trainer's path: its encoders are frozen)
  forward + backward          the layer through autograd, both inputs asking for gradients, a sum loss
  head train step             BNCompactBilinear in train mode, frozen inputs: forward, L2 norm, BatchNorm, sum loss, backward to
                              dgamma / dbeta
  head eval forward           the layer + the finish launch

with the achieved FMA rate (B P D^2 multiply-adds per convolution; the sketches' d1 + d2 adds per position are not counted) against
the 78.6 T FMA/s (157.3 TFLOP/s) of the fp32 vector ALUs.

    python tools/bench_compact_bilinear.py [--iters 100] [--batches 60 256]
    python tools/bench_compact_bilinear.py --trainer [--rounds 2]     train_fusion.Trainer('train') at bs 60, LMCL: `linear` and
                                                                      `compact_bilinear` alternating in one process

Engine only, one process; prints one line per measurement and one JSON line.  Per-kernel times: run it under
rocprofv3 --kernel-trace --stats (counters in a run of their own)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplip_amd import ops  # noqa: E402
from deeplip_amd.fusion import BNCompactBilinear, CompactBilinearPooling  # noqa: E402

PEAK_FMA = 78.65e12
C, D = 512, 512


def timed(fn, iters):
    """ms per call between two events on the current stream (3 warm-up calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def recorded(fn, stream, iters):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        keep = fn()      # noqa: F841 -- the graph's pool owns the outputs
    return timed(g.replay, iters)


def kernels(a):
    torch.manual_seed(0)
    out = {"C": C, "D": D, "iters": a.iters, "device": torch.cuda.get_device_name(0), "batches": {}}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tiny = CompactBilinearPooling(4, 4, 4).cuda()
        t = torch.randn(1, 4, device="cuda")
        with torch.no_grad():
            tiny(t, t)
            bare = recorded(lambda: tiny(t, t), stream, a.iters)
        out["bare_launch_us"] = round(bare * 1e3, 2)
        print(f"bare launch (B = 1, d = 4, D = 4) {bare * 1e3:9.2f} us")
        head = BNCompactBilinear(C, C, D).cuda()
        m = head.cbp
        for B in a.batches:
            e1, e2 = torch.randn(B, C, device="cuda"), torch.randn(B, C, device="cuda")
            g1, g2 = e1.clone().requires_grad_(), e2.clone().requires_grad_()
            fma = float(B) * D * D
            r = {}

            def line(name, ms, n_conv):
                rate = n_conv * fma / ms / 1e9                     # T FMA/s
                r[name] = {"us": round(ms * 1e3, 2), "TFMAs": round(rate, 3), "of_peak": round(rate / (PEAK_FMA / 1e12), 4),
                           "x_bare_launch": round(ms / bare, 2)}
                print(f"B={B:4d} {name:28s} {ms * 1e3:9.2f} us  {rate:7.3f} T FMA/s ({100 * rate / (PEAK_FMA / 1e12):5.2f} % of 78.6)  "
                      f"{ms / bare:5.2f} x bare launch")

            with torch.no_grad():
                p = m._pack(e1.device)
                line("forward", recorded(lambda: m(e1, e2), stream, a.iters), 1)
                line("forward, sketches kept", recorded(lambda: ops.compact_bilinear(e1, e2, p["s1"], p["s2"], True, save=True), stream, a.iters), 1)
                z, psi1, psi2 = ops.compact_bilinear(e1, e2, p["s1"], p["s2"], True, save=True)
                dz = torch.randn_like(z)
                line("backward (dx1, dx2)", recorded(lambda: ops.compact_bilinear_bwd(dz, psi1, psi2, p["s1"], p["s2"], e1.shape, e2.shape), stream,
                                                     a.iters), 2)
                head.eval()
                line("head eval forward", recorded(lambda: head(e1, e2), stream, a.iters), 1)

            def fb():
                g1.grad = g2.grad = None
                y = m(g1, g2)
                y.sum().backward()
                return y
            line("forward + backward", recorded(fb, stream, a.iters), 3)
            head.train()

            def step():
                for q in head.parameters():
                    q.grad = None
                y = head(e1, e2)
                y.sum().backward()
                return y
            line("head train step", recorded(step, stream, a.iters), 1)
            out["batches"][str(B)] = r
    print(json.dumps(out))


def trainer(a):
    """Two heads alternating in one process: the step is bound by the frozen encoders, so the heads are compared by how far they
    differ against how far one of them differs from itself between the rounds."""
    import tempfile
    import train_fusion
    ov = {"train.bs": 60, "train.loss": "LMCL", "train.steps_per_epoch": 12, "train.data_cache": 2, "train.epoch": 2, "data.utt_per_spk": 4}
    res = {"device": torch.cuda.get_device_name(0), "rounds": []}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for rnd in range(a.rounds):
                row = {}
                for kind in ("linear", "compact_bilinear"):
                    tr = train_fusion.Trainer("train", overrides=dict(ov, **{"model.fusion": kind}))
                    try:
                        tr.current_epoch = 1
                        tr._train_epoch()                      # eager head step, recording, first replays
                        tr.current_epoch = 2
                        tr._train_epoch()
                        st = tr.last_epoch_stats
                        row[kind] = {"pairs_per_s": round(st["pairs_per_s"], 1), "ms_per_step": round(st["ms_per_step"], 4),
                                     "step_mode": st["step_mode"], "loss": round(st["loss"], 4)}
                    finally:
                        tr.close()
                    print(f"round {rnd} {kind:17s} {row[kind]}", flush=True)
                res["rounds"].append(row)
        finally:
            os.chdir(cwd)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="*", default=[60, 256])
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    trainer(a) if a.trainer else kernels(a)


if __name__ == "__main__":
    main()
