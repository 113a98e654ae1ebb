#!/usr/bin/env python3
"""Throughput of Lipreading(backbone_type='shufflenet').embed on one GPU, per width, eager and recorded (StepPlan), next to the ResNet
lip-clip encoder's embed measured in the same process.  Prints one JSON line.

    python tools/bench_shufflenet.py [--batch 64] [--frames 29] [--iters 20] [--widths 0.5,1.0,1.5,2.0]

Weights come from deeplip_amd.weightgen (seeded), clips from weightgen.video_input.  The ShuffleNet path is exact fp32 under every
arithmetic mode; the ResNet figure is taken in the library's default mode (auto: split fp16), as bench.py runs it.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplip_amd import weightgen as wg  # noqa: E402
from deeplip_amd.plan import StepPlan  # noqa: E402
from deeplip_amd.video import Lipreading  # noqa: E402

TCN_OPTS = {"num_layers": 4, "kernel_size": [3, 5, 7], "dropout": 0.2, "dwpw": False, "width_mult": 1}
# multiply-adds x 2 per 29-frame 88 x 88 clip (torch.utils.flop_counter on the reference, extract_feats=True)
GFLOP_PER_CLIP = {0.5: 0.98, 1.0: 2.04, 2.0: 6.52}


def model(backbone, width=1.0):
    m = Lipreading(hidden_dim=256, backbone_type=backbone, num_classes=500, relu_type="prelu", tcn_options=TCN_OPTS,
                   width_mult=width, extract_feats=True)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, prefix=f"bench.{backbone}.{width}.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval().cuda()


def timed(fn, iters):
    """ms per call: host clock around `iters` calls closed by a device synchronise (warm-up done by the caller)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def measure(m, x, iters):
    with torch.no_grad():
        for _ in range(3):
            m.embed(x)
        eager_ms = timed(lambda: m.embed(x), iters)
        plan = StepPlan(lambda v: m.embed(v), x.clone())
        for _ in range(3):
            plan.run()
        plan_ms = timed(plan.run, iters)
        launches = plan.launches
        plan.close()
    B = x.shape[0]
    return {"eager_ms": round(eager_ms, 3), "plan_ms": round(plan_ms, 3), "eager_clips_per_s": round(B / eager_ms * 1e3, 1),
            "plan_clips_per_s": round(B / plan_ms * 1e3, 1), "launches_per_forward": launches}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=29)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--widths", default="0.5,1.0,1.5,2.0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shufflenet: no GPU (the numbers are GPU timings; there is no CPU fallback)")
    x = torch.from_numpy(wg.video_input(a.batch, frames=a.frames, key="bench.shufflenet")).cuda()
    out = {"batch": a.batch, "frames": a.frames, "iters": a.iters, "device": torch.cuda.get_device_name(0), "shufflenet": {}}
    for w in [float(s) for s in a.widths.split(",")]:
        r = measure(model("shufflenet", w), x, a.iters)
        if w in GFLOP_PER_CLIP and a.frames == 29:
            r["tflops_plan"] = round(GFLOP_PER_CLIP[w] * r["plan_clips_per_s"] / 1e3, 2)
        out["shufflenet"][str(w)] = r
        torch.cuda.empty_cache()
    out["resnet"] = measure(model("resnet"), x, a.iters)
    out["resnet_embed_clips_per_s"] = out["resnet"]["plan_clips_per_s"]
    out["shufflenet_w1_embed_clips_per_s"] = out["shufflenet"].get("1.0", {}).get("plan_clips_per_s")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
