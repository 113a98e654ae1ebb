#!/usr/bin/env python
"""The ResNet speech encoder's statistics pooling (`pooling: statistic`) at the size a user extracts at: B = 256, F = 24,
T = 300 through the shipped trunk (hidden [64,128,256], layers [3,3,3]) -> last map [256, 6, 75, 256] fp32 (118 MB).

  kernels    dlip_statpool_nhwc_f32, its backward, and a device-to-device copy of the same map bytes (the yardstick EXPERIMENTS R8.1
             uses for its kernel: what moving the bytes once costs on this box), device events around each launch, interleaved
             rounds, medians.  Bytes the algorithm needs: forward = one read of the map; backward = one read + one write.
  extract    extract_embedding of the shipped encoder with `statistic` against `average` (same trunk, same weights for it, same batch),
             interleaved rounds, medians, in both arithmetic modes.

    python tools/bench_audio_resnet_heads.py [--batch 256] [--frames 300] [--rounds 15] [--out FILE.json]
Prints one JSON line.  Needs a ROCm GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeplip_amd import ops, packing, weightgen as wg                      # noqa: E402
from deeplip_amd._lib import call                                           # noqa: E402
from deeplip_amd.audio_resnet import POOL_EPS                              # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def interleaved(fns, rounds, warm=3):
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f))
    return {k: statistics.median(v) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}


def net(pooling, F):
    from models.resnet import SpeakerEmbNet
    n = SpeakerEmbNet({"arch": "resnet", "resnet": {"input_dim": 1, "hidden_dim": [64, 128, 256], "residual_block_layers": [3, 3, 3],
                                                   "fc_layers": 1, "embedding_dim": 256, "pooling": pooling, "feat_dim": F}})
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in n.state_dict().items()}, prefix="aresnet.")
    n.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return n.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--feat", type=int, default=24)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_resnet_heads.py needs a ROCm GPU: nothing here is measured on a CPU")
    B, H, W, C = a.batch, ((a.feat - 1) >> 2) + 1, ((a.frames - 1) >> 2) + 1, 256
    m = torch.relu(torch.randn((B, H, W, C), device="cuda"))
    dst = torch.empty_like(m)
    y = ops.statpool_nhwc(m, None, 0, POOL_EPS)
    dy = torch.randn_like(y)
    dx = torch.empty_like(m)

    def bwd():          # (the entry point StatPoolNHWCFn.backward calls, on preallocated tensors: a launch, no allocation in the window)
        call("dlip_statpool_nhwc_bwd_f32", m, y, dy, POOL_EPS, dx, B, H, W, C)

    med, spread = interleaved({"statpool_fwd_us": lambda: ops.statpool_nhwc(m, None, 0, POOL_EPS), "statpool_bwd_us": bwd,
                               "copy_d2d_us": lambda: dst.copy_(m)}, a.rounds)
    nbytes = m.numel() * 4
    out = {"map": [B, H, W, C], "map_mbytes": round(nbytes / 1e6, 1), **{k: round(v, 1) for k, v in med.items()},
           "spread_us": {k: [round(x, 1) for x in v] for k, v in spread.items()},
           "statpool_fwd_tb_s": round(nbytes / med["statpool_fwd_us"] / 1e6, 2), "statpool_bwd_tb_s": round(2 * nbytes / med["statpool_bwd_us"] / 1e6, 2),
           "copy_d2d_tb_s": round(2 * nbytes / med["copy_d2d_us"] / 1e6, 2)}
    x = torch.from_numpy(wg.audio_input(B, a.feat, a.frames, key="bench.aresnet.heads")).unsqueeze(1).cuda()
    for mode in ("f32", "f16x3"):
        packing.set_precision(mode)
        nets = {p: net(p, a.feat) for p in ("average", "statistic")}
        with torch.no_grad():
            med, _ = interleaved({p: (lambda n=n: n.extract_embedding(x)) for p, n in nets.items()}, max(5, a.rounds // 3), warm=2)
        out[f"extract_{mode}_ms"] = {p: round(v / 1e3, 3) for p, v in med.items()}
        out[f"extract_{mode}_statistic_over_average"] = round(med["statistic"] / med["average"], 4)
    packing.set_precision("f32")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
