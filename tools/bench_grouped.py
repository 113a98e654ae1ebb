#!/usr/bin/env python3
"""Border groups of the ring kernel, per layer: grouped (dlip_debug_set(10, 1)) against ungrouped (0), ALTERNATING in one process,
for the 3x3 launches of ResNet layers 2.0 / 3 / 4 at the bench's batch (split-format activations, residual / shortcut as in the
trunk).  Per mode: median and min over the rounds and the spread (max - min) of the rounds -- a layer belongs under the rule only
where grouped is faster by more than the spread of its own ungrouped timings."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deeplip_amd import _lib, ops, packing

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=8, help="timed rounds per mode (one more runs first as warm-up and is dropped)")
ap.add_argument("--only", default="")
a = ap.parse_args()
N = a.batch * 29
L = [  # name, input, K, stride, residual, shortcut source (H2, C2) or None, launches per step
    ("l2.0.conv1", (N, 22, 22, 64), 128, 2, False, None, 1),
    ("l2.0.conv2", (N, 11, 11, 128), 128, 1, False, (22, 64), 1),
    ("l3.0.conv1", (N, 11, 11, 128), 256, 2, False, None, 1),
    ("l3.0.conv2", (N, 6, 6, 256), 256, 1, False, (11, 128), 1),
    ("l3.1.conv", (N, 6, 6, 256), 256, 1, True, None, 2),
    ("l4.0.conv1", (N, 6, 6, 256), 512, 2, False, None, 1),
    ("l4.0.conv2", (N, 3, 3, 512), 512, 1, False, (6, 256), 1),
    ("l4.1.conv1", (N, 3, 3, 512), 512, 1, True, None, 1),
]


def timed(fn):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters


tot = {0: 0.0, 1: 0.0}
for name, (n, h, w, c), k, st, res, short, count in L:
    if a.only and a.only not in name:
        continue
    x = ops.split_pack(torch.randn(n, h, w, c, device="cuda"))
    b = torch.randn(k, device="cuda")
    sl = torch.rand(k, device="cuda")
    if short is None:
        wsp, wsc = packing.split_weights(torch.randn(k, 3, 3, c, dtype=torch.float64) * 0.05)
        wsp, wsc = wsp.cuda(), wsc.cuda()
        kw = dict(stride=(st, st), pad=(1, 1), slope=sl, w_scale=wsc, x_split=True, out_split=True)
        y = ops.conv_nhwc(x, wsp, b, **kw)
        rs = ops.split_pack(torch.randn_like(y)) if res else None
        fn = lambda: ops.conv_nhwc(x, wsp, b, residual=rs, out=y, **kw)
    else:
        h2, c2 = short
        x2 = ops.split_pack(torch.randn(n, h2, h2, c2, device="cuda"))
        wsp, wsc = packing.split_weights(torch.randn(k, 9 * c + c2, dtype=torch.float64) * 0.05)
        wsp, wsc = wsp.cuda(), wsc.cuda()
        fn = lambda: ops.conv2_nhwc(x, x2, wsp, b, wsc, pad=(1, 1), stride2=(2, 2), slope=sl, out_split=True)
    t = {0: [], 1: []}
    outs = {}
    for rnd in range(a.rounds + 1):
        for mode in (0, 1):
            _lib.debug_set(_lib.DBG_GROUPED, mode)
            if rnd == 0:
                outs[mode] = ops.split_unpack(fn()).clone()
            us = timed(fn)
            if rnd > 0:       # (round 0: clocks and caches settle)
                t[mode].append(us)
    _lib.debug_set(_lib.DBG_GROUPED, -1)
    dmax = float((outs[0] - outs[1]).abs().max() / outs[0].abs().max())
    m = {k_: statistics.median(v) for k_, v in t.items()}
    for mode in (0, 1):
        tot[mode] += m[mode] * count
    print(f"{name:11s} x{count}  ungrouped med {m[0]:7.1f} min {min(t[0]):7.1f} spread {max(t[0]) - min(t[0]):5.1f} us | "
          f"grouped med {m[1]:7.1f} min {min(t[1]):7.1f} spread {max(t[1]) - min(t[1]):5.1f} us | "
          f"{(m[1] / m[0] - 1) * 100:+6.1f} %  max|d|/max {dmax:.1e}", flush=True)
print(f"sum(us x count): ungrouped {tot[0]:8.0f}  grouped {tot[1]:8.0f}  {(tot[1] / tot[0] - 1) * 100:+.1f} %")
