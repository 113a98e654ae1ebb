#!/usr/bin/env python3
"""Segment boundaries of the ring kernel's ping-pong 256 x 128 tile, per layer: dlip_debug_set(11, 0 | 1 | 2) -- the LDS-staged
epilogue, the epilogue from the accumulators, that plus the next segment's head issued in front of it -- ALTERNATING in one process,
for the split-output 3x3 launches of ResNet layers 2.0 / 3 / 4 at the bench's batch (split-format activations, residual / shortcut
and border groups as in the trunk).  Per route: median and min over the rounds and the spread (max - min) of the rounds; a route
counts as faster on a layer only where it wins by more than the spread of that layer's route-0 timings."""
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
ap.add_argument("--rounds", type=int, default=8, help="timed rounds per route (one more runs first as warm-up and is dropped)")
ap.add_argument("--only", default="")
a = ap.parse_args()
N = a.batch * 29
ROUTES = (0, 1, 2)
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


tot = {r: 0.0 for r in ROUTES}
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
    t = {r: [] for r in ROUTES}
    outs = {}
    for rnd in range(a.rounds + 1):
        for route in ROUTES:
            _lib.debug_set(_lib.DBG_RING_HEAD, route)
            if rnd == 0:
                outs[route] = fn().clone().view(torch.int32)
            us = timed(fn)
            if rnd > 0:       # (round 0: clocks and caches settle)
                t[route].append(us)
    _lib.debug_set(_lib.DBG_RING_HEAD, -1)
    same = all(torch.equal(outs[0], outs[r]) for r in (1, 2))
    m = {r: statistics.median(v) for r, v in t.items()}
    for r in ROUTES:
        tot[r] += m[r] * count
    print(f"{name:11s} x{count}  route 0 med {m[0]:7.1f} min {min(t[0]):7.1f} spread {max(t[0]) - min(t[0]):5.1f} us | "
          f"route 1 med {m[1]:7.1f} min {min(t[1]):7.1f} {(m[1] / m[0] - 1) * 100:+6.1f} % | "
          f"route 2 med {m[2]:7.1f} min {min(t[2]):7.1f} {(m[2] / m[0] - 1) * 100:+6.1f} % | bits {'equal' if same else 'DIFFER'}", flush=True)
print(f"sum(us x count): route 0 {tot[0]:8.0f}  route 1 {tot[1]:8.0f} ({(tot[1] / tot[0] - 1) * 100:+.1f} %)  "
      f"route 2 {tot[2]:8.0f} ({(tot[2] / tot[0] - 1) * 100:+.1f} %)")
