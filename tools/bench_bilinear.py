#!/usr/bin/env python3
"""BNBilinear at the shipped sizes (d1 = d2 = 512, o = 512, k = 30: two 512 x 15 360 fp32 factor matrices, 63 MB) at B = 60
(conf/fusion_config.yaml: bs) and B = 256.  Per batch size, each inside a recorded plan (torch.cuda.CUDAGraph replay, what a
recorded training step does), in us per call:

  eval forward            the pooling launch + the finish launch
  train forward+backward  the module in train mode, a sum loss, backward (dU, dV, dgamma, dbeta; frozen embeddings as in train_fusion)
  the parts               pooling without / with keeping P and Q, the weight-gradient launch, the input-gradient launch

with the achieved bytes/s against the bytes that MUST move (forward: U and V read once; backward: U and V not read at all by the
weight gradient, so dU and dV written once plus P, Q read once -- the line prints both that and the issue's U + V + dU + dV figure)
and the achieved FLOP/s against the fp32 matrix peak of 157.3 TFLOP/s.

    python tools/bench_bilinear.py [--iters 100] [--batches 60 256]

Engine only, one process; prints one line per measurement and one JSON line.  Per-kernel times: run it under
rocprofv3 --kernel-trace --stats (counters in a run of their own)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplip_amd import ops  # noqa: E402
from deeplip_amd.fusion import BNBilinear  # noqa: E402

PEAK_FLOPS = 157.3e12
D, O, K = 512, 512, 30


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="*", default=[60, 256])
    a = ap.parse_args()
    torch.manual_seed(0)
    out = {"d": D, "o": O, "k": K, "iters": a.iters, "device": torch.cuda.get_device_name(0), "batches": {}}
    wbytes = 2 * D * K * O * 4                         # U + V (= dU + dV)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        m = BNBilinear(D, D, O, k=K).cuda()
        U, V = m.U.detach(), m.V.detach()
        for B in a.batches:
            e1, e2 = torch.randn(B, D, device="cuda"), torch.randn(B, D, device="cuda")
            pq = 2 * B * K * O * 4
            f_fwd = 2 * 2.0 * B * D * K * O            # two products
            r = {}

            def line(name, ms, nbytes, flop):
                r[name] = {"us": round(ms * 1e3, 2), "GBps": round(nbytes / ms / 1e6, 1), "TFLOPs": round(flop / ms / 1e9, 2),
                           "of_peak": round(flop / ms / 1e9 / (PEAK_FLOPS / 1e12), 3)}
                print(f"B={B:4d} {name:44s} {ms * 1e3:9.1f} us  {nbytes / ms / 1e6:8.1f} GB/s  {flop / ms / 1e9:7.2f} TFLOP/s "
                      f"({100 * flop / ms / 1e9 / (PEAK_FLOPS / 1e12):4.1f} % of 157.3)")

            m.eval()
            with torch.no_grad():
                line("eval forward (pool + finish)", recorded(lambda: m(e1, e2), stream, a.iters), wbytes, f_fwd)
                line("pool, P and Q not written", recorded(lambda: ops.bilinear_pool(e1, e2, U, V, K), stream, a.iters), wbytes, f_fwd)
                line("pool, P and Q kept", recorded(lambda: ops.bilinear_pool(e1, e2, U, V, K, save=True), stream, a.iters), wbytes + pq, f_fwd)
                z, P, Q = ops.bilinear_pool(e1, e2, U, V, K, save=True)
                dz = torch.randn_like(z)
                line("weight gradient (dU, dV; P, Q read)", recorded(lambda: ops.bilinear_pool_bwd_w(e1, e2, P, Q, dz, K), stream, a.iters),
                     wbytes + pq, f_fwd)
                line("input gradient (de1, de2)", recorded(lambda: ops.bilinear_pool_bwd_x(P, Q, dz, U, V, K), stream, a.iters), wbytes + pq, f_fwd)
            m.train()

            def step():
                for p in m.parameters():
                    p.grad = None
                y = m(e1, e2)
                y.sum().backward()
                return y
            ms = recorded(step, stream, a.iters)
            line("train forward + backward (U, V, P, Q, dU, dV)", ms, 2 * wbytes + 2 * pq, 2 * f_fwd)
            r["train forward + backward (U, V, P, Q, dU, dV)"]["GBps_of_U_V_dU_dV_alone"] = round(2 * wbytes / ms / 1e6, 1)
            out["batches"][str(B)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
