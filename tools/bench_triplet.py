#!/usr/bin/env python3
"""OnlineTriplet at the shipped batch: B = 256 embeddings of E = 512 features over 57 speakers (conf/audio_config.yaml: bs,
embedding_dim; the speaker count of the shipped lists).  Per selector (hardest, semihard, random, all): mining + loss + backward
through ``deeplip_amd.loss.OnlineTriplet`` -- eager (launches issued from Python) and inside a recorded plan (torch.cuda.CUDAGraph
replay, what a recorded training step does) -- in ms per call, plus the number of triplets.  Then the parts: G = X X^T by the mining
entry point's own MFMA kernel against the existing exact GEMM (``autograd._gemm``), the mining kernel alone, the loss entry point,
the backward entry point.

    python tools/bench_triplet.py [--iters 200] [--batch 256] [--dim 512] [--speakers 57]

Engine only, one process; prints one line per measurement and one JSON line.  Per-kernel times: run it under
rocprofv3 --kernel-trace --stats (counters in a run of their own)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeplip_amd import autograd as ag, triplet as tp, weightgen as wg  # noqa: E402
from deeplip_amd.loss import OnlineTriplet  # noqa: E402

MARGIN = 0.2


def inputs(B, E, S):
    labels = np.minimum((wg.gen("bench_triplet.labels", (B,), kind="uniform") * S).astype(np.int64), S - 1)
    x = 0.1 * (0.2 * wg.gen("bench_triplet.centres", (S, E))[labels] + wg.gen("bench_triplet.noise", (B, E)))
    return torch.from_numpy(x.astype(np.float32)).cuda(), torch.from_numpy(labels).cuda()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--speakers", type=int, default=57)
    a = ap.parse_args()
    B, E, S = a.batch, a.dim, a.speakers
    x, lab = inputs(B, E, S)
    out = {"B": B, "E": E, "speakers": S, "iters": a.iters, "device": torch.cuda.get_device_name(0)}
    stream = torch.cuda.Stream()
    for name in ("hardest", "semihard", "random", "all"):
        crit = OnlineTriplet(MARGIN, tp.make_selector(name, MARGIN))
        with torch.cuda.stream(stream):          # (the leaf's gradient accumulator belongs to the stream that captures)
            xg = x.clone().requires_grad_()
        state = {}

        def step():
            xg.grad = None
            loss, n = crit(xg, lab)
            loss.backward()
            state["n"] = n
            return loss

        with torch.cuda.stream(stream):
            eager = timed(step, a.iters)
            n = int(state["n"])
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=stream):
                step()
            replay = timed(g.replay, a.iters)
        out[name] = {"eager_ms": round(eager, 4), "replay_ms": round(replay, 4), "triplets": n}
        print(f"{name:9s} mining + loss + backward: eager {eager * 1e3:8.1f} us, recorded {replay * 1e3:8.1f} us per call, {n} triplets")
    # the parts, each recorded on its own and replayed (device time plus the graph launch; the kernel trace has the kernels alone)
    lab32 = lab.to(torch.int32)
    parts = {
        "G by the mining entry point (MFMA 16x16x4 f32)": lambda: tp.mine(x, lab32, MARGIN, tp.MODE_ALL),
        "G by autograd._gemm (dlip_gemm_small_f32)": lambda: ag._gemm(x, x, B, B, E, tb=True),
        "G + mining, hardest": lambda: tp.mine(x, lab32, MARGIN, tp.MODE_HARDEST),
    }
    m = tp.mine(x, lab32, MARGIN, tp.MODE_HARDEST)
    loss, n, wc = tp.loss_forward(m, MARGIN)
    parts["loss, hardest"] = lambda: tp.loss_forward(m, MARGIN)
    parts["backward, hardest"] = lambda: tp.loss_backward(x, m, wc, n)
    with torch.cuda.stream(stream):
        for k, fn in parts.items():
            g = torch.cuda.CUDAGraph()
            fn()
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=stream):
                keep = fn()      # noqa: F841 -- the graph's pool owns the outputs
            ms = timed(g.replay, a.iters)
            out.setdefault("parts_replay_ms", {})[k] = round(ms, 4)
            print(f"  {k:48s} {ms * 1e3:8.1f} us per recorded call")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
