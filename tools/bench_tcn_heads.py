#!/usr/bin/env python3
"""The lip-clip temporal heads side by side at B = 64 clips x T = 29 frames of ResNet features (512 channels): the dense MS-TCN
[3,5,7] (the shipped config), the single-branch TCN [3] dense and dwpw, and the dwpw MS-TCN [3,5,7].  Per head: the eval forward
(recorded StepPlan replay; eager), a recorded training step of the head alone (forward + backward + Adam, TrainStepGraph replay) and
the dlip_* launches of each (eval: the recorded plan's count; train: dlip_* calls of one eager step -- torch's own kernels of the
optimiser and of tensor fills are not counted).

    python tools/bench_tcn_heads.py [--iters 50] [--heads ms357,k3,k3_dwpw,ms357_dwpw]

Prints one line per head and one JSON line.  Per-kernel times: run it under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplip_amd import arith, weightgen as wg  # noqa: E402

HEADS = {"ms357": ([3, 5, 7], False), "k3": ([3], False), "k3_dwpw": ([3], True), "ms357_dwpw": ([3, 5, 7], True)}
B, T, CIN, CLASSES = 64, 29, 512, 500


def make(name, dropout):
    from deeplip_amd.video import TCN, MultiscaleMultibranchTCN
    ks, dwpw = HEADS[name]
    cls = TCN if len(ks) == 1 else MultiscaleMultibranchTCN
    opts = {"num_layers": 4, "kernel_size": ks, "dropout": dropout, "dwpw": dwpw, "width_mult": 1}
    h = cls(input_size=CIN, num_channels=[256 * len(ks)] * 4, num_classes=CLASSES, tcn_options=opts, dropout=dropout,
            relu_type="prelu", dwpw=dwpw)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in h.state_dict().items()}, prefix=f"bench_tcn_heads.{name}.")
    h.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return h.cuda()


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters      # us


def count_dlip_calls(fn):
    """dlip_* entry points called by fn (every one goes through _lib.call, which hands the status to _lib.check)."""
    from deeplip_amd import _lib
    n = [0]
    orig = _lib.check

    def counting(rc, what=""):
        n[0] += 1
        return orig(rc, what)
    _lib.check = counting
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib.check = orig
    return n[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--heads", default=",".join(HEADS))
    ap.add_argument("--arith", default="auto", choices=list(arith.MODES))
    a = ap.parse_args()
    arith.configure(a.arith)
    from deeplip_amd import autograd_video as av
    from deeplip_amd.plan import StepPlan
    from deeplip_amd.train_plan import TrainStepGraph
    x = torch.from_numpy(wg.gen("bench_tcn_heads.x", (B, T, CIN))).cuda()
    ln = torch.full((B,), T, dtype=torch.int32, device="cuda")
    G = torch.from_numpy(wg.gen("bench_tcn_heads.G", (B, CLASSES))).cuda()
    rows = {}
    for name in a.heads.split(","):
        h = make(name, 0.2).eval()
        with torch.no_grad():
            eager_us = timed(lambda: h(x, ln, B), a.iters)
            plan = StepPlan(lambda v: h(v, ln, B), x.clone())
            plan_us = timed(lambda: plan(x), a.iters)
            eval_launches = plan.launches
            plan.close()
        h.train()
        opt = torch.optim.Adam(h.parameters(), lr=torch.tensor(1e-4, device="cuda"), capturable=True, fused=True)

        def one(xb, lb):
            opt.zero_grad(set_to_none=True)
            av.prepare_weights(h)
            l = (h.forward_train(xb, lb, 0.2) * G).sum()
            l.backward()
            opt.step()
            return l
        train_calls = count_dlip_calls(lambda: one(x, ln))
        tsg = TrainStepGraph(one, eager_steps=1)
        train_us = timed(lambda: tsg.step(x, ln), a.iters)
        tsg.finish()
        rows[name] = {"eval_plan_us": round(plan_us, 1), "eval_eager_us": round(eager_us, 1), "eval_launches": eval_launches,
                      "train_step_us": round(train_us, 1), "train_dlip_calls": train_calls,
                      "params": sum(p.numel() for p in h.parameters())}
        print(f"{name:11s} eval {plan_us:8.1f} us replayed ({eager_us:8.1f} eager), {eval_launches:3d} launches | "
              f"train step {train_us:8.1f} us replayed, {train_calls:4d} dlip calls | {rows[name]['params']} parameters", flush=True)
    print(json.dumps({"B": B, "T": T, "C_in": CIN, "arith": a.arith, "heads": rows}))


if __name__ == "__main__":
    main()
