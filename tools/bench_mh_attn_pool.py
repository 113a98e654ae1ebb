#!/usr/bin/env python
"""Multi-head attentive statistics pooling (`pooling: multi_head_attention`) at the sizes a user runs it at: the E-TDNN's
last tensor, C = 1500 channels, T = 278 frames, head widths [100,200,300,400].

  train      B = 256: forward and backward of the pooling STAGE (hidden-layer GEMM + tail) through autograd, the fused route
             (autograd.mh_attentive_stat_pool: one GEMM, the dlip_mh_attn_* kernels with n heads) against the COMPOSITION of single heads:
             one autograd.attentive_stat_pool (the same kernels with n = 1) per head, torch.cat of the results -- x is read n times
             forward and 2 n times backward and autograd adds the heads' dx tensors.  Same parameters, same x, same dy; the two outputs
             are compared before anything is timed.
  extract    B = 64, ragged lengths: MultiHeadAttention.run_ntc against one AttentiveStatPooling.run_ntc per head + torch.cat.
  tail       the three entry points alone on preallocated tensors, and the bytes the algorithm needs over their time:
             scores = hidden once; stat = x once; bwd = x twice + dx + hidden + dhidden + rde.
Device events around each call, interleaved rounds, medians.

    python tools/bench_mh_attn_pool.py [--batch 256] [--extract-batch 64] [--frames 278] [--channels 1500] [--rounds 11] [--out FILE.json]
Prints one JSON line.  Needs a ROCm GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from deeplip_amd import autograd as ag, ops                                # noqa: E402
from deeplip_amd._lib import call                                           # noqa: E402
from deeplip_amd.audio import AttentiveStatPooling, MultiHeadAttention     # noqa: E402
from deeplip_amd.audio_resnet import POOL_EPS                              # noqa: E402

HBM_TB_S = 6.29          # MI355X, measured float4 copy (8.0 TB/s spec)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3      # us


def interleaved(fns, rounds, warm=3, measure=False):
    """``measure``: the callables time their own window and return microseconds."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(f() if measure else timed(f))
    return {k: statistics.median(v) for k, v in t.items()}, {k: (min(v), max(v)) for k, v in t.items()}


def modules(C, widths):
    """The fused module and one single-head module per head holding the same parameters."""
    g = torch.Generator().manual_seed(5)
    pool = MultiHeadAttention(C, len(widths), list(widths))
    with torch.no_grad():
        pool.W.copy_(torch.randn(pool.W.shape, generator=g) / C ** 0.5)
        pool.b.copy_(torch.randn(pool.b.shape, generator=g) * 0.1)
        pool.v.copy_(torch.randn(pool.v.shape, generator=g) * 0.5)
        pool.k.copy_(torch.randn(pool.k.shape, generator=g) * 0.1)
    singles = []
    for h, w in enumerate(widths):
        lo = pool.offsets[h]
        s = AttentiveStatPooling(C, w)
        with torch.no_grad():
            s.W.copy_(pool.W[lo:lo + w]); s.b.copy_(pool.b[:, lo:lo + w]); s.v.copy_(pool.v[lo:lo + w]); s.k.copy_(pool.k[:, h:h + 1])
        singles.append(s.cuda())
    return pool.cuda(), singles


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--extract-batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=278)
    ap.add_argument("--channels", type=int, default=1500)
    ap.add_argument("--widths", type=int, nargs="+", default=[100, 200, 300, 400])
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mh_attn_pool.py needs a ROCm GPU: nothing here is measured on a CPU")
    B, T, C, widths = a.batch, a.frames, a.channels, a.widths
    n, S = len(widths), sum(widths)
    pool, singles = modules(C, widths)
    g = torch.Generator().manual_seed(6)
    out = {"train_shape": [B, T, C], "widths": widths, "x_mbytes": round(B * T * C * 4 / 1e6, 1)}

    # ---- training stage through autograd
    x = (torch.randn((B, T, C), generator=g) * 0.8 + 0.3).cuda().requires_grad_()
    dy = torch.randn((B, n * 2 * C), generator=g).cuda()
    params = list(pool.parameters()) + [p for s in singles for p in s.parameters()]

    def fused_fwd():
        return ag.mh_attentive_stat_pool(x, pool)

    def comp_fwd():
        return torch.cat([ag.attentive_stat_pool(x, s, POOL_EPS) for s in singles], dim=1)

    def clear():
        x.grad = None
        for p in params:
            p.grad = None

    yf, yc = fused_fwd(), comp_fwd()
    yf.backward(dy)
    gx_f = x.grad.clone()
    clear()
    yc.backward(dy)
    out["fused_vs_composition"] = {"y": rel(yf.detach(), yc.detach()), "dx": rel(gx_f, x.grad)}
    del gx_f, yf, yc
    clear()

    def bwd_of(f):
        def measure():                  # the forward builds the graph outside the timed window; the window is backward() alone
            clear()
            y = f()
            return timed(lambda: y.backward(dy))
        return measure

    med_f, spread_f = interleaved({"fused_fwd_us": fused_fwd, "composition_fwd_us": comp_fwd}, a.rounds)
    med_b, spread_b = interleaved({"fused_bwd_us": bwd_of(fused_fwd), "composition_bwd_us": bwd_of(comp_fwd)}, a.rounds, measure=True)
    clear()
    out["train"] = {**{k: round(v, 1) for k, v in {**med_f, **med_b}.items()},
                    "spread_us": {k: [round(v, 1) for v in s] for k, s in {**spread_f, **spread_b}.items()},
                    "fused_over_composition_fwd": round(med_f["fused_fwd_us"] / med_f["composition_fwd_us"], 4),
                    "fused_over_composition_bwd": round(med_b["fused_bwd_us"] / med_b["composition_bwd_us"], 4)}

    # ---- the tail's entry points alone
    xd = x.detach()
    with torch.no_grad():
        hidden = ops.linear(xd.reshape(B * T, C), pool.W.detach().contiguous(), pool.b.detach().reshape(-1).contiguous()).view(B, T, S)
    vv, kk = pool.v.detach().reshape(-1).contiguous(), pool.k.detach().reshape(-1).contiguous()
    alpha = ops.mh_attn_scores(hidden, vv, kk, pool.head_off)
    y = ops.mh_attn_stat_pool(xd, alpha, POOL_EPS)
    dx, dh, rde = torch.empty_like(xd), torch.empty_like(hidden), torch.empty_like(hidden)
    de, dek = torch.empty((B, n, T), device="cuda"), torch.empty((B, n), device="cuda")

    def tail_bwd():
        call("dlip_mh_attn_stat_pool_bwd_f32", xd, hidden, vv, pool.head_off, alpha, y, dy, None, 0, POOL_EPS, dx, dh, rde, de, dek, B, T, C, S, n)

    med, spread = interleaved({"scores_us": lambda: ops.mh_attn_scores(hidden, vv, kk, pool.head_off),
                               "stat_us": lambda: ops.mh_attn_stat_pool(xd, alpha, POOL_EPS), "bwd_us": tail_bwd}, a.rounds)
    xb, hb = xd.numel() * 4, hidden.numel() * 4
    need = {"scores": hb, "stat": xb, "bwd": 3 * xb + 3 * hb}
    out["tail"] = {**{k: round(v, 1) for k, v in med.items()}, "spread_us": {k: [round(v, 1) for v in s] for k, s in spread.items()},
                   "needed_mbytes": {k: round(v / 1e6, 1) for k, v in need.items()},
                   "tb_s": {k: round(need[k] / med[k + "_us"] / 1e6, 2) for k in need},
                   "share_of_measured_hbm": {k: round(need[k] / med[k + "_us"] / 1e6 / HBM_TB_S, 3) for k in need}, "hbm_tb_s": HBM_TB_S}
    del x, xd, hidden, alpha, y, dx, dh, rde, de, dek, dy

    # ---- extraction: a ragged batch
    Be = a.extract_batch
    lens_h = [max(2, T - (b * (2 * T // 3)) // max(Be - 1, 1)) for b in range(Be)]       # T down to T / 3
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    xe = (torch.randn((Be, T, C), generator=g) * 0.8 + 0.3).cuda()

    def comp_extract():
        return torch.cat([s.run_ntc(xe, lens, eps=POOL_EPS) for s in singles], dim=1)

    with torch.no_grad():
        err = rel(pool.run_ntc(xe, lens), comp_extract())
        med, spread = interleaved({"fused_us": lambda: pool.run_ntc(xe, lens), "composition_us": comp_extract}, a.rounds)
    out["extract"] = {"shape": [Be, T, C], "lengths": [min(lens_h), max(lens_h)], "fused_vs_composition_y": err,
                      **{k: round(v, 1) for k, v in med.items()}, "spread_us": {k: [round(v, 1) for v in s] for k, s in spread.items()},
                      "fused_over_composition": round(med["fused_us"] / med["composition_us"], 4)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
