#!/usr/bin/env python3
"""Cohort score normalisation at GRID's size: U = 25 834 distinct utterances, D = 512, adaptive S-norm with K = 300, cohorts of
Nc = 1 024 / 4 096 / 16 384 rows (EXPERIMENTS R8.1).  Per cohort size, in ms (device events around back-to-back
launches, the median of --repeats interleaved rounds after a warm-up round):

  topk_stats (chunk)          dlip_topk_stats_f32 alone on one chunk of the score matrix ([chunk_rows, Nc], what cohort_stats hands it)
  GEMM (chunk)                the exact-fp32 GEMM that fills that chunk, alone
  cohort_stats                the whole walk over the table: two normalisations, then GEMM + selection per chunk
  normalised_scores           20 000 trials end to end: raw cosines, the rows the trials use, cohort_stats, the normalisation launch

and two yardsticks, neither of them the code under test:

  torch.topk + mean + std     stock torch on the same device matrix (sorted=False; std with correction 0)
  device-to-device copy       the chunk's bytes copied once: the bandwidth ceiling the selection kernel (which reads every byte
                              of the chunk once and writes 8 bytes per row) is read against

The selection kernel's achieved GB/s is chunk bytes over its time; the ratios printed are topk_stats over each yardstick (below 1
against torch.topk = faster than stock torch; against the copy it cannot be below ~0.5, a copy moving every byte twice).

    python tools/bench_score_norm.py [--repeats 7] [--iters 10] [--cohorts 1024 4096 16384] [--rows 25834]

Engine only, one process; prints one line per measurement and one JSON line (the box is named in it)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from deeplip_amd import build, ops, scoring  # noqa: E402

D, K, TRIALS = 512, 300, 20000


def once(fn, iters):
    """ms per call between two events on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cohorts", type=int, nargs="*", default=[1024, 4096, 16384])
    ap.add_argument("--rows", type=int, default=25834)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_score_norm.py measures on a ROCm GPU; there is nothing to time without one")
    g = torch.Generator().manual_seed(0)
    U = a.rows
    cent = torch.randn(200, D, generator=g)
    emb = (cent[torch.randint(0, 200, (U,), generator=g)] + 0.8 * torch.randn(U, D, generator=g)).cuda()
    ia = torch.randint(0, U, (TRIALS,), generator=g).to(torch.int32).cuda()
    ib = torch.randint(0, U, (TRIALS,), generator=g).to(torch.int32).cuda()
    rows = scoring.trial_rows(ia, ib, U)
    out = {"U": U, "D": D, "K": K, "trials": TRIALS, "trial_rows": rows.n_used, "repeats": a.repeats, "iters": a.iters,
           "device": torch.cuda.get_device_name(0), "box": build.box_id(), "cohorts": {}}
    for Nc in a.cohorts:
        cohort = (cent[torch.randint(0, 200, (Nc,), generator=g)] + 0.8 * torch.randn(Nc, D, generator=g)).cuda()
        k = min(K, Nc)
        chunk = ops.cohort_chunk_rows(U, Nc)
        e, c = ops.l2_normalize(emb), ops.l2_normalize(cohort)
        S = ops.linear(e[:chunk], c)                              # the chunk cohort_stats hands the selection kernel
        S2 = torch.empty_like(S)
        nbytes = S.numel() * 4
        legs = {
            "topk_stats (chunk)": lambda: ops.topk_stats(S, k),
            "GEMM (chunk)": lambda: ops.linear(e[:chunk], c, out=S2.view(1, 1, chunk, Nc)),
            "torch.topk + mean + std": lambda: (lambda t: (t.mean(1), t.std(1, correction=0)))(torch.topk(S, k, dim=1, sorted=False).values),
            "device-to-device copy": lambda: S2.copy_(S),
            "cohort_stats": lambda: ops.cohort_stats(emb, cohort, top_k=k),
            "normalised_scores": lambda: scoring.normalised_scores(emb, ia, ib, cohort, "asnorm", k, rows=rows),
        }
        # the two routes agree before either is timed
        m, s = ops.topk_stats(S, k)
        t = torch.topk(S, k, dim=1).values.double()
        assert torch.allclose(m.double(), t.mean(1), rtol=1e-5, atol=1e-7) and torch.allclose(s.double(), t.std(1, correction=0), rtol=1e-5, atol=1e-7)
        for fn in legs.values():                                  # warm-up round: every shape the timed rounds use
            once(fn, 2)
        times = {name: [] for name in legs}
        for _ in range(a.repeats):                                # interleaved: one round times every leg once
            for name, fn in legs.items():
                times[name].append(once(fn, a.iters if "scores" not in name and "cohort_stats" not in name else max(1, a.iters // 5)))
        r = {name: {"ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for name, v in times.items()}
        sel, gemm = r["topk_stats (chunk)"]["ms"], r["GEMM (chunk)"]["ms"]
        r["chunk_rows"], r["chunk_MiB"] = chunk, round(nbytes / 2 ** 20, 1)
        r["topk_stats_GBps"] = round(nbytes / sel / 1e6, 1)
        r["copy_GBps_read_plus_write"] = round(2 * nbytes / r["device-to-device copy"]["ms"] / 1e6, 1)
        r["topk_stats_over_torch_topk"] = round(sel / r["torch.topk + mean + std"]["ms"], 3)
        r["topk_stats_over_copy"] = round(sel / r["device-to-device copy"]["ms"], 3)
        r["gemm_TFLOPs"] = round(2.0 * chunk * Nc * D / gemm / 1e9, 2)
        r["selection_share_of_chunk"] = round(sel / (sel + gemm), 3)
        for name in legs:
            print(f"Nc={Nc:6d} {name:28s} {r[name]['ms']:10.4f} ms  (min {r[name]['min']:.4f}, max {r[name]['max']:.4f})")
        print(f"Nc={Nc:6d} chunk {chunk} rows = {r['chunk_MiB']} MiB; topk_stats {r['topk_stats_GBps']} GB/s read; copy "
              f"{r['copy_GBps_read_plus_write']} GB/s read + write; topk_stats / torch.topk route = {r['topk_stats_over_torch_topk']}; "
              f"topk_stats / copy = {r['topk_stats_over_copy']}; GEMM {r['gemm_TFLOPs']} TFLOP/s; selection = "
              f"{100 * r['selection_share_of_chunk']:.1f} % of GEMM + selection", flush=True)
        out["cohorts"][str(Nc)] = r
        del S, S2, cohort
    print(json.dumps(out))


if __name__ == "__main__":
    main()
