#!/usr/bin/env python3
"""Capture golden vectors of the REFERENCE's OnlineTriplet criterion and triplet selectors (models/audio_models/loss.py:18-31,
utils.py:18-142); run in the build container only, like capture_tcn_heads_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_triplet_golden.py

Imports ``models.audio_models.loss`` / ``.utils`` from the reference checkout (read-only; ``kaldiio``, which utils.py:2 imports and
nothing here uses, is replaced by an empty stand-in module) and writes DATA only to ``triplet_golden.npz``.  Inputs come from
``deeplip_amd.weightgen`` (``case_inputs`` below; tests/test_triplet_gpu.py restates the same formula and checks ``<case>.x_probe``):

  cases                     json: name -> {B, S, E, gain}; margin (one value for mining and loss)
  <case>.labels             int64 [B];  <case>.x_probe = x[:2, :8]
  <case>.dot_err            max OFF-DIAGONAL |G_fp32 - G_fp64| of the reference's own F.linear(x, x) (mining never reads the diagonal)
  <case>.pairs, <case>.gap  every anchor-positive pair a < p [P,2] and its fp64 gap = min(best v - second best v, |best v|),
                            v_n = G[a,n] + margin - G[a,p] over the negatives n (one negative: |best v|)
  <case>.<sel>.triplets / .triplets64          the selector's [N,3] from fp32 / fp64 embeddings (.triplets64 only where it differs;
                                               sel = hardest, all; ``all`` of the
                                               B = 256 cases stores ``.n`` only: its rows follow from the labels)
  <case>.<sel>.loss / .loss64, .n              OnlineTriplet's loss and len(triplets)
  <case>.<sel>.dx / .dx64                      d loss / d embeddings (rows ``<case>.dx_rows``: 16 of them where B E > 4096), .dx_absmax / .dx64_absmax,
                                               .dx_norm / .dx64_norm of the whole tensor
  onelabel.*                one label holds the whole batch: the reference fails there (no negatives); inputs and n = 0 only
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DEEPLIP_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deeplip_amd import weightgen as wg  # noqa: E402

sys.path = [p for p in sys.path if os.path.realpath(p or os.getcwd()) != os.path.realpath(ROOT)]
sys.path.insert(0, REF)
for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
    del sys.modules[m]
sys.modules.setdefault("kaldiio", types.ModuleType("kaldiio"))
from models.audio_models import loss as ref_loss, utils as ref_utils  # noqa: E402
assert os.path.realpath(ref_utils.__file__).startswith(os.path.realpath(REF)), "reference not imported"

torch.set_num_threads(8)
MARGIN = 0.2
CASES = {
    "b64_g1": dict(B=64, S=8, E=64, gain=1.0),
    "b64_g002": dict(B=64, S=8, E=64, gain=0.02),
    "b256_g01": dict(B=256, S=57, E=512, gain=0.1),
    "b256_g1": dict(B=256, S=57, E=512, gain=1.0),
    "b60_g01": dict(B=60, S=57, E=512, gain=0.1),
    "onelabel": dict(B=32, S=1, E=64, gain=0.1),
}
DX_ROWS = 16
FRAGILE_FACTOR, FRAGILE_SHARE = 100.0, 0.02


def case_inputs(name, B, S, E, gain):
    """x = gain * (0.2 * centre[label] + noise), centres and noise standard normal from weightgen; labels = floor(S * uniform)."""
    labels = np.minimum((wg.gen(f"triplet.{name}.labels", (B,), kind="uniform") * S).astype(np.int64), S - 1)
    centres = wg.gen(f"triplet.{name}.centres", (S, E))
    noise = wg.gen(f"triplet.{name}.noise", (B, E))
    x = (np.float32(gain) * (np.float32(0.2) * centres[labels] + noise)).astype(np.float32)
    return x, labels


def run(sel, x, labels):
    crit = ref_loss.OnlineTriplet(MARGIN, sel)
    xt = x.clone().requires_grad_()
    sel_t = sel.get_triplets(xt, labels)
    loss, n = crit(xt, labels)
    loss.backward()
    assert n == len(sel_t)
    return sel_t.numpy().astype(np.int16), loss.detach().numpy(), xt.grad.numpy(), n


def main():
    out = {"cases": np.array(json.dumps({"margin": MARGIN, "cases": CASES}))}
    for name, c in CASES.items():
        x, labels = case_inputs(name, **c)
        B = c["B"]
        out[f"{name}.labels"] = labels
        out[f"{name}.x_probe"] = x[:2, :8].copy()
        if c["S"] == 1:
            out[f"{name}.n"] = np.array(0, dtype=np.int64)
            continue
        xt, lt = torch.from_numpy(x), torch.from_numpy(labels)
        g32 = torch.nn.functional.linear(xt, xt).double().numpy()
        g64 = torch.nn.functional.linear(xt.double(), xt.double()).numpy()
        off = ~np.eye(B, dtype=bool)
        dot_err = float(np.abs(g32 - g64)[off].max())
        out[f"{name}.dot_err"] = np.array(dot_err)
        pairs, gaps = [], []
        for a in range(B):
            negs = np.where(labels != labels[a])[0]
            for p in range(a + 1, B):
                if labels[p] != labels[a] or len(negs) == 0:
                    continue
                v = np.sort(g64[a, negs] + MARGIN - g64[a, p])[::-1]
                gaps.append(min(v[0] - v[1], abs(v[0])) if len(v) > 1 else abs(v[0]))
                pairs.append((a, p))
        out[f"{name}.pairs"] = np.array(pairs, dtype=np.int16).reshape(-1, 2)
        out[f"{name}.gap"] = np.array(gaps, dtype=np.float64)
        share = float((np.array(gaps) < FRAGILE_FACTOR * dot_err).mean()) if gaps else 0.0
        print(f"{name}: {len(pairs)} pairs, dot_err {dot_err:.3e}, smallest gap {min(gaps) if gaps else float('nan'):.3e}, "
              f"fragile share {share:.4f}")
        assert share <= FRAGILE_SHARE, (name, share)
        rows = np.arange(B) if B * c["E"] <= 4096 else np.linspace(0, B - 1, DX_ROWS).astype(np.int64)
        out[f"{name}.dx_rows"] = rows
        for sname, sel in (("hardest", ref_utils.HardestNegativeTripletSelector(MARGIN)), ("all", ref_utils.AllTripletSelector())):
            t32, l32, d32, n32 = run(sel, xt, lt)
            t64, l64, d64, n64 = run(sel, xt.double(), lt)
            k = f"{name}.{sname}"
            if sname == "all":
                assert n32 == n64
            out[k + ".n"] = np.array(n32, dtype=np.int64)
            out[k + ".n64"] = np.array(n64, dtype=np.int64)
            if not (sname == "all" and B > 64):
                out[k + ".triplets"] = t32
                if not np.array_equal(t32, t64):
                    out[k + ".triplets64"] = t64
            out[k + ".loss"], out[k + ".loss64"] = l32, l64
            out[k + ".dx"], out[k + ".dx64"] = d32[rows], d64[rows]
            out[k + ".dx_absmax"], out[k + ".dx64_absmax"] = np.array(np.abs(d32).max()), np.array(np.abs(d64).max())
            out[k + ".dx_norm"], out[k + ".dx64_norm"] = np.array(np.linalg.norm(d32.astype(np.float64))), np.array(np.linalg.norm(d64))
            print(f"  {sname}: n {n32} (fp64 {n64}), loss {float(l32):.6f} (fp64 {float(l64):.6f})")
    path = os.path.join(HERE, "triplet_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
