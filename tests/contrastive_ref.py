"""Shared by test_contrastive_cpu.py and test_contrastive_gpu.py: the cases, their inputs and the restatement of the online contrastive
loss in torch on the CPU, in fp64 (the reference) and in fp32 (the yardstick of the bars).  Upstream has no implementation."""
import functools

import numpy as np
import torch

from deeplip_amd import weightgen as wg

CASES = {"b64_g1": (64, 8, 64, 1.0), "b64_g002": (64, 8, 64, 0.02), "b256_g01": (256, 57, 512, 0.1), "b60_g01": (60, 57, 512, 0.1),
         "b33": (33, 5, 20, 1.0)}                                       # name -> (B, S, E, gain)
MARGIN = 0.1                # every case: >= 1 % of the negative pairs active, none within 50 x cos_err of the margin (asserted on the CPU)
MARGIN_CLEAR, FRAGILE_FACTOR, FRAGILE_SHARE = 50.0, 100.0, 0.05
BAR_LOSS, BAR_GRAD = 2e-5, 1e-4


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """The formula of the triplet tests: x = gain * (0.2 * centre[label] + noise)."""
    B, S, E, gain = CASES[name]
    labels = np.minimum((wg.gen(f"contrastive.{name}.labels", (B,), kind="uniform") * S).astype(np.int64), S - 1)
    centres = wg.gen(f"contrastive.{name}.centres", (S, E))
    noise = wg.gen(f"contrastive.{name}.noise", (B, E))
    x = (np.float32(gain) * (np.float32(0.2) * centres[labels] + noise)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(labels)


def cosines(x, dtype):
    x = x.to(dtype)
    r = x.norm(dim=1).clamp_min(1e-8)
    return (x @ x.T) / (r[:, None] * r[None, :])


def select64(x, labels, mode):
    """The selection in fp64: (positive pairs, negative pairs, rows) -- rows[a] = (K, candidates in selection order, their cosines) for
    the hard mode's rows that have a choice to make (0 < K < #candidates)."""
    C = cosines(x, torch.float64).numpy()
    lab = np.asarray(labels)
    B = len(lab)
    pos, neg, rows = [], [], {}
    for a in range(B):
        later = np.arange(a + 1, B)
        p = later[lab[later] == lab[a]]
        n = later[lab[later] != lab[a]]
        pos += [(a, int(j)) for j in p]
        if mode == "all":
            neg += [(a, int(j)) for j in n]
            continue
        K = min(len(p), len(n))
        order = n[np.lexsort((n, -C[a, n]))]                  # cosine descending, the lower index first among equals
        neg += [(a, int(j)) for j in order[:K]]
        if 0 < K < len(n):
            rows[a] = (K, order, C[a, order])
    return pos, neg, rows


def restate(x, pos, neg, margin, dtype):
    """(loss, dX) of the definition on the given pair sets: mean over all pairs of 1 - cos (positive) / relu(cos - margin) (negative)."""
    xx = x.to(dtype).clone().requires_grad_()
    if len(pos) + len(neg) == 0:
        return 0.0, np.zeros(tuple(x.shape))
    r = xx.norm(dim=1).clamp_min(1e-8)
    C = (xx @ xx.T) / (r[:, None] * r[None, :])
    terms = []
    if len(pos):
        p = torch.as_tensor(np.asarray(pos), dtype=torch.int64)
        terms.append(1 - C[p[:, 0], p[:, 1]])
    if len(neg):
        n = torch.as_tensor(np.asarray(neg), dtype=torch.int64)
        terms.append(torch.relu(C[n[:, 0], n[:, 1]] - margin))
    loss = torch.cat(terms).mean()
    loss.backward()
    return float(loss.detach()), xx.grad.double().numpy()


@functools.lru_cache(maxsize=None)
def case_facts(name):
    """What the conditions on a case are stated in: cos_err (the fp32 restatement's worst cosine error), the share of negative pairs
    that are active at MARGIN, the distance of the nearest negative cosine from MARGIN, and the hard mode's fragile rows."""
    x, labels = case_inputs(name)
    C64 = cosines(x, torch.float64).numpy()
    cos_err = float(np.abs(cosines(x, torch.float32).double().numpy() - C64).max())
    lab = labels.numpy()
    iu = np.triu_indices(len(lab), 1)
    negc = C64[iu][lab[iu[0]] != lab[iu[1]]]
    _, _, rows = select64(x, labels, "hard_negative")
    fragile = sorted(a for a, (K, order, c) in rows.items() if c[K - 1] - c[K] < FRAGILE_FACTOR * cos_err)
    return {"cos_err": cos_err, "active": float((negc > MARGIN).mean()), "clear": float(np.abs(negc - MARGIN).min()), "rows": len(rows),
            "fragile": fragile}


def rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(scale if scale is not None else np.abs(b).max(), 1e-30))
