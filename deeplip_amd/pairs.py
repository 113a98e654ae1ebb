"""Pair selectors of the online contrastive loss, the selection on the device (``deeplip_amd.loss.Contrastive``).

The reference adapted its triplet loss to cosine scores and took its selectors from adambielski/siamese-triplet
(models/audio_models/utils.py:18-142); the contrastive counterpart there is ``OnlineContrastiveLoss(margin, pair_selector)``.
Upstream leaves ``Contrastive`` empty (loss.py:69-75), so the selectors are the build's own: a selector only names a MODE of
``dlip_contrastive_loss_f32`` (G = X X^T on the fp32 MFMA, then one workgroup per anchor row selects among the columns behind it) and
nothing is read back on the training path, so that a recorded step can contain the criterion.

``get_pairs(embeddings, labels) -> (positive_pairs [P,2], negative_pairs [N,2])`` (LongTensors, rows ``i < j`` in index order) is there
for callers that use a selector on its own: this one call reads back (the row counts depend on the data).

Tests fill every output and scratch tensor before the launches (NaN, -2) through ``deeplip_amd.triplet.DEBUG_PREFILL``, as the triplet
launches do.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import triplet as tp
from ._lib import call

Tensor = torch.Tensor

MODE_ALL, MODE_HARD_NEGATIVE = 0, 1
MODES = {"all": MODE_ALL, "hard_negative": MODE_HARD_NEGATIVE}


class PairLoss(NamedTuple):
    """What dlip_contrastive_loss_f32 leaves on the device."""
    loss: Tensor        # 0-dim fp32
    n: Tensor           # 0-dim int32: the selected pairs
    g: Tensor           # [B,B] raw dot products
    rownorm: Tensor     # [B] max(|x_i|, 1e-8)
    w: Tensor           # [B,B] int32: -1 positive pair, +1 selected negative with an active hinge, 0 otherwise
    sel: Optional[Tensor]   # [B,B] int32: 1 positive pair, 2 selected negative, 0 otherwise (None unless asked for)


def loss_forward(embeddings: Tensor, labels: Tensor, margin: float, mode: int, want_sel: bool = False) -> PairLoss:
    """dlip_contrastive_loss_f32 under ``triplet.check_inputs``' limits (fp32 [B,E], 1 <= B <= 1024, E % 4 == 0, labels int32 or int64),
    refused on the host before any launch."""
    B, E = tp.check_inputs(embeddings, labels)
    if mode not in (MODE_ALL, MODE_HARD_NEGATIVE):
        raise ValueError(f"pair selection: unknown mode {mode}")
    x = embeddings.detach().contiguous()
    lab = labels.detach().to(torch.int32).contiguous()
    dev = x.device
    g = tp._out((B, B), dev)
    rownorm = tp._out((B,), dev)
    rowsum = tp._out((B,), dev, torch.float64)
    rowcnt = tp._out((B,), dev, torch.int32)
    w = tp._out((B, B), dev, torch.int32)
    sel = tp._out((B, B), dev, torch.int32) if want_sel else None
    loss = tp._out((1,), dev)
    n = tp._out((1,), dev, torch.int32)
    call("dlip_contrastive_loss_f32", x, lab, float(margin), int(mode), g, rownorm, rowsum, rowcnt, w, sel, loss, n, B, E)
    return PairLoss(loss[0], n[0], g, rownorm, w, sel)


def loss_backward(embeddings: Tensor, p: PairLoss, gscale: Optional[Tensor] = None) -> Tensor:
    """dX [B,E] (times ``gscale``, a device scalar; None = 1): with the signed weights ``w`` the gradient is the one
    dlip_triplet_loss_bwd_f32 computes -- M_ij = (w_ij + w_ji) g / (N r_i r_j), the diagonal correction, dX = M X -- so that launch is
    reused unchanged (``wcount`` = w, ``n_triplets`` = n_pairs)."""
    return tp.loss_backward(embeddings, tp.Mined(p.g, p.rownorm, None, None, 0), p.w, p.n, gscale)


class PairSelector:
    """``mode`` is what deeplip_amd.loss.Contrastive hands to the launch."""
    mode = None

    def __init__(self):
        pass

    def get_pairs(self, embeddings: Tensor, labels: Tensor):
        if self.mode is None:
            raise NotImplementedError
        sel = loss_forward(embeddings, labels, 0.0, self.mode, want_sel=True).sel      # (the selection does not depend on the margin)
        return (sel == 1).nonzero(), (sel == 2).nonzero()


class AllPairSelector(PairSelector):
    """Every pair ``i < j``: positive where the labels agree, negative otherwise (adambielski's AllPositivePairSelector with
    ``balance=False``)."""
    mode = MODE_ALL


class HardNegativePairSelector(PairSelector):
    """Every positive pair ``a < p``, and per anchor row ``a`` the hardest negatives: with P_a = #{p > a : label_p = label_a} the
    min(P_a, #negatives after a) negatives ``n > a`` of highest cos(a, n), the lower index winning ties.  This is a PER-ROW form of
    adambielski's balanced HardNegativePairSelector (which takes the len(positive_pairs) closest negative pairs of the whole batch):
    chosen because a row of the cosine matrix fits in LDS, so one workgroup selects exactly with no pass over the whole matrix and no
    read-back; the batch keeps as many negatives as positives except where a row runs out of later negatives."""
    mode = MODE_HARD_NEGATIVE


SELECTORS = {"all": AllPairSelector, "hard_negative": HardNegativePairSelector}


def make_pair_selector(name: str) -> PairSelector:
    """``train.contrastive.selector`` -> a selector; an unknown name is a ValueError."""
    if name not in SELECTORS:
        raise ValueError(f"pair selector {name!r}: expected one of {sorted(SELECTORS)}")
    return SELECTORS[name]()
