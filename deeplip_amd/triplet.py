"""Triplet selectors with the mining on the device: mirror of the reference's ``models/audio_models/utils.py:18-142``.

The reference's ``FunctionNegativeTripletSelector.get_triplets`` copies the embeddings to the host and walks every
anchor-positive pair in a Python loop (utils.py:101-113).  Here the selector only names a MODE; ``mine`` runs
``dlip_triplet_mine_f32`` (G = X X^T on the fp32 MFMA, one workgroup per anchor row picks a negative per positive) and the
result stays on the device as the dense ``neg [B,B]`` (``neg[a,p]`` = the chosen negative of the pair ``a < p``, ``-1`` = none),
so that a recorded training step can contain it (``deeplip_amd.loss.OnlineTriplet``).  The reference's quirks are kept: mining
reads the RAW dot products (utils.py:93), the anchor of a pair is its lower index (utils.py:103), the value of a candidate is
``(G[a,n] + margin) - G[a,p]``.

``get_triplets(embeddings, labels) -> LongTensor [N,3]`` is there for callers that use a selector directly: this one call reads
back (the row count depends on the data); it is not on the training path.  Rows are ordered by (anchor, positive, negative), the
reference's by Python's ``set`` of labels -- compare as sets.  Where the reference fails (no triplet at all: utils.py:114-118
builds a ragged array) the result is an empty ``[0,3]`` tensor.

The two random selectors draw ``u [B,B]`` from torch's generator (graph-safe Philox offsets, as ``autograd_video.DropoutFn``
does) and take candidate number ``floor(u[a,p] * count)`` in index order; numpy's generator (utils.py:61,68) is not reproduced.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops
from ._lib import DeepLipHipError, call

Tensor = torch.Tensor

MODE_ALL, MODE_HARDEST, MODE_RANDOM, MODE_SEMIHARD = 0, 1, 2, 3
MODES = {"all": MODE_ALL, "hardest": MODE_HARDEST, "random": MODE_RANDOM, "semihard": MODE_SEMIHARD}
MAX_BATCH = 1024

# tests: fill every output / scratch tensor before the launches (NaN, -2) so that an element no kernel wrote shows
DEBUG_PREFILL = False


def _out(shape, device, dtype=torch.float32) -> Tensor:
    t = ops._empty(shape, device, dtype)
    if DEBUG_PREFILL:
        t.fill_(float("nan") if dtype.is_floating_point else -2)
    return t


# ---- the three shipped selection functions (utils.py:56-73): host-side numpy, for callers that use them on their own ----
def hardest_negative(loss_values):
    i = int(np.argmax(loss_values))
    return i if loss_values[i] > 0 else None


def random_hard_negative(loss_values):
    idx = np.where(loss_values > 0)[0]
    return np.random.choice(idx) if len(idx) > 0 else None


def semihard_negative(loss_values, margin):
    idx = np.where(np.logical_and(loss_values < margin, loss_values > 0))[0]
    return np.random.choice(idx) if len(idx) > 0 else None


_FN_MODE = {hardest_negative: MODE_HARDEST, random_hard_negative: MODE_RANDOM, semihard_negative: MODE_SEMIHARD}


class Mined(NamedTuple):
    """What the mining launch leaves on the device."""
    g: Tensor           # [B,B] raw dot products
    rownorm: Tensor     # [B] max(|x_i|, 1e-8)
    neg: Optional[Tensor]   # [B,B] int32 (None for mode all)
    labels: Tensor      # [B] int32
    mode: int


def check_inputs(embeddings: Tensor, labels: Tensor):
    """The limits of the kernels, refused on the host before any launch: fp32 [B,E] on the device, 1 <= B <= 1024 (a row of G and
    the labels sit in LDS), E % 4 == 0 (16-byte loads), labels int64 or int32 [B] on the device."""
    for t, name in ((embeddings, "embeddings"), (labels, "labels")):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise DeepLipHipError(f"{name}: expected a CUDA (ROCm) tensor; deeplip_amd has no CPU path")
    if embeddings.dtype != torch.float32 or embeddings.dim() != 2:
        raise ValueError(f"embeddings: expected float32 [B,E], got {embeddings.dtype} {tuple(embeddings.shape)}")
    B, E = embeddings.shape
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"triplet mining: batch of {B} embeddings, supported 1 .. {MAX_BATCH}")
    if E < 4 or E % 4 != 0:
        raise ValueError(f"triplet mining: embedding dimension {E} is not a positive multiple of 4")
    if labels.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"labels: expected int64 or int32, got {labels.dtype}")
    if labels.dim() != 1 or labels.shape[0] != B:
        raise ValueError(f"labels: expected [{B}], got {tuple(labels.shape)}")
    return B, E


def mine(embeddings: Tensor, labels: Tensor, margin: float, mode: int, u: Optional[Tensor] = None) -> Mined:
    """dlip_triplet_mine_f32.  ``u`` [B,B] fp32 in [0,1): the draws of the random / semi-hard modes (required there)."""
    B, E = check_inputs(embeddings, labels)
    if mode not in (MODE_ALL, MODE_HARDEST, MODE_RANDOM, MODE_SEMIHARD):
        raise ValueError(f"triplet mining: unknown mode {mode}")
    x = embeddings.detach().contiguous()
    lab = labels.detach().to(torch.int32).contiguous()
    if mode in (MODE_RANDOM, MODE_SEMIHARD):
        if u is None:
            raise ValueError("triplet mining: the random and semi-hard modes need the uniform draws u [B,B]")
        ops._req(u, "u")
        if tuple(u.shape) != (B, B):
            raise ValueError(f"u: expected [{B},{B}], got {tuple(u.shape)}")
    else:
        u = None
    g = _out((B, B), x.device)
    rownorm = _out((B,), x.device)
    neg = _out((B, B), x.device, torch.int32) if mode != MODE_ALL else None
    call("dlip_triplet_mine_f32", x, lab, float(margin), int(mode), u, g, rownorm, neg, B, E)
    return Mined(g, rownorm, neg, lab, int(mode))


def loss_forward(m: Mined, margin: float):
    """dlip_triplet_loss_f32 -> (loss, n_triplets, wcount): 0-dim fp32 / int32 device tensors and the backward's weights."""
    B = m.g.shape[0]
    dev = m.g.device
    rowsum = _out((B,), dev, torch.float64)
    rowcnt = _out((B,), dev, torch.int32)
    wcount = _out((B, B), dev, torch.int32)
    loss = _out((1,), dev)
    n = _out((1,), dev, torch.int32)
    call("dlip_triplet_loss_f32", m.g, m.rownorm, m.labels, m.neg, float(margin), m.mode, rowsum, rowcnt, wcount, loss, n, B)
    return loss[0], n[0], wcount


def loss_backward(embeddings: Tensor, m: Mined, wcount: Tensor, n: Tensor, gscale: Optional[Tensor] = None) -> Tensor:
    """dlip_triplet_loss_bwd_f32 -> dX [B,E] (times ``gscale``, a device scalar; None = 1)."""
    x = embeddings.detach().contiguous()
    B, E = x.shape
    mw = _out((B, (B + 15) // 16 * 16), x.device)
    dx = _out((B, E), x.device)
    call("dlip_triplet_loss_bwd_f32", x, m.g, m.rownorm, wcount, n, gscale, mw, dx, B, E)
    return dx


def triplets_from(m: Mined) -> Tensor:
    """The list form [N,3] (anchor, positive, negative) of a mining result.  Reads back (the row count depends on the data)."""
    lab = m.labels
    B = lab.shape[0]
    if m.mode == MODE_ALL:
        same = lab[:, None] == lab[None, :]
        idx = torch.arange(B, device=lab.device)
        pair = same & (idx[None, :] > idx[:, None])                       # [a,p]
        ap = pair.nonzero()
        if ap.shape[0] == 0:
            return torch.zeros((0, 3), dtype=torch.int64, device=lab.device)
        other = ~same[ap[:, 0]]                                           # [pairs, n]: n of another label than a
        pn = other.nonzero()
        return torch.cat([ap[pn[:, 0]], pn[:, 1:2]], dim=1)
    ap = (m.neg >= 0).nonzero()
    return torch.cat([ap, m.neg[ap[:, 0], ap[:, 1]].to(torch.int64)[:, None]], dim=1)


class TripletSelector:
    """utils.py:18-29.  ``mode`` / ``margin`` are what deeplip_amd.loss.OnlineTriplet hands to the mining launch."""
    mode = None
    margin = 0.0

    def __init__(self):
        pass

    def draws(self, embeddings: Tensor) -> Optional[Tensor]:
        """u [B,B] for the modes that draw (torch's generator on the embeddings' device), else None."""
        if self.mode in (MODE_RANDOM, MODE_SEMIHARD):
            B = embeddings.shape[0]
            return torch.rand((B, B), device=embeddings.device, dtype=torch.float32)
        return None

    def mine(self, embeddings: Tensor, labels: Tensor, u: Optional[Tensor] = None) -> Mined:
        if self.mode is None:
            raise NotImplementedError
        check_inputs(embeddings, labels)
        if u is None:
            u = self.draws(embeddings)
        return mine(embeddings, labels, self.margin, self.mode, u)

    def get_triplets(self, embeddings, labels, u: Optional[Tensor] = None):
        return triplets_from(self.mine(embeddings, labels, u))


class AllTripletSelector(TripletSelector):
    """utils.py:32-53: every (a, p, n) with a < p of one label and n of another."""
    mode = MODE_ALL

    def __init__(self):
        super().__init__()


class FunctionNegativeTripletSelector(TripletSelector):
    """utils.py:76-121.  ``negative_selection_fn`` must be one of the three shipped functions (``hardest_negative``,
    ``random_hard_negative``, ``semihard_negative``): each names a mode of the mining kernel; any other callable would have to run on
    the host per pair and raises NotImplementedError.  ``cpu`` is accepted and ignored: the embeddings never leave the device."""

    def __init__(self, margin, negative_selection_fn, cpu=True):
        super().__init__()
        self.cpu = cpu
        self.margin = margin
        self.negative_selection_fn = negative_selection_fn
        try:
            self.mode = _FN_MODE[negative_selection_fn]
        except (KeyError, TypeError):
            raise NotImplementedError("FunctionNegativeTripletSelector: only hardest_negative, random_hard_negative and semihard_negative "
                                      "run on the device; an arbitrary selection function is not supported") from None


def HardestNegativeTripletSelector(margin, cpu=False):
    return FunctionNegativeTripletSelector(margin=margin, negative_selection_fn=hardest_negative, cpu=cpu)


def RandomNegativeTripletSelector(margin, cpu=False):
    return FunctionNegativeTripletSelector(margin=margin, negative_selection_fn=random_hard_negative, cpu=cpu)


def SemihardNegativeTripletSelector(margin, cpu=False):
    return FunctionNegativeTripletSelector(margin=margin, negative_selection_fn=semihard_negative, cpu=cpu)


SELECTORS = {"hardest": HardestNegativeTripletSelector, "semihard": SemihardNegativeTripletSelector,
             "random": RandomNegativeTripletSelector, "all": lambda margin, cpu=False: AllTripletSelector()}


def make_selector(name: str, margin: float) -> TripletSelector:
    """``train.triplet.selector`` -> a selector; an unknown name is a ValueError."""
    if name not in SELECTORS:
        raise ValueError(f"triplet selector {name!r}: expected one of {sorted(SELECTORS)}")
    return SELECTORS[name](margin)
