"""Speaker-classification criteria on the HIP engine: mirror of the reference's
``models/audio_models/loss.py`` (LMCL = CosFace / AM-softmax, CrossEntropy, OnlineTriplet), plus the build's own definitions of the
three classes upstream leaves empty (AAMSoftmax, ASoftmax, Contrastive).

``forward(embeddings, labels) -> (loss, logits)`` exactly as the reference; both values come from
``dlip_logits_argmax_f32`` + ``dlip_margin_ce_loss_f32``.  ``predict`` adds the first-max argmax
(torch.max(logits, 1)[1], train_fusion.py:296) from the same launch.  With grad enabled, forward
goes through deeplip_amd/autograd.py (HIP forward + backward kernels) so the criterion trains
(config C5).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from . import ops
from .holders import LinearParams


class LMCL(nn.Module):
    """loss.py:33-51.  ``margin`` is a plain attribute the trainers mutate (train_fusion.py:137-141)."""

    def __init__(self, embedding_size, num_classes, s, margin):
        super().__init__()
        self.embedding_size, self.num_classes = embedding_size, num_classes
        self.s, self.margin = s, margin
        self.weights = nn.Parameter(torch.Tensor(num_classes, embedding_size))
        nn.init.kaiming_normal_(self.weights)

    def predict(self, embeddings, labels=None):
        w = self.weights.detach().contiguous()
        logits, amax = ops.logits_argmax(embeddings.contiguous(), w, cosine=True)
        loss = None
        if labels is not None:
            loss = ops.margin_ce_loss(logits, labels.contiguous(), float(self.s), float(self.margin))
            loss = loss + ops.l1_sum(w) * 0.00001      # L1 regulariser 1e-5*||W||_1 (loss.py:49-50)
        return loss, logits, amax

    def forward(self, embeddings, labels):
        if torch.is_grad_enabled() and (self.weights.requires_grad or embeddings.requires_grad):
            from . import autograd as ag       # differentiable path (training)
            logits = ag.linear(ag.l2_normalize(embeddings), ag.l2_normalize(self.weights))
            loss = ag.margin_ce_loss(logits, labels, self.s, self.margin)
            loss = loss + ag.l1_norm(self.weights, 0.00001)       # L1 term (loss.py:49-50)
            return loss, logits
        loss, logits, _ = self.predict(embeddings, labels)
        return loss, logits


class AAMSoftmax(nn.Module):
    """Additive angular margin softmax (ArcFace).  Upstream `AAMSoftmax` is an empty TODO stub (loss.py:62-67) that
    the north star nevertheless names, so this is the published recipe (parity unpinned) behind the interface of
    the reference's LMCL: ``forward(embeddings, labels) -> (loss, cosine logits)``.
    loss = CE(s * [cos(theta_y + m) on the target, cos(theta_j) elsewhere]); cos(theta + m) where theta + m < pi,
    else cos(theta) - m sin(pi - m); ``easy_margin`` applies the margin only where cos(theta) > 0."""

    def __init__(self, embedding_size, num_classes, s=30.0, margin=0.2, easy_margin=False):
        super().__init__()
        self.embedding_size, self.num_classes = embedding_size, num_classes
        self.s, self.margin, self.easy_margin = s, margin, easy_margin
        self.weights = nn.Parameter(torch.Tensor(num_classes, embedding_size))
        nn.init.kaiming_normal_(self.weights)

    def predict(self, embeddings, labels=None):
        from . import autograd as ag
        w = self.weights.detach().contiguous()
        logits, amax = ops.logits_argmax(embeddings.detach().contiguous(), w, cosine=True)
        loss = None
        if labels is not None:
            with torch.no_grad():
                loss = ops.margin_ce_loss(ag.aam_margin(logits, labels, self.margin, self.easy_margin), labels.contiguous(),
                                          float(self.s), 0.0)
        return loss, logits, amax

    def forward(self, embeddings, labels):
        if torch.is_grad_enabled() and (self.weights.requires_grad or embeddings.requires_grad):
            from . import autograd as ag
            logits = ag.linear(ag.l2_normalize(embeddings), ag.l2_normalize(self.weights))
            loss = ag.margin_ce_loss(ag.aam_margin(logits, labels, self.margin, self.easy_margin), labels, self.s, 0.0)
            return loss, logits
        loss, logits, _ = self.predict(embeddings, labels)
        return loss, logits


class CrossEntropy(nn.Module):
    """loss.py:6-16: Linear + CE(logits + 1e-8)."""

    def __init__(self, embedding_size, num_classes):
        super().__init__()
        self.embedding_size, self.num_classes = embedding_size, num_classes
        self.fc = LinearParams(embedding_size, num_classes)

    def predict(self, embeddings, labels=None):
        logits, amax = ops.logits_argmax(embeddings.contiguous(), self.fc.weight.detach().contiguous(),
                                         self.fc.bias.detach().contiguous(), cosine=False)
        loss = ops.margin_ce_loss(logits, labels.contiguous(), 1.0, 0.0) if labels is not None else None
        return loss, logits, amax

    def forward(self, embeddings, labels):
        if torch.is_grad_enabled() and (self.fc.weight.requires_grad or embeddings.requires_grad):
            from . import autograd as ag
            logits = ag.linear(embeddings, self.fc.weight, self.fc.bias)
            return ag.margin_ce_loss(logits, labels, 1.0, 0.0), logits
        loss, logits, _ = self.predict(embeddings, labels)
        return loss, logits


class OnlineTriplet(nn.Module):
    """loss.py:18-31: ``forward(embeddings, labels) -> (loss, n_triplets)`` with ``triplet_selector`` one of
    deeplip_amd.triplet's selectors (the reference's names and constructors).  The selector names the mining mode; mining, loss and
    backward are dlip_triplet_* launches that never leave the device, so a recorded training step can contain the criterion:
    ``loss`` is a 0-dim fp32 device tensor (mean over the triplets of relu(cos(a,n) - cos(a,p) + margin)), ``n_triplets`` a 0-dim int32
    device tensor (``int(n)`` is the reference's ``len(triplets)``; it synchronises, keep it out of a step).  With grad enabled the
    call goes through ``autograd.TripletLossFn``; under ``torch.no_grad()`` the same forward launches run.

    Zero triplets (no label twice in the batch, one label only, or no pair with a candidate): the reference's selector builds a
    ragged array and fails (utils.py:114-118); here loss = 0, n_triplets = 0 and the gradient is all zeros -- no division by zero.
    No parameters.  CPU tensors are refused (DeepLipHipError); E % 4 != 0, B > 1024 and float labels raise ValueError before any
    launch."""

    def __init__(self, margin, triplet_selector):
        super().__init__()
        from . import triplet as tp
        if not isinstance(triplet_selector, tp.TripletSelector) or triplet_selector.mode is None:
            raise TypeError("OnlineTriplet: triplet_selector must be one of deeplip_amd.triplet's selectors (AllTripletSelector, "
                            "HardestNegativeTripletSelector, RandomNegativeTripletSelector, SemihardNegativeTripletSelector)")
        self.margin = margin
        self.triplet_selector = triplet_selector

    def forward(self, embeddings, labels, u=None):
        from . import autograd as ag, triplet as tp
        tp.check_inputs(embeddings, labels)
        sel = self.triplet_selector
        if u is None:
            u = sel.draws(embeddings)
        if torch.is_grad_enabled() and embeddings.requires_grad:
            return ag.triplet_loss(embeddings, labels, self.margin, sel.margin, sel.mode, u)
        loss, n, _ = tp.loss_forward(tp.mine(embeddings, labels, sel.margin, sel.mode, u), float(self.margin))
        return loss, n


class ASoftmax(nn.Module):
    """A-Softmax (SphereFace, Liu et al. 2017).  Upstream `ASoftmax` is an empty TODO stub (loss.py:53-59) that the config comment
    nevertheless lists (conf/audio_config.yaml:130), so the definition is the build's own (parity unpinned) behind the
    interface of the reference's LMCL: ``forward(embeddings, labels) -> (loss, cosine logits)``.

    With c_bj = cos(theta_bj) the cosine logits and r_b = |x_b| (clamped below as ``l2_normalize`` clamps it) the cross-entropy sees
    z_bj = r_b c_bj off the target and z_by = r_b (lambda c + psi(c)) / (1 + lambda) on it, psi(c) = (-1)^k T_m(c) - 2k, T_m the
    Chebyshev polynomial (c, 2c^2 - 1, 4c^3 - 3c, 8c^4 - 8c^2 + 1 for m = 1 .. 4), k = #{ j in 1 .. m-1 : c <= cos(j pi / m) }, c
    clamped to [-1, 1].  loss = mean_b CE(z_b, y_b): no scale ``s``, no L1 term.  psi is continuous and psi' vanishes at every
    branch point, so no case is fragile.

    lambda lives in a 1-element fp32 device buffer (non-persistent: the state dict holds ``weights`` alone, as LMCL's) that the
    kernels read through the pointer, so a recorded step follows the schedule without being recorded again.  ``anneal(it=None)``
    writes max(lambda_min, lambda_base (1 + gamma it)^(-power)) into it on the current stream (call it outside a capture);
    ``it=None`` advances the criterion's own counter and uses the new count (SphereFace's order: the first step runs at it = 1).
    ``forward`` never changes lambda; ``set_lambda(value)`` fixes it by hand.  ``margin`` = m (the trainer keys recorded steps by it)."""

    def __init__(self, embedding_size, num_classes, m=4, lambda_min=5.0, lambda_base=1000.0, gamma=0.12, power=1.0):
        super().__init__()
        if isinstance(m, bool) or m not in (1, 2, 3, 4):
            raise ValueError(f"ASoftmax: m = {m!r}, supported 1, 2, 3, 4")
        self.embedding_size, self.num_classes = embedding_size, num_classes
        self.m = self.margin = int(m)
        self.lambda_min, self.lambda_base, self.gamma, self.power = float(lambda_min), float(lambda_base), float(gamma), float(power)
        self.it = 0
        self.weights = nn.Parameter(torch.Tensor(num_classes, embedding_size))
        nn.init.kaiming_normal_(self.weights)
        self.register_buffer("lam", torch.full((1,), self.schedule(0), dtype=torch.float32), persistent=False)

    def schedule(self, it) -> float:
        """lambda at iteration ``it``: max(lambda_min, lambda_base (1 + gamma it)^(-power))."""
        return max(self.lambda_min, self.lambda_base * (1.0 + self.gamma * float(it)) ** (-self.power))

    def anneal(self, it=None) -> float:
        if it is None:
            self.it += 1
            it = self.it
        return self.set_lambda(self.schedule(it))

    def set_lambda(self, value) -> float:
        self.lam.fill_(float(value))         # one fill launch on the current stream: nothing is read back
        return float(value)

    def predict(self, embeddings, labels=None):
        w = self.weights.detach().contiguous()
        x = embeddings.detach().contiguous()
        logits, amax = ops.logits_argmax(x, w, cosine=True)
        loss = None
        if labels is not None:
            lab = labels.to(torch.int64).contiguous()
            loss = ops.margin_ce_loss(ops.asoftmax_logits(logits, ops.row_norm(x), lab, self.lam, self.m), lab, 1.0, 0.0)
        return loss, logits, amax

    def forward(self, embeddings, labels):
        if torch.is_grad_enabled() and (self.weights.requires_grad or embeddings.requires_grad):
            from . import autograd as ag
            logits = ag.linear(ag.l2_normalize(embeddings), ag.l2_normalize(self.weights))
            lab = labels.to(torch.int64)
            z = ag.asoftmax_logits(logits, ag.row_norm(embeddings), lab, self.lam, self.m)
            return ag.margin_ce_loss(z, lab, 1.0, 0.0), logits
        loss, logits, _ = self.predict(embeddings, labels)
        return loss, logits


class Contrastive(nn.Module):
    """Online contrastive loss on cosines, the pairs selected on the device.  Upstream `Contrastive` is an empty TODO stub
    (loss.py:69-75) that the config comment lists (conf/audio_config.yaml:130); the definition is the build's own (parity unpinned;
    DESIGN.md 3g): the cosine form of adambielski/siamese-triplet's ``OnlineContrastiveLoss(margin, pair_selector)`` -- the source of
    the reference's triplet selectors --, i.e. torch.nn.CosineEmbeddingLoss on the selected pairs: a positive pair (one label) costs
    1 - cos_ij, a negative pair relu(cos_ij - margin), cos_ij = x_i.x_j / (max(|x_i|, 1e-8) max(|x_j|, 1e-8)); ``loss`` is the mean
    over all selected pairs (inactive negatives count in the denominator).

    ``forward(embeddings, labels) -> (loss, n_pairs)``: 0-dim fp32 and int32 device tensors with OnlineTriplet's contract -- nothing is
    read back, so a recorded training step can contain the criterion (``int(n_pairs)`` synchronises, keep it out of a step).  Zero
    selected pairs: loss = 0, n_pairs = 0, an all-zero gradient.  ``pair_selector``: one of deeplip_amd.pairs' selectors.  No
    parameters.  CPU tensors are refused (DeepLipHipError); E % 4 != 0, B > 1024 and float labels raise ValueError before any launch."""

    def __init__(self, margin, pair_selector):
        super().__init__()
        from . import pairs as pr
        if not isinstance(pair_selector, pr.PairSelector) or pair_selector.mode is None:
            raise TypeError("Contrastive: pair_selector must be one of deeplip_amd.pairs' selectors (AllPairSelector, "
                            "HardNegativePairSelector)")
        self.margin = margin
        self.pair_selector = pair_selector

    def forward(self, embeddings, labels):
        from . import autograd as ag, pairs as pr, triplet as tp
        tp.check_inputs(embeddings, labels)
        if torch.is_grad_enabled() and embeddings.requires_grad:
            return ag.contrastive_loss(embeddings, labels, self.margin, self.pair_selector.mode)
        p = pr.loss_forward(embeddings, labels, float(self.margin), self.pair_selector.mode)
        return p.loss, p.n
