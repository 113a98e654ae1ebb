"""Fusion heads on the HIP engine: mirror of ``models/fusion_models/model_fusion.py`` (Linearfusion)
and ``models/fusion_models/LBP.py`` (LowFER, and the BNBilinear head its trainer asks for) and of the lost
``models/fusion_models/compact_bilinear_pooling.py`` (CompactBilinearPooling), plus the test-time fusion the reference actually
uses for scoring: per-modality z-norm + concat (train_fusion.py:233-238,353-358)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import ops, packing
from .holders import BatchNormParams, LinearParams, Marker
from .video import _cached_pack


class Linearfusion(nn.Module):
    """model_fusion.py:10-24: fc1 - bn1 - LeakyReLU(0.2) - fc2; returns x1 if extract_feats."""

    def __init__(self, input_size, hidden_size, num_classes, extract_feats):
        super().__init__()
        self.extract_feats = extract_feats
        self.hidden_size = hidden_size
        self.fc1 = LinearParams(input_size, hidden_size)
        self.bn1 = BatchNormParams(hidden_size)
        self.fc2 = LinearParams(hidden_size, hidden_size)
        self.activation = Marker("LeakyReLU(0.2)")

    def _pack(self, device):
        return {"fc1": packing.pack_linear(self.fc1.weight, self.fc1.bias, self.bn1, device,
                                           packing.const_slope(self.hidden_size, 0.2, device)),
                "fc2": packing.pack_linear(self.fc2.weight, self.fc2.bias, None, device)}

    def forward(self, x):
        if self.training:
            # train mode (config C5): batch-statistics BN through the autograd-wrapped HIP kernels
            from . import autograd as ag
            x1 = ag.bn_act_train(ag.linear(x, self.fc1.weight, self.fc1.bias), self.bn1, 0.2)
            return x1 if self.extract_feats else ag.linear(x1, self.fc2.weight, self.fc2.bias)
        p = _cached_pack(self, x.device, self._pack)
        x1 = ops.linear(x.contiguous(), p["fc1"].w, p["fc1"].b, slope=p["fc1"].slope, w_scale=p["fc1"].wscale)  # fc1+bn1+lrelu fused
        if self.extract_feats:
            return x1
        return ops.linear(x1, p["fc2"].w, p["fc2"].b, w_scale=p["fc2"].wscale)


def model_fusion(input_size, hidden_size, num_classes, extract_feats):
    """model_fusion.py:26-27."""
    return Linearfusion(input_size, hidden_size, num_classes, extract_feats)


class LowFER(nn.Module):
    """LBP.py:8-54.  Parameters U, V, bn0, bn1 are kept for state-dict compatibility (created on the
    CPU: the reference hard-codes device='cuda', LBP.py:12-15).  forward returns what the shipped
    code returns -- cat[e1, sigmoid(e2), sigmoid(e2)*e1] -- because the MFB product (LBP.py:38-42) is
    overwritten before use (LBP.py:48-50)."""

    def __init__(self, d1, d2, o):
        super().__init__()
        k = 30
        self.U = nn.Parameter(torch.tensor(np.random.uniform(-1, 1, (d1, k * o)), dtype=torch.float))
        self.V = nn.Parameter(torch.tensor(np.random.uniform(-1, 1, (d2, k * o)), dtype=torch.float))
        self.input_dropout = Marker("Dropout(0.3)")
        self.hidden_dropout1 = Marker("Dropout(0.4)")
        self.hidden_dropout2 = Marker("Dropout(0.5)")
        self.bn0 = BatchNormParams(d1)
        self.bn1 = BatchNormParams(d1)
        self.k, self.o = k, o

    def forward(self, e1, e2):
        return ops.lowfer_cat(e1.contiguous(), e2.contiguous())


class BNBilinear(nn.Module):
    """``LBP.BNBilinear(d1, d2, o)``: the head the reference's train_fusion.py:84 builds and its LBP.py does not define.  Build-owned
    (there is nothing upstream to pin it to); it follows the live and commented lines of LBP.py:38-44 in their order, without the
    signed square root of :42 (its derivative is unbounded at 0):

        P = e1 @ U, Q = e2 @ V                      U [d1, k o], V [d2, k o]: LowFER's names, shapes and uniform(-1, 1) start
        z = (P * Q).view(-1, o, k).mean(-1)         low-rank bilinear pooling
        out = bn1(F.normalize(z, p=2, dim=-1))      BatchNorm1d(o): batch statistics in train mode, folded in eval mode

    The product runs on csrc/bilinear_ops.hip (exact fp32 MFMA under every arithmetic mode, hence the f32 pack precision below);
    train mode composes autograd.bilinear_pool with the engine's L2-normalise and BatchNorm Functions."""

    def __init__(self, d1, d2, o, k=30):
        super().__init__()
        d1, d2, o, k = int(d1), int(d2), int(o), int(k)
        if d1 < 4 or d2 < 4 or d1 % 4 or d2 % 4:
            raise ValueError(f"BNBilinear: embedding widths ({d1}, {d2}) must be positive multiples of 4")
        if o < 1 or k < 1:
            raise ValueError(f"BNBilinear: o = {o} and k = {k} must be positive")
        self.U = nn.Parameter(torch.tensor(np.random.uniform(-1, 1, (d1, k * o)), dtype=torch.float))
        self.V = nn.Parameter(torch.tensor(np.random.uniform(-1, 1, (d2, k * o)), dtype=torch.float))
        self.bn1 = BatchNormParams(o)
        self.d1, self.d2, self.k, self.o = d1, d2, k, o
        self.__dict__["_dlip_precision"] = "f32"      # packing.state_version: its pack is the same under every mode

    def _pack(self, device):
        scale, shift = packing.bn_scale_shift(self.bn1)
        return {"scale": packing._dev(scale, device), "shift": packing._dev(shift, device)}

    def forward(self, e1, e2):
        e1, e2 = e1.contiguous(), e2.contiguous()
        U, V = self.U.contiguous(), self.V.contiguous()
        ops.bilinear_check(e1, e2, U.detach(), V.detach(), self.k)
        if self.training:
            if e1.shape[0] < 2:
                raise ValueError("BNBilinear: train mode needs at least two rows (BatchNorm1d's batch statistics)")
            from . import autograd as ag
            return ag.bn_act_train(ag.l2_normalize(ag.bilinear_pool(e1, e2, U, V, self.k), 1e-12), self.bn1, 1.0)
        p = _cached_pack(self, e1.device, self._pack)
        return ops.bilinear_finish(ops.bilinear_pool(e1, e2, U.detach(), V.detach(), self.k), p["scale"], p["shift"], 1e-12)


class CompactBilinearPooling(nn.Module):
    """``CompactBilinearPooling(in_channels1, in_channels2, out_channels, sum_pool=True)``: the head the reference's
    train_fusion.py:31-32,83 imports and builds; upstream ships no source for it any more.  Constructor, attribute names and
    state-dict keys are upstream's:

        tensor_sketch1 [C1, D], tensor_sketch2 [C2, D]      count sketches, requires_grad=False: row i is s[i] = +-1 at column h[i]
        psi1 = x1.permute(0,2,3,1) @ tensor_sketch1, psi2 likewise
        cbp  = irfft(rfft(psi1) * rfft(psi2), n=D) * D      = D * (psi1 circularly convolved with psi2)
        return cbp.sum(dim=[1,2]) if sum_pool else cbp      [B,D] or [B,H,W,D]

    The hashes come from torch's global generator in the order h1, s1, h2, s2 (h: randint(D, (C,)), s: 2 randint(2, (C,)) - 1), so
    torch.manual_seed reproduces a head and a checkpoint carries its hashes.  The kernels (csrc/compact_bilinear_ops.hip) never
    touch the dense matrices: the pack is h, s and their bin-sorted lists, re-read from the parameters whenever these change
    (load_state_dict); a sketch that is not one +-1 per row is refused there.  [B,C] inputs are taken as one position (build-owned:
    upstream's permute needs 4-D)."""

    def __init__(self, in_channels1, in_channels2, out_channels, sum_pool=True):
        super().__init__()
        c1, c2, d = int(in_channels1), int(in_channels2), int(out_channels)
        if c1 < 1 or c2 < 1 or not 1 <= d <= ops.CBP_MAX_D:
            raise ValueError(f"CompactBilinearPooling: channels ({c1}, {c2}) must be positive and out_channels = {d} in 1 .. {ops.CBP_MAX_D}")
        self.in_channels1, self.in_channels2, self.out_channels, self.sum_pool = c1, c2, d, bool(sum_pool)
        h1, s1 = self._draw(c1, d)
        h2, s2 = self._draw(c2, d)
        self.tensor_sketch1 = nn.Parameter(self.generate_tensor_sketch(h1, s1, d), requires_grad=False)
        self.tensor_sketch2 = nn.Parameter(self.generate_tensor_sketch(h2, s2, d), requires_grad=False)
        self.__dict__["_dlip_precision"] = "f32"      # packing.state_version: its pack is the same under every mode

    @staticmethod
    def _draw(c, d):
        h = torch.randint(d, (c,))
        s = 2 * torch.randint(2, (c,), dtype=torch.float32) - 1
        return h, s

    @staticmethod
    def generate_tensor_sketch(rand_h, rand_s, out_channels):
        sketch = torch.zeros(rand_h.numel(), int(out_channels), dtype=torch.float32)
        sketch[torch.arange(rand_h.numel()), rand_h.long()] = rand_s.float()
        return sketch

    def _pack(self, device):
        return {"s1": ops.compact_bilinear_pack(packing._dev(self.tensor_sketch1, device), "tensor_sketch1"),
                "s2": ops.compact_bilinear_pack(packing._dev(self.tensor_sketch2, device), "tensor_sketch2")}

    def forward(self, x1, x2):
        for t, name in ((x1, "x1"), (x2, "x2")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ops._lib.DeepLipHipError(f"{name}: expected a CUDA (ROCm) tensor; deeplip_amd has no CPU path")
        p = _cached_pack(self, x1.device, self._pack)
        ops.compact_bilinear_check(x1, x2, p["s1"], p["s2"])
        from . import autograd as ag
        return ag.compact_bilinear(x1, x2, p["s1"], p["s2"], self.sum_pool)


class BNCompactBilinear(nn.Module):
    """The trainer's compact bilinear head (``model.fusion: compact_bilinear``): bn1(F.normalize(cbp(e1, e2))), the tail of
    BNBilinear behind CompactBilinearPooling(d1, d2, o).  The raw layer's outputs scale with D |e1| |e2|; the row norm and the
    BatchNorm1d(o) are what make them usable in front of CrossEntropy / LMCL.  The signed square root that usually precedes the
    norm is not built, for BNBilinear's reason (its derivative is unbounded at 0).  Build-owned; trains only bn1 (the sketches are
    constants)."""

    def __init__(self, d1, d2, o):
        super().__init__()
        self.cbp = CompactBilinearPooling(d1, d2, o)
        self.bn1 = BatchNormParams(int(o))
        self.d1, self.d2, self.o = int(d1), int(d2), int(o)
        self.__dict__["_dlip_precision"] = "f32"

    def _pack(self, device):
        scale, shift = packing.bn_scale_shift(self.bn1)
        return {"scale": packing._dev(scale, device), "shift": packing._dev(shift, device)}

    def forward(self, e1, e2):
        if self.training:
            if isinstance(e1, torch.Tensor) and e1.is_cuda and e1.shape[0] < 2:
                raise ValueError("BNCompactBilinear: train mode needs at least two rows (BatchNorm1d's batch statistics)")
            from . import autograd as ag
            return ag.bn_act_train(ag.l2_normalize(self.cbp(e1, e2), 1e-12), self.bn1, 1.0)
        z = self.cbp(e1, e2)
        p = _cached_pack(self, e1.device, self._pack)
        return ops.bilinear_finish(z, p["scale"], p["shift"], 1e-12)


def feature_normalize(data: torch.Tensor) -> torch.Tensor:
    """Trainer.feature_normalize (train_fusion.py:233-238): per-row z-norm, unbiased std."""
    return ops.znorm_cat(data.contiguous(), None)


def fuse_av(xv_audio: torch.Tensor, em_video) -> torch.Tensor:
    """train_fusion.py:353-358: cat([znorm(audio), znorm(video)], 1) in one launch -> [U, Da+Dv].  ``em_video`` may be
    the per-clip means [U,512] or what ``Lipreading.embed(x, finish=False)`` returns while they are still pooled partial
    sums (ops.Pooled): the temporal mean of train_fusion.py:348 is then finished inside the same launch."""
    if isinstance(em_video, ops.Pooled):
        return ops.znorm_cat_pooled(xv_audio.contiguous(), em_video)
    return ops.znorm_cat(xv_audio.contiguous(), em_video.contiguous())


_side_streams: dict = {}


def embed_av(model_audio, model_video, feats_audio: torch.Tensor, clips: torch.Tensor, two_streams: bool = True) -> torch.Tensor:
    """One batch of the test-time pipeline (train_fusion.py:338-358): x-vectors, per-clip lip embeddings, z-norm + concat
    -> [B, 1024].  ``two_streams``: the speech encoder is issued on a second HIP stream (fork / join by events), so the
    two encoders' launches -- each of which fills the chip's LDS on its own -- overlap at their heads and tails;
    recorded into a step plan the fork / join becomes two branches of the graph (measured +4.5-5 % on the B = 64 step)."""
    from ._lib import range_scope
    with range_scope():      # one scope over both encoders: its verdict goes out on `cur` behind the join
        return _embed_av(model_audio, model_video, feats_audio, clips, two_streams)


def _embed_av(model_audio, model_video, feats_audio, clips, two_streams):
    if not two_streams:
        return fuse_av(model_audio.extract_embedding(feats_audio)[0], model_video.embed(clips, finish=False))
    cur = torch.cuda.current_stream(clips.device)
    side = _side_streams.get((clips.device, cur.cuda_stream))
    if side is None:
        side = _side_streams[(clips.device, cur.cuda_stream)] = torch.cuda.Stream(device=clips.device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        xv_audio = model_audio.extract_embedding(feats_audio)[0]
    em_video = model_video.embed(clips, finish=False)
    cur.wait_stream(side)
    return fuse_av(xv_audio, em_video)
