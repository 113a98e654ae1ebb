"""ResNet speech encoder on the HIP engine: ``models.resnet.SpeakerEmbNet`` for ``arch: resnet``.

The reference selects it by config (conf/audio_config.yaml:93-102: ``input_dim 1, hidden_dim [64,128,256],
residual_block_layers [3,3,3], fc_layers 1, embedding_dim 256, pooling average``; train_audio.py:64-66 imports
``models.resnet`` and feeds it ``[B,1,F,T]`` features, :183-184) but ships NO source for it, while the north star
names the "audio_models ResNet ... mel-feature encoder over [B,1,F,T]".  So the architecture is build-owned
(parity unpinned; pinned only to this repo's own oracle restatement, oracle.audio_resnet_embedding), the thin
speaker ResNet those config keys describe:

    Conv2d(1 -> h0, 3x3, pad 1, no bias) - BN - ReLU
    stage i (h_i channels): residual_block_layers[i] BasicBlocks (conv3x3 - BN - ReLU - conv3x3 - BN, + shortcut
        (1x1 stride-2 conv + BN where the shape changes), ReLU); stages 1.. start with stride 2
    pooling of the last map [B, h_last, F', T']               ("pooling": below)
    Linear(P -> embedding_dim)                                ("fc_layers: 1"), or
    Linear(P -> E) - BN - ReLU - Linear(E -> E)               ("fc_layers: 2": keys fc1 / fc1_bn / fc2; returns (xv, x_a) as tdnn.py:89-101)

Poolings (k = number of stride-2 stages, F' = ((F - 1) >> k) + 1, Wb = the utterance's valid frames of T'):
    average               mean over (F', Wb) -> P = h_last
    statistic             per feature j = f' h_last + c (the channels-last flatten of (F', h_last), D = F' h_last): mean over Wb frames and
                          sqrt(unbiased variance + POOL_EPS) -> P = 2 D; needs Wb >= 2
    attentive_statistic   deeplip_amd.audio.AttentiveStatPooling(D, attention_hidden_size) over the frames' D-vectors, with
                          std = sqrt(max(sum alpha x^2 - mean^2, 0) + POOL_EPS) -> P = 2 D
    multi_head_attention  deeplip_amd.audio.MultiHeadAttention(D, attention_heads, attention_hidden_size): n such poolings of their own
                          hidden width over the same D-vectors, concatenated -> P = n 2 D
The last map is post-ReLU: a good share of its features is exactly constant over time (zero), where a standard deviation without a
floor has a 0/0 gradient.  POOL_EPS under the root is part of the definition, in eval and in training.  D depends on the feature
dimension, so both statistics poolings need ``feat_dim`` in the options.

Engine mapping: exactly the lip-clip trunk's -- every conv is one implicit-GEMM launch with BN / ReLU / residual
fused (deeplip_amd.video.BasicBlock is reused as is), channels-last activations, split activation format
between layers in ``f16x3`` mode.  The 1-channel input is zero-padded to the kernels' channel granule (4, or 32
in split format) once at the boundary.  Train mode runs the same autograd Functions as the lip-clip trunk.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import ops, packing
from . import arith
from .holders import BatchNormParams, ConvParams, LinearParams, Marker
from .video import BasicBlock, _basic_block_train, _cached_pack, downsample_basic_block

Tensor = torch.Tensor
POOL_EPS = 1e-5          # under the root of both statistics poolings' standard deviation
POOLINGS = ("average", "statistic", "attentive_statistic", "multi_head_attention")


def attentive_pool_nhwc(h: Tensor, pool, lens: Optional[Tensor] = None, shift: int = 0) -> Tensor:
    """Eval-mode attentive statistics pooling of the map h [N,H,W,C] fp32 -> [N, heads 2 H C]: ``pool`` (deeplip_amd.audio.AttentiveStatPooling
    or MultiHeadAttention of input size H C) over the D-vectors of each utterance's valid frames (``lens`` int32 CUDA input lengths /
    ``shift`` as ops.time_tail_zero; the frame counts are formed on the device), every standard deviation with POOL_EPS."""
    from .audio import attentive_pool_ntc
    N, H, W, C_ = h.shape
    xt = ops.swap_axes_nhwc(h).view(N, W, H * C_)              # each frame's D-vector contiguous: the hidden layer is one GEMM
    valid = None if lens is None else ops.time_valid_lengths(lens, shift, W)
    return attentive_pool_ntc(pool, xt, valid, 0, POOL_EPS)


def attentive_pool_nhwc_train(h: Tensor, pool) -> Tensor:
    """The same under model.train(), differentiable in h and in the pooling's four parameters (one length per batch)."""
    from . import autograd as ag
    N, H, W, C_ = h.shape
    return ag.attentive_stat_pool(ag.swap_axes_nhwc(h).view(N, W, H * C_), pool, POOL_EPS)


class SpeakerEmbNet(nn.Module):
    def __init__(self, opts):
        super().__init__()
        o = opts[opts["arch"]] if "arch" in opts else opts
        self.pooling_type = o.get("pooling", "average")
        if self.pooling_type not in POOLINGS:
            raise NotImplementedError(f"resnet speech encoder: pooling is one of {POOLINGS} (conf/audio_config.yaml:102)")
        self.fc_layers = o.get("fc_layers", 1)
        if self.fc_layers not in (1, 2):
            raise NotImplementedError("resnet speech encoder: fc_layers must be 1 or 2 (conf/audio_config.yaml:99)")
        self.input_dim = o.get("input_dim", 1)
        if self.input_dim != 1:
            raise ValueError("resnet speech encoder takes [B,1,F,T] features (input_dim 1)")
        hidden, layers = list(o["hidden_dim"]), list(o["residual_block_layers"])
        self.embedding_dim = o["embedding_dim"]
        self.conv1 = ConvParams(1, hidden[0], (3, 3), bias=False)
        self.bn1 = BatchNormParams(hidden[0])
        self.relu = Marker("ReLU")
        blocks, inplanes = [], hidden[0]
        for i, (planes, n) in enumerate(zip(hidden, layers)):
            stride = 1 if i == 0 else 2
            stage = []
            for j in range(n):
                s = stride if j == 0 else 1
                down = downsample_basic_block(inplanes, planes, s) if (s != 1 or inplanes != planes) else None
                stage.append(BasicBlock(inplanes, planes, s, down, relu_type="relu"))
                inplanes = planes
            blocks.append(nn.Sequential(*stage))
        self.layers = nn.Sequential(*blocks)
        self.stages2 = len(hidden) - 1          # k: stride-2 stages in front of the last map
        if self.pooling_type == "average":
            self.avgpool = Marker("AdaptiveAvgPool2d(1)")
            self.feat_dim, pooled = None, inplanes
        else:
            if o.get("feat_dim") is None:
                raise ValueError(f"resnet speech encoder: pooling {self.pooling_type!r} needs the key 'feat_dim' (the pooled vector has "
                                 "((feat_dim - 1) >> stride-2 stages) + 1 features per channel)")
            if inplanes % 4:
                raise ValueError("resnet speech encoder: statistics poolings need a last width that is a multiple of 4")
            self.feat_dim = int(o["feat_dim"])
            if self.feat_dim < 1:
                raise ValueError("resnet speech encoder: feat_dim must be >= 1")
            self.pool_dim = (((self.feat_dim - 1) >> self.stages2) + 1) * inplanes       # D
            pooled = 2 * self.pool_dim
            if self.pooling_type == "attentive_statistic":
                from .audio import AttentiveStatPooling
                self.pooling = AttentiveStatPooling(self.pool_dim, int(o.get("attention_hidden_size", 64)))
            elif self.pooling_type == "multi_head_attention":
                from .audio import MultiHeadAttention
                ahs = o.get("attention_hidden_size", 64)
                self.pooling = MultiHeadAttention(self.pool_dim, o.get("attention_heads", 4), ahs if isinstance(ahs, int) else list(ahs))
                pooled = self.pooling.output_size
        if self.fc_layers == 1:
            self.fc = LinearParams(pooled, self.embedding_dim)
        else:                                   # ("bn1" is the stem's)
            self.fc1 = LinearParams(pooled, self.embedding_dim)
            self.fc1_bn = BatchNormParams(self.embedding_dim)
            self.fc2 = LinearParams(self.embedding_dim, self.embedding_dim)
        for m in self.modules():
            if isinstance(m, ConvParams):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))

    def _blocks(self):
        return [b for stage in self.layers for b in stage]

    def _pack(self, device):
        cp = 32 if packing.PRECISION == "f16x3" else 4
        w = torch.zeros(self.conv1.out_channels, cp, 3, 3, dtype=self.conv1.weight.dtype)
        w[:, :1] = self.conv1.weight.detach().cpu()
        pk = {"stem": packing.pack_conv2d(w, None, self.bn1, device, packing.const_slope(self.conv1.out_channels, 0.0, device)),
              "blocks": [b.pack(device) for b in self._blocks()], "cp": cp}
        if self.fc_layers == 1:
            pk["fc"] = packing.pack_linear(self.fc.weight, self.fc.bias, None, device)
        else:
            sc, sh = packing.bn_scale_shift(self.fc1_bn)
            pk["fc1"] = packing.pack_linear(self.fc1.weight, self.fc1.bias, None, device)
            pk["fc1_bn"] = (sc.float().to(device), sh.float().to(device))
            pk["fc2"] = packing.pack_linear(self.fc2.weight, self.fc2.bias, None, device)
        return pk

    def _features_4d(self, x: Tensor) -> Tensor:
        if x.dim() == 3:
            x = x.unsqueeze(1)
        if x.dim() != 4 or x.shape[1] != 1:
            raise ValueError(f"resnet speech encoder expects [B,1,F,T] features, got {tuple(x.shape)}")
        if self.feat_dim is not None and x.shape[2] != self.feat_dim:
            raise ValueError(f"resnet speech encoder: built for feat_dim {self.feat_dim} (pooling {self.pooling_type!r}), got F = {x.shape[2]}")
        return x

    def _input_nhwc(self, x: Tensor, cp: int) -> Tensor:
        x = self._features_4d(x)
        B, _, Fq, T = x.shape
        # [B,1,F,T] -> channels-last [B,F,T,cp] with the one real channel first (a transpose-and-pad launch: [B*F, 1, T] -> [B*F, T, cp])
        return ops.nct_to_ntc(x.contiguous().float().view(B * Fq, 1, T), pad_to=cp).view(B, Fq, T, cp)

    def _embed_train(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        from . import autograd as ag, autograd_video as av
        h = self._input_nhwc(x, 4)
        w = torch.cat([self.conv1.weight, torch.zeros_like(self.conv1.weight).expand(-1, 3, -1, -1)], dim=1)   # pad C 1 -> 4
        h = av.prelu(av.batchnorm(av.conv(h, w, None, pad=(1, 1)), self.bn1), self.relu)
        for b in self._blocks():
            h = _basic_block_train(b, h)
        if self.pooling_type == "average":
            pooled = av.avgpool(h)
        elif self.pooling_type == "statistic":
            if h.shape[2] < 2:
                raise ValueError(f"resnet speech encoder: pooling 'statistic' needs utterances of >= {self.min_frames()} frames")
            pooled = ag.statpool_nhwc(h, POOL_EPS)
        else:
            pooled = attentive_pool_nhwc_train(h, self.pooling)
        if self.fc_layers == 1:
            e = ag.linear(pooled, self.fc.weight, self.fc.bias)
            return e, e
        x_a = ag.linear(pooled, self.fc1.weight, self.fc1.bias)
        xv = ag.linear(ag.bn_rows_act_train(x_a, self.fc1_bn, 0.0, act_first=False), self.fc2.weight, self.fc2.bias)
        return xv, x_a

    def frames_consumed(self) -> int:
        """Frames the convolutions take off an utterance: none (every convolution is zero-padded; the TDNN encoders' valid convolutions
        take 22).  The shortest utterance the encoder embeds is min_frames()."""
        return 0

    def min_frames(self) -> int:
        """The shortest utterance the encoder embeds: one frame, or with pooling 'statistic' the (1 << k) + 1 frames that leave two on the
        last map (the unbiased standard deviation)."""
        return (1 << self.stages2) + 1 if self.pooling_type == "statistic" else 1

    def _pool_eval(self, h: Tensor, lens: Optional[Tensor], shift: int) -> Tensor:
        """The last map [N,H,W,C] fp32 -> the pooled vector, each utterance over its own valid frames."""
        if self.pooling_type == "average":
            return ops.avgpool(h) if lens is None else ops.avgpool_time_ragged(h, lens, shift)
        if self.pooling_type == "statistic":
            if h.shape[2] < 2:
                raise ValueError(f"resnet speech encoder: pooling 'statistic' needs utterances of >= {self.min_frames()} frames")
            return ops.statpool_nhwc(h, lens, shift, POOL_EPS)
        return attentive_pool_nhwc(h, self.pooling, lens, shift)

    @arith.guarded_eval
    def extract_embedding(self, x: Tensor, lengths=None) -> Tuple[Tensor, Tensor]:
        """[B,1,F,T] (or [B,F,T]) -> (embedding [B,E], the same tensor) with a single fully connected layer; with ``fc_layers: 2``
        (xv [B,E] = fc2 output, x_a [B,E] = fc1 output), the TDNN encoder's interface (tdnn.py:89-101).  ``lengths`` (eval mode; B values
        in [min_frames(), T], or an int32 device tensor, which is not read on the host): a ragged batch padded to T -- whatever the
        padding holds, row b equals extract_embedding(x[b:b+1, :, :, :lengths[b]]).  Every layer's input is kept zero at frames t >= L_b, where a zero-padded convolution over the batch reads what it reads at the
        end of the utterance run alone; after k stride-2 stages L_b has become ((L_b - 1) >> k) + 1, so the one length vector and a
        shift count serve every layer (ops.time_tail_zero behind each convolution; the pooling kernels take the same pair)."""
        if self.training:
            if lengths is not None:
                raise NotImplementedError("the resnet speech encoder takes a ragged batch (lengths) in eval mode only: a training batch "
                                          "is cropped to one length (datasets.py:112-115)")
            return self._embed_train(x)
        self._features_4d(x)        # (a wrong shape is refused before anything is packed or launched)
        p = _cached_pack(self, x.device, self._pack)
        split = p["stem"].wscale is not None
        blocks = self._blocks()
        # f16x3: a block runs in the split activation format when both its widths are whole 32-channel blocks (every shipped width is);
        # a narrower one takes and leaves fp32.  The pooling kernels read fp32.
        want = [split and b.conv1.weight.shape[1] % 32 == 0 and b.planes % 32 == 0 for b in blocks] + [False]
        h = self._input_nhwc(x, p["cp"])
        lens = ops.lengths_i32(lengths, x.device, n=h.shape[0], lo=self.min_frames(), hi=h.shape[2])
        if lens is not None:
            ops.time_tail_zero(h, lens, 0)     # the caller's padding need not be zero
        if split:
            h = ops.split_pack(h)
        h = ops.conv_nhwc(h, p["stem"].w, p["stem"].b, pad=(1, 1), slope=p["stem"].slope, w_scale=p["stem"].wscale,
                          x_split=split, out_split=want[0])
        if lens is not None:
            ops.time_tail_zero(h, lens, 0)
        shift, cur = 0, want[0]
        for i, (b, bp) in enumerate(zip(blocks, p["blocks"])):
            shift += int(b.stride == 2)
            if want[i] and not cur:
                h = ops.split_pack(h)
            cur = want[i] and want[i + 1]
            h = b.run(h, bp, split=want[i], out_split=cur, time_lengths=None if lens is None else (lens, shift))
        pooled = self._pool_eval(h, lens, shift)
        if self.fc_layers == 1:
            e = ops.linear(pooled, p["fc"].w, p["fc"].b, w_scale=p["fc"].wscale)
            return e, e
        x_a = ops.linear(pooled, p["fc1"].w, p["fc1"].b, w_scale=p["fc1"].wscale)
        xv = ops.linear(ops.affine_act(x_a, p["fc1_bn"][0], p["fc1_bn"][1], 0.0), p["fc2"].w, p["fc2"].b, w_scale=p["fc2"].wscale)
        return xv, x_a

    def forward(self, x: Tensor) -> Tensor:
        return self.extract_embedding(x)[0]
