"""Speech encoder (TDNN / E-TDNN x-vector) on the HIP engine.  Host-side mirror of the
reference's ``models/audio_models/{tdnn,pooling}.py``: same class names, ``opts`` schema,
state-dict keys and return tuples.

Engine layout is time-major channels-last [B,T,C]: each TDNN_Block (dilated Conv1d + BN +
LeakyReLU, tdnn.py:35-43) is one implicit-GEMM launch (k=1 layers are plain GEMMs over B*T rows),
statistics pooling is a two-pass fp64 reduction, fc1/fc2 reuse the GEMM kernel.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, arith, ops, packing
from .holders import BatchNormParams, ConvParams, LinearParams, Marker
from .video import _cached_pack, _require_eval

Tensor = torch.Tensor
LRELU = 0.2

# f16x3 extraction path: statistics pooling comes out of the last TDNN layer's epilogue as pooled partial sums
# (dlip_conv_pool_f16x3 + dlip_pool_finish_f32) instead of a [B,T',1500] tensor written and read back once
# (pooling.py:24-26).  The unfused twin stays for the tests, for taps and for utterances shorter than a tile.
FUSE_POOL = True


class MeanStdPooling(nn.Module):
    """pooling.py:7-26: [B,C,T] -> [B,2C] = cat(mean, unbiased std) over T."""

    def forward(self, x: Tensor) -> Tensor:
        return ops.meanstd_pool(ops.nct_to_ntc(x.contiguous()))

    def run_ntc(self, x_ntc: Tensor) -> Tensor:
        return ops.meanstd_pool(x_ntc)


def attentive_pool_ntc(pool, x_ntc: Tensor, lengths: Optional[Tensor], len_add: int, eps: float) -> Tensor:
    """The eval-mode route of both attentive poolings: x [B,T,C] -> [B, heads 2C].  hidden = W x + b is ONE GEMM launch for all heads;
    scores, softmax and the weighted statistics read hidden and x once (dlip_mh_attn_scores_f32 / dlip_mh_attn_stat_pool_f32)."""
    B, T, C_ = x_ntc.shape
    ops.mh_attn_check(pool.head, T, C_)
    hidden = ops.linear(x_ntc.reshape(B * T, C_), pool.W.detach().contiguous(), pool.b.detach().reshape(-1).contiguous())
    alpha = ops.mh_attn_scores(hidden.view(B, T, pool.hidden_size), pool.v.detach().reshape(-1).contiguous(),
                               pool.k.detach().reshape(-1).contiguous(), pool.head_off, lengths, len_add)
    return ops.mh_attn_stat_pool(x_ntc, alpha, eps, lengths, len_add)


class AttentiveStatPooling(nn.Module):
    """pooling.py:73-107: attention over frames, then attention-weighted mean and std -- one head of the kernels MultiHeadAttention runs
    (DESIGN.md 4h).  ``eps`` = 0 is the reference's std = sqrt(sum alpha x^2 - mean^2); the ResNet speech encoder's head passes POOL_EPS
    (std = sqrt(max(sum alpha x^2 - mean^2, 0) + eps), deeplip_amd/audio_resnet.py)."""
    head, head_off = 1, None        # (one head owns every hidden column: the kernels take no offsets array)

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.hidden_size, self.input_size = hidden_size, input_size
        self.W = nn.Parameter(torch.Tensor(hidden_size, input_size))
        self.b = nn.Parameter(torch.Tensor(1, hidden_size))
        self.v = nn.Parameter(torch.Tensor(hidden_size, 1))
        self.k = nn.Parameter(torch.Tensor(1, 1))
        for p in self.parameters():
            nn.init.xavier_normal_(p)

    def run_ntc(self, x_ntc: Tensor, lengths: Optional[Tensor] = None, len_add: int = 0, eps: float = 0.0) -> Tensor:
        """x [B,T,C] -> [B,2C]; ``lengths`` (int32 CUDA [B]): attention and statistics over the first lengths[b] + len_add frames."""
        return attentive_pool_ntc(self, x_ntc, lengths, len_add, eps)

    def forward(self, x):
        """[B,C,T] (reference layout) -> [B,2C]."""
        return self.run_ntc(ops.nct_to_ntc(x.contiguous()))


class MultiHeadAttention(nn.Module):
    """``pooling: multi_head_attention`` (pooling.py:62-71 is an empty TODO class upstream; this is the definition):
    ``head`` attentive statistics poolings of their own hidden width over the same frames, concatenated -- [B,C,T] -> [B, head 2C] =
    cat_h [mean_h | std_h], std = sqrt(max(sum alpha x^2 - mean^2, 0) + POOL_EPS).  ``hidden_size``: an int (every head that width) or a
    sequence of ``head`` widths.  The heads' parameters are stacked: W [S,C], b [1,S], v [S,1], k [1,head] with S the sum of the widths;
    head h owns rows off_h : off_{h+1} of the first three and column h of k.  hidden = W x + b is ONE GEMM launch for all heads; scores,
    softmax and the weighted statistics read hidden and x once (dlip_mh_attn_scores_f32 / dlip_mh_attn_stat_pool_f32)."""

    def __init__(self, input_size, head=4, hidden_size=(100, 200, 300, 400)):
        super().__init__()
        if isinstance(head, bool) or not isinstance(head, int) or not 1 <= head <= ops.MH_MAX_HEADS:
            raise ValueError(f"MultiHeadAttention: head is an int in [1, {ops.MH_MAX_HEADS}], got {head!r}")
        if isinstance(hidden_size, int) and not isinstance(hidden_size, bool):
            widths = [hidden_size] * head
        elif isinstance(hidden_size, (list, tuple)) and all(isinstance(w, int) and not isinstance(w, bool) for w in hidden_size):
            widths = list(hidden_size)
        else:
            raise ValueError(f"MultiHeadAttention: hidden_size is an int or a sequence of {head} ints, got {hidden_size!r}")
        if len(widths) != head:
            raise ValueError(f"MultiHeadAttention: {len(widths)} hidden sizes for {head} heads")
        if any(w < 1 for w in widths):
            raise ValueError(f"MultiHeadAttention: every hidden size must be positive, got {widths}")
        self.input_size, self.head, self.hidden_sizes = int(input_size), head, tuple(widths)
        offs = [0]
        for w in widths:
            offs.append(offs[-1] + w)
        self.offsets = tuple(offs)
        self.hidden_size = S = offs[-1]
        self.W = nn.Parameter(torch.empty(S, self.input_size))
        self.b = nn.Parameter(torch.empty(1, S))
        self.v = nn.Parameter(torch.empty(S, 1))
        self.k = nn.Parameter(torch.empty(1, head))
        # (the kernels read the head boundaries on the device; not a part of the state dict)
        self.register_buffer("head_off", torch.tensor(offs, dtype=torch.int32), persistent=False)
        with torch.no_grad():       # every head's slice on its own block: a head's init does not depend on its neighbours
            for h in range(head):
                lo, hi = offs[h], offs[h + 1]
                nn.init.xavier_normal_(self.W[lo:hi])
                nn.init.xavier_normal_(self.b[:, lo:hi])
                nn.init.xavier_normal_(self.v[lo:hi])
                nn.init.xavier_normal_(self.k[:, h:h + 1])

    @property
    def output_size(self) -> int:
        return self.head * 2 * self.input_size

    def run_ntc(self, x_ntc: Tensor, lengths: Optional[Tensor] = None, len_add: int = 0) -> Tensor:
        """x [B,T,C] -> [B, head 2C]; ``lengths`` (int32 CUDA [B]): attention and statistics over the first lengths[b] + len_add frames."""
        from .audio_resnet import POOL_EPS
        return attentive_pool_ntc(self, x_ntc, lengths, len_add, POOL_EPS)

    def forward(self, x):
        """[B,C,T] (reference layout) -> [B, head 2C]."""
        return self.run_ntc(ops.nct_to_ntc(x.contiguous()))


class TDNN_Block(nn.Module):
    """tdnn.py:7-43.  ``dilation`` is the context list, e.g. [-2,0,2] -> kernel 3, dilation 2."""

    def __init__(self, input_dim, output_dim, dilation, padding=0, stride=1, bn_first=True):
        super().__init__()
        kernel_size = len(dilation)
        if len(dilation) > 1:
            dilation = (dilation[-1] - dilation[0]) // (len(dilation) - 1)
        else:
            dilation = 1
        if stride != 1:
            raise NotImplementedError("TDNN_Block stride != 1 is never used (tdnn.py:62)")
        self.kernel_size, self.dilation, self.padding = kernel_size, dilation, padding
        self.input_dim, self.output_dim = input_dim, output_dim
        self.context_layer = ConvParams(input_dim, output_dim, (kernel_size,), bias=True)
        self.bn = BatchNormParams(output_dim)
        self.activation = Marker("LeakyReLU(0.2)")
        self.bn_first = bn_first

    def pack(self, device, e_in: int = 0, e_out: int = 0) -> packing.Packed:
        """``e_in`` / ``e_out``: activation exponents of the layer's input / output in the f16x3 pack (packing.act_exponents)."""
        cp = packing.pad_channels(self.input_dim)
        slope = packing.const_slope(self.output_dim, LRELU, device)
        if self.bn_first:   # conv -> BN -> LReLU: BN folds into the conv
            return packing.pack_conv1d(self.context_layer.weight, self.context_layer.bias, self.bn, device, slope, cp, e_in, e_out)
        p = packing.pack_conv1d(self.context_layer.weight, self.context_layer.bias, None, device, slope, cp, e_in, e_out)
        sc, sh = packing.bn_scale_shift(self.bn)  # conv -> LReLU -> BN: BN is the post-affine of the epilogue
        if packing.PRECISION == "f16x3" and e_out:
            sh = sh * (2.0 ** int(e_out))          # (the shift lands behind the activation: scaled with the output)
        p.post_scale, p.post_shift = sc.float().to(device), sh.float().to(device)
        return p

    def run_ntc(self, x: Tensor, p: packing.Packed, x_split: bool = False, out_split: bool = False) -> Tensor:
        """x [B,T,C] -> [B,T',K]; x_split / out_split: split activation format (f16x3 packing only)."""
        return ops.conv1d_ntc(x, p.w, p.b, dilation=self.dilation, pad=self.padding, slope=p.slope,
                              post_scale=p.post_scale, post_shift=p.post_shift, w_scale=p.wscale,
                              x_split=x_split, out_split=out_split)

    def run_pooled(self, x: Tensor, p: packing.Packed, lengths: Optional[Tensor] = None, len_add: int = 0):
        """x [B,T,C] split format -> ops.Pooled column sums of the layer's output over each utterance's T' frames (the
        input of statistics pooling), or None when T' is shorter than the workgroup tile the launch would use.  ``lengths``
        (int32 CUDA [B]): ragged batch -- only the first lengths[b] + len_add output frames of utterance b are pooled."""
        B, T, Cx = x.shape
        Tp = ops.conv_out_size(T, self.kernel_size, 1, self.padding, self.dilation)
        xv = x.view(B, 1, T, Cx)
        wv = p.w.view(p.w.shape[0], 1, p.w.shape[1], p.w.shape[2])
        kw = dict(pad=(0, self.padding), dil=(1, self.dilation))
        if Tp < ops.conv_pool_tile_rows(xv, wv, **kw):
            return None
        return ops.conv_pool(xv, wv, p.b, p.wscale, Tp, slope=p.slope, post_scale=p.post_scale, post_shift=p.post_shift,
                             lengths=lengths, len_add=len_add, **kw)

    def forward(self, x: Tensor) -> Tensor:
        """[B,C,T] -> [B,K,T'] (reference layout, standalone use)."""
        _require_eval(self)
        p = _cached_pack(self, x.device, self.pack)
        h = ops.nct_to_ntc(x.contiguous(), pad_to=packing.pad_channels(self.input_dim))
        return ops.ntc_to_nct(self.run_ntc(h, p))


class PackedFTDNN:
    """The eval pack of an FTDNN_Block: its two convolutions and the bypass scale the stored tensors need (2^(e_out - e_in) s)."""

    def __init__(self, factor: packing.Packed, ctx: packing.Packed, bypass: float):
        self.factor, self.ctx, self.bypass = factor, ctx, bypass

    @property
    def wscale(self):
        return self.ctx.wscale


class FTDNN_Block(nn.Module):
    """One factorized TDNN layer (``arch: ftdnn``, conf/audio_config.yaml:84-92; the definition is the build's own: DESIGN.md 4k).
    ``factor``: Conv1d(input_dim -> bottleneck_dim, one tap per context offset, dilation as TDNN_Block derives it, no bias), no
    BatchNorm, no activation -- its weight [Bn, Cin, k] seen as M [Bn, Cin k] is what the semi-orthogonal step constrains;
    ``context_layer``: Conv1d(bottleneck_dim -> output_dim, 1 tap, bias); ``bn`` and LeakyReLU(0.2) in the order ``bn_first`` says, as
    TDNN_Block; then, when the widths agree and ``bypass_scale`` != 0, y[b, :, t] += bypass_scale x[b, :, t - context[0]]: the input frame
    at context offset 0, added behind the activation and the BatchNorm."""

    def __init__(self, input_dim, output_dim, dilation, bottleneck_dim=128, bypass_scale=0.66, bn_first=True):
        super().__init__()
        context = [int(c) for c in dilation]
        kernel_size = len(context)
        dil = (context[-1] - context[0]) // (kernel_size - 1) if kernel_size > 1 else 1
        Bn = int(bottleneck_dim)
        if Bn < 4 or Bn % 4:
            raise ValueError(f"FTDNN_Block: bottleneck_dim must be a positive multiple of 4 (the convolutions' channel granule), got {Bn}")
        if Bn > input_dim * kernel_size:
            raise ValueError(f"FTDNN_Block: bottleneck_dim {Bn} exceeds input_dim * taps = {input_dim * kernel_size}: the factor matrix "
                             "[Bn, Cin k] cannot have orthonormal rows")
        if Bn > ops.SEMI_ORTH_MAX_ROWS:
            raise ValueError(f"FTDNN_Block: bottleneck_dim {Bn} exceeds {ops.SEMI_ORTH_MAX_ROWS}, what the semi-orthogonal step's LDS plan "
                             "carries (P = M M^T stays in one workgroup's LDS)")
        self.bypass_scale = float(bypass_scale) if input_dim == output_dim else 0.0
        if self.bypass_scale != 0.0:
            if not context[0] <= 0 <= context[-1]:
                raise ValueError(f"FTDNN_Block: the bypass adds the input frame at context offset 0, which {context} does not span")
            if input_dim % 4:
                raise ValueError(f"FTDNN_Block: the bypass moves four channels per lane; width {input_dim} is no multiple of 4")
        self.bypass_shift = -context[0]
        self.kernel_size, self.dilation, self.padding = kernel_size, dil, 0
        self.input_dim, self.output_dim, self.bottleneck_dim = input_dim, output_dim, Bn
        self.factor = ConvParams(input_dim, Bn, (kernel_size,), bias=False)
        self.context_layer = ConvParams(Bn, output_dim, (1,), bias=True)
        self.bn = BatchNormParams(output_dim)
        self.activation = Marker("LeakyReLU(0.2)")
        self.bn_first = bn_first

    def pack(self, device, e_in: int = 0, e_out: int = 0) -> PackedFTDNN:
        """The bottleneck tensor carries exponent 0 (an out-of-range one is arith auto's exact re-run); ``e_in`` / ``e_out`` as TDNN_Block."""
        pf = packing.pack_conv1d(self.factor.weight, None, None, device, packing.const_slope(self.bottleneck_dim, 1.0, device),
                                 packing.pad_channels(self.input_dim), e_in, 0)
        slope = packing.const_slope(self.output_dim, LRELU, device)
        cp = packing.pad_channels(self.bottleneck_dim)
        if self.bn_first:
            pc = packing.pack_conv1d(self.context_layer.weight, self.context_layer.bias, self.bn, device, slope, cp, 0, e_out)
        else:
            pc = packing.pack_conv1d(self.context_layer.weight, self.context_layer.bias, None, device, slope, cp, 0, e_out)
            sc, sh = packing.bn_scale_shift(self.bn)
            if packing.PRECISION == "f16x3" and e_out:
                sh = sh * (2.0 ** int(e_out))
            pc.post_scale, pc.post_shift = sc.float().to(device), sh.float().to(device)
        f16x3 = packing.PRECISION == "f16x3"
        return PackedFTDNN(pf, pc, self.bypass_scale * (2.0 ** int(e_out - e_in) if f16x3 else 1.0))

    def run_ntc(self, x: Tensor, p: PackedFTDNN, x_split: bool = False, out_split: bool = False) -> Tensor:
        """x [B,T,C] -> [B,T',K]; x_split / out_split as TDNN_Block.  The bottleneck travels split when it is whole 32-channel blocks."""
        f, c = p.factor, p.ctx
        z_split = f.wscale is not None and self.bottleneck_dim % 32 == 0
        z = ops.conv1d_ntc(x, f.w, f.b, dilation=self.dilation, pad=0, slope=f.slope, w_scale=f.wscale, x_split=x_split, out_split=z_split)
        byp = self.bypass_scale != 0.0
        y = ops.conv1d_ntc(z, c.w, c.b, dilation=1, pad=0, slope=c.slope, post_scale=c.post_scale, post_shift=c.post_shift,
                           w_scale=c.wscale, x_split=z_split, out_split=out_split and not byp)
        if byp:
            y = ops.ftdnn_bypass(y, x, p.bypass, self.bypass_shift, x_split=x_split, out_split=out_split)
        return y

    def forward(self, x: Tensor) -> Tensor:
        """[B,C,T] -> [B,K,T'] (reference layout, standalone use)."""
        _require_eval(self)
        p = _cached_pack(self, x.device, self.pack)
        h = ops.nct_to_ntc(x.contiguous(), pad_to=packing.pad_channels(self.input_dim))
        return ops.ntc_to_nct(self.run_ntc(h, p))


def default_factorized_layers(context) -> List[int]:
    """Every layer i >= 1 whose context has more than one offset (layers 1 and 2 of the reference's five-layer ``ftdnn`` section)."""
    return [i for i, c in enumerate(context) if i >= 1 and len(c) > 1]


class SemiOrthStep(nn.Module):
    """The semi-orthogonal constraint on every ``factor`` matrix of a model, applied behind the optimizer step: one
    launch pair for all of them.  ``counter`` (a buffer: it goes into checkpoints and into a recorded step's snapshot) counts the
    optimizer steps ON THE DEVICE; the launch advances it and applies the step when the count is a multiple of ``every``, so a replayed
    graph and an eager loop update on the same iterations.  Every rank of a job applies the same deterministic update to identical
    parameters: no collective."""

    def __init__(self, model, every: int = 4):
        super().__init__()
        if isinstance(every, bool) or not isinstance(every, int) or every < 0:
            raise ValueError(f"train.semi_orth_every is an int >= 0 (0: off), got {every!r}")
        self.every = every
        self._mats = [m.factor.weight for m in model.modules() if isinstance(m, FTDNN_Block)]
        if not self._mats:
            raise ValueError("SemiOrthStep: the model has no factorized layer")
        if len(self._mats) > ops.SEMI_ORTH_MAX_MATS:
            raise ValueError(f"SemiOrthStep: at most {ops.SEMI_ORTH_MAX_MATS} factorized layers, got {len(self._mats)}")
        dev = self._mats[0].device
        if dev.type != "cuda":
            raise _lib.DeepLipHipError("SemiOrthStep: the factor matrices must be on the GPU; deeplip_amd has no CPU path")
        self.register_buffer("counter", torch.zeros(2, dtype=torch.int32, device=dev))
        self._ws = ops.semi_orth_workspace(len(self._mats), dev)
        self._key = self._table = None

    def matrices(self):
        return list(self._mats)

    def forward(self):
        key = tuple(m.data_ptr() for m in self._mats)
        if key != self._key:            # (first call, or the parameters moved: a host-to-device copy, never inside a capture)
            self._table, self._key = ops.semi_orth_table([m.detach() for m in self._mats]), key
        tab, max_rows, max_cols = self._table
        ops.semi_orth_step(tab, len(self._mats), max_rows, max_cols, self.counter, self.every, self._ws)


class SpeakerEmbNet(nn.Module):
    """tdnn.py:45-111.  ``opts`` = model options with sub-dict ``opts[opts['arch']]``.  ``arch: ftdnn`` (conf/audio_config.yaml:84-92;
    DESIGN.md 4k) takes the ``tdnn`` keys and three of the build's own: ``bottleneck_dim`` (128), ``bypass_scale`` (0.66) and
    ``factorized_layers`` (default_factorized_layers); the layers it lists are FTDNN_Blocks.  ``arch: sincnet`` is the
    TDNN plus ``.sinc``, a SincConv of ``input_dim`` filters built from the build-owned ``sinc:`` sub-dict: the encoder then takes
    WAVEFORMS [B, S] (``lengths``: sample counts) and the layer trains with the stack."""

    def __init__(self, opts):
        super().__init__()
        arch = opts["arch"]
        opts = opts[arch]
        self.sinc = None
        if arch == "sincnet":
            from .sincnet import SincConv, parse_sinc_section
            self.sinc = SincConv(int(opts["input_dim"]), **parse_sinc_section(opts.get("sinc")))
        context = opts["context"]
        input_dim = opts["input_dim"]
        hidden_dim = opts["hidden_dim"]
        layers_num = opts["tdnn_layers"]
        embedding_dim = opts["embedding_dim"]
        attention_hidden_size = opts.get("attention_hidden_size", 64)     # (upstream's ftdnn section leaves it out)
        self.bn_first = opts["bn_first"]
        self.input_dim = input_dim
        self.embedding_dim = embedding_dim
        self.activation = Marker("LeakyReLU(0.2)")
        factorized = ()
        if arch == "ftdnn":
            factorized = opts.get("factorized_layers")
            factorized = default_factorized_layers(context[:layers_num]) if factorized is None else [int(i) for i in factorized]
            bad = [i for i in factorized if not 1 <= i < layers_num]
            if bad or len(set(factorized)) != len(factorized):
                raise ValueError(f"model.ftdnn.factorized_layers: distinct layer indices in [1, {layers_num - 1}] (layer 0 reads the "
                                 f"features and stays a plain TDNN layer), got {factorized}")
        self.factorized_layers = tuple(sorted(factorized))
        layers = []
        for i in range(layers_num):
            if i in self.factorized_layers:
                layers.append(FTDNN_Block(input_dim, hidden_dim[i], dilation=context[i], bottleneck_dim=opts.get("bottleneck_dim", 128),
                                          bypass_scale=opts.get("bypass_scale", 0.66), bn_first=self.bn_first))
            else:
                layers.append(TDNN_Block(input_dim, hidden_dim[i], dilation=context[i], stride=1, bn_first=self.bn_first))
            input_dim = hidden_dim[i]
        self.tdnn = nn.Sequential(*layers)
        self.pooling_type = opts["pooling"]
        if opts["pooling"] == "statistic":
            self.pooling = MeanStdPooling()
        elif opts["pooling"] == "average":
            self.pooling = Marker("AdaptiveAvgPool1d(1)")
        elif opts["pooling"] == "attentive_statistic":
            self.pooling = AttentiveStatPooling(hidden_dim[-1], attention_hidden_size)
        elif opts["pooling"] == "multi_head_attention":
            # (build-owned keys: attention_heads, default 4; attention_hidden_size an int -- every head that width -- or a list)
            ahs = attention_hidden_size if isinstance(attention_hidden_size, int) else list(attention_hidden_size)
            self.pooling = MultiHeadAttention(hidden_dim[-1], opts.get("attention_heads", 4), ahs)
        else:
            raise NotImplementedError("Other pooling method has not implemented.")
        if opts["pooling"] == "multi_head_attention":
            self.fc1 = LinearParams(self.pooling.output_size, embedding_dim)
        elif opts["pooling"] in ("statistic", "attentive_statistic"):
            self.fc1 = LinearParams(hidden_dim[-1] * 2, embedding_dim)
        elif opts["pooling"] == "average":
            self.fc1 = LinearParams(hidden_dim[-1], embedding_dim)
        else:
            raise ValueError("pooling method is wrong!")
        self.bn1 = BatchNormParams(embedding_dim)
        self.fc2 = LinearParams(embedding_dim, embedding_dim)
        self.bn2 = BatchNormParams(embedding_dim)

    def _exp(self, name: str) -> int:
        """Activation exponent of a tensor of the f16x3 pack: "in" (the features), "t<i>" (output of TDNN layer i = input of
        layer i + 1; the last one also scales the pooled statistics that fc1 reads).  Zero unless a calibration set it."""
        if packing.PRECISION != "f16x3":
            return 0
        if name == f"t{len(self.tdnn) - 1}" and self.pooling_type in ("attentive_statistic", "multi_head_attention"):
            return 0            # (the attention scores are not homogeneous in their input: that tensor stays unscaled)
        return packing.act_exponents(self).get(name, 0)

    def _pack(self, device):
        def ss(bn):
            sc, sh = packing.bn_scale_shift(bn)
            return sc.float().to(device), sh.float().to(device)
        n = len(self.tdnn)
        e = [self._exp("in")] + [self._exp(f"t{i}") for i in range(n)]
        pk = {"tdnn": [b.pack(device, e[i], e[i + 1]) for i, b in enumerate(self.tdnn)],
              "fc1": packing.pack_linear(self.fc1.weight, self.fc1.bias, None, device, e_in=e[n], e_out=0),
              "fc2": packing.pack_linear(self.fc2.weight, self.fc2.bias, None, device),
              "bn1": ss(self.bn1), "bn2": ss(self.bn2), "e_in": e[0], "e_last": e[n]}
        if e[0]:
            pk["in_scale"] = torch.full((1,), 2.0 ** e[0], dtype=torch.float32, device=device)
        return pk

    def _to_ntc(self, x: Tensor, split: bool = False, pad32: bool = False) -> Tensor:
        """[B,F,T] -> [B,T,Fp] channels-last; ``split``: Fp = F rounded up to 32, split activation format (``pad32``: that width, fp32)."""
        if x.dim() == 4:            # [B,1,F,T] (the north-star / train_audio.py:183-184 resnet layout)
            x = x.squeeze(1)
        if x.dim() != 3 or x.shape[1] != self.input_dim:
            raise ValueError(f"SpeakerEmbNet expects [B,{self.input_dim},T] features, got {tuple(x.shape)}")
        return ops.nct_to_ntc(x.contiguous().float(), pad_to=packing.pad_channels(self.input_dim, 32 if (split or pad32) else 4),
                              out_split=split)

    def _train_pad(self) -> int:
        """Channels of the training step's first tensor: F zero-padded to 32 when the first layer can then run on the split-fp16 kernels."""
        from . import autograd_video as av
        pad32 = av.TRAIN_CONV == "f16x3" and self.input_dim % 32 != 0 and self.tdnn[0].output_dim % 4 == 0
        return packing.pad_channels(self.input_dim, 32 if pad32 else 4)

    def _to_ntc_padded(self, x: Tensor) -> Tensor:
        if x.dim() == 4:
            x = x.squeeze(1)
        if x.dim() != 3 or x.shape[1] != self.input_dim:
            raise ValueError(f"SpeakerEmbNet expects [B,{self.input_dim},T] features, got {tuple(x.shape)}")
        return ops.nct_to_ntc(x.contiguous().float(), pad_to=self._train_pad())

    def _require_waves(self, x: Tensor) -> Tensor:
        if x.dim() != 2:
            raise ValueError(f"SpeakerEmbNet(arch: sincnet): the encoder takes waveforms [B, S] (its first layer is the sinc filter bank), "
                             f"got a tensor of shape {tuple(x.shape)}")
        return x.contiguous().float()

    def _extract_embedding_train(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        """extract_embedding under model.train() (train_audio.py:167-183): batch-statistics BatchNorm, every
        layer differentiable.  Each step is a torch.autograd Function whose forward and backward are dlip_*
        launches (deeplip_amd/autograd.py: TDNNBlockTrainFn, MeanStdPoolFn, LinearFn, BNRowsActFn)."""
        from . import autograd as ag
        if self.pooling_type not in ("statistic", "attentive_statistic", "multi_head_attention"):
            raise NotImplementedError("train-mode encoder: pooling 'statistic' (the shipped configs), 'attentive_statistic' or "
                                      "'multi_head_attention'")
        if self.input_dim % 4:
            raise ValueError("train-mode encoder: input_dim must be a multiple of 4")
        # [B,T,F] channels-last; F zero-padded to a multiple of 32 when the first layer can then run on the split-fp16 kernels
        # (24 features: the exact-fp32 kernel took 0.55 ms per launch on it, 1.1 of a 15 ms step at B = 256)
        if self.sinc is not None:
            # the sinc layer writes that tensor itself, channels-last and padded: no transpose between the layer and the first block
            h, _ = self.sinc.features(self._require_waves(x), None, channels_last_pad=self._train_pad())
        else:
            h = self._to_ntc_padded(x)
        from . import autograd_video as av
        av.prepare_weights(self)                           # the step's split weight images (forward and data-gradient banks): one launch
        pend = None                                        # (a block's activated output is not stored when the next block takes it on load)
        # (round 6) the LAST block's activated output is not stored either when the statistics pooling takes it on load (ABI 48)
        # ... and the pooling's BACKWARD writes nothing: the last block's BatchNorm backward forms that gradient per loaded value (hand_over)
        last_on_load = self.pooling_type == "statistic" and ag.POOL_BN_ON_LOAD
        n = len(self.tdnn)
        hand_over = False
        for i, blk in enumerate(self.tdnn):
            if i + 1 == n and last_on_load:
                T_out = h.shape[1] - blk.dilation * (blk.kernel_size - 1) + 2 * blk.padding
                hand_over = ag.POOL_BWD_ON_LOAD and h.shape[0] * T_out > ag.BN_SMALL_ROWS and T_out > 1 and blk.bn_first and ag.BN_ON_LOAD
            defer = (2 if hand_over else True) if (i + 1 < n or last_on_load) else False
            if isinstance(blk, FTDNN_Block):
                h, pend = ag.ftdnn_block_train(h, blk, pending=pend, defer=defer)
            else:
                h, pend = ag.tdnn_block_train(h, blk, pending=pend, defer=defer)
        # (pooling.py:24-26 | :87-107: attention scores, softmax over frames, weighted mean and std, all differentiable)
        if self.pooling_type == "statistic":
            h = ag.meanstd_pool(h, pending=pend, hand_over=hand_over and pend is not None)
        elif self.pooling_type == "attentive_statistic":
            h = ag.attentive_stat_pool(h, self.pooling)
        else:
            h = ag.mh_attentive_stat_pool(h, self.pooling)
        x_a = ag.linear(h, self.fc1.weight, self.fc1.bias)
        h = ag.bn_rows_act_train(x_a, self.bn1, LRELU, act_first=not self.bn_first)
        xv = ag.linear(h, self.fc2.weight, self.fc2.bias)
        return xv, x_a

    def frames_consumed(self) -> int:
        """Frames the stack's valid convolutions take off an utterance: T' = T - frames_consumed() (22 for the E-TDNN)."""
        return sum(b.dilation * (b.kernel_size - 1) - 2 * b.padding for b in self.tdnn)

    @arith.guarded_eval
    @_lib.scoped_eval
    def extract_embedding(self, x: Tensor, lengths=None, taps: Optional[dict] = None) -> Tuple[Tensor, Tensor]:
        """[B,F,T] -> (xv [B,E] = fc2 output, x_a [B,E] = fc1 output)   (tdnn.py:89-101).

        ``lengths`` (list / int32 tensor [B]; build-owned): a RAGGED batch -- x is zero-padded to the longest utterance and
        utterance b has lengths[b] frames.  Row b then equals ``extract_embedding(x[b:b+1, :, :lengths[b]])``, the reference's
        one-utterance-at-a-time test loop (train_fusion.py:334-338, train_audio.py:343-373): the convolutions are valid ones, so
        an output frame t < lengths[b] - frames_consumed() never reads the padding, and the statistics pooling covers exactly
        those frames.  A device tensor is read by the kernels directly (a recorded plan replays with new lengths)."""
        if self.training:
            if lengths is not None:
                raise NotImplementedError("train mode crops every utterance of a batch to one length (datasets.py:112-115)")
            return self._extract_embedding_train(x)
        _lib.check_range()      # an overflow reported by an earlier f16x3 launch surfaces here (host read, no sync)
        shrink = self.frames_consumed()
        if self.sinc is not None:
            # arch: sincnet -- x is the waveform batch and ``lengths`` counts samples; the layer (exact fp32 in every arithmetic mode)
            # hands over [B,F,NF] and the rows' frame counts on the device
            x = self._require_waves(x)
            if lengths is not None and not (isinstance(lengths, Tensor) and lengths.is_cuda):
                short = [int(l) for l in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)
                         if 1 <= int(l) and self.sinc.frames_for_samples(int(l)) < shrink + 2]
                if short:
                    raise ValueError(f"lengths: {min(short)} samples make fewer than the {shrink + 2} frames the encoder needs")
            with torch.no_grad():
                x, nf = self.sinc.features(x, lengths)
            lengths = None if lengths is None else nf
        p = _cached_pack(self, x.device, self._pack)
        lens = ops.lengths_i32(lengths, x.device, n=x.shape[0], lo=shrink + 2, hi=x.shape[-1])   # >= 2 pooled frames (unbiased std)
        len_add = -shrink
        # f16x3 packing: frame-level activations travel between layers as (hi, lo) fp16 pairs, written
        # by the producing layer's epilogue; the last layer hands fp32 to the pooling kernel, which
        # writes the utterance statistics in that format again for fc1.
        f16x3 = p["tdnn"][0].wscale is not None
        packing.calib_note(self, "in", x)                    # (a calibrating exact pass notes the tensors' magnitudes; no-op otherwise)
        if f16x3 and p["e_in"]:
            # an input whose gain put it outside the split format (calibrated: packing.act_exponents): 2^e x, then the split
            h = ops.split_pack_scaled(self._to_ntc(x, split=False, pad32=True), p["in_scale"])
        else:
            h = self._to_ntc(x, split=f16x3)
        if taps is not None and f16x3 and (p["e_in"] or p["e_last"] or packing.act_exponents(self)):
            raise NotImplementedError("taps of a model with calibrated activation exponents (the intermediate tensors are scaled)")
        split, n = f16x3, len(self.tdnn)
        pooled = None
        for i, (blk, bp) in enumerate(zip(self.tdnn, p["tdnn"])):
            nxt = bp.wscale is not None and i + 1 < n and blk.output_dim % 32 == 0
            if (i + 1 == n and split and FUSE_POOL and taps is None and self.pooling_type == "statistic"
                    and blk.output_dim % 4 == 0 and isinstance(blk, TDNN_Block)):
                pooled = blk.run_pooled(h, bp, lens, len_add)       # None when an utterance is shorter than a workgroup tile
                if pooled is not None:
                    break
            h = blk.run_ntc(h, bp, x_split=split, out_split=nxt)
            packing.calib_note(self, f"t{i}", h)
            split = nxt
        if taps is not None:
            taps["tdnn_out"] = h
        pooled_split = False
        if pooled is not None:
            pooled_split = True
            h = ops.pool_finish(pooled, "meanstd", out_split=True)
        elif self.pooling_type == "statistic":
            pooled_split = f16x3 and h.shape[2] % 4 == 0
            h = ops.meanstd_pool(h, out_split=pooled_split, lengths=lens, len_add=len_add)
        elif self.pooling_type == "average":
            h = ops.time_mean(h, lens, len_add)
        else:
            h = self.pooling.run_ntc(h, lens, len_add)
        if taps is not None:
            taps["pooled"] = ops.split_unpack(h)[:, :self.fc1.in_features].contiguous() if pooled_split else h
        x_a = ops.linear(h, p["fc1"].w, p["fc1"].b, w_scale=p["fc1"].wscale, x_split=pooled_split)
        h = ops.affine_act(x_a, p["bn1"][0], p["bn1"][1], LRELU, act_first=not self.bn_first)
        xv = ops.linear(h, p["fc2"].w, p["fc2"].b, w_scale=p["fc2"].wscale)
        return xv, x_a

    @arith.guarded_eval
    def forward(self, x: Tensor) -> Tensor:
        """tdnn.py:103-111: extract_embedding()[0] -> bn2 / LeakyReLU."""
        xv, _ = self.extract_embedding(x)
        if self.training:
            from . import autograd as ag
            return ag.bn_rows_act_train(xv, self.bn2, LRELU, act_first=not self.bn_first)
        p = _cached_pack(self, x.device, self._pack)
        return ops.affine_act(xv, p["bn2"][0], p["bn2"][1], LRELU, act_first=not self.bn_first)
