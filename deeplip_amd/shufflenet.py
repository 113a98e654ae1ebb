"""ShuffleNetV2 lip-clip trunk on the HIP engine: host-side mirror of the reference's ``models/video_models/shufflenetv2.py`` (same
class names, constructor signatures and attribute = state-dict key names) plus the packing and the eval-mode ``run()`` that
``Lipreading(backbone_type='shufflenet')`` (model.py:72-78) drives.  Exact fp32 under every arithmetic mode.

Channel layout.  An InvertedResidual unit's output has 2h logical channels (channel_shuffle order, shufflenetv2.py:27-40: branch
channel j at 2j for the first branch, 2j + 1 for the second).  It is stored as two halves padded to hp = h rounded up to 4
channels: logical L at physical L (L < h) or hp + L - h (L >= h), pitch 2hp, the 2(hp - h) padding channels zero (written by
their producer).  A stride-1 unit's x1 / x2 (shufflenetv2.py:98-99) are then the aligned slices [0, hp) and [hp, 2hp); consumers
of a whole tensor see zero weights on the padding channels.  h = 58 (width 1.0, stage 2) and 122 (width 2.0) are the padded
cases; every other width and stage has h % 4 == 0 and no padding.

Launches: stem, max pool, then per unit 2 (stride 1: banch2's first 1x1 on dlip_conv_nhwc_f32, then dlip_shuffle_dwpw_f32 with the
depthwise on load, the shuffled store and x1's copy) or 3 (stride 2: banch1 and banch2's tail on dlip_shuffle_dwpw_f32, banch2's
first 1x1 on dlip_conv_nhwc_f32), conv_last (dlip_conv_nhwc_f32) and AvgPool2d(3) (dlip_avgpool3_nhwc_f32): 38 per forward.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from . import ops, packing
from .holders import BatchNormParams, ConvParams, LinearParams, Marker

Tensor = torch.Tensor

STAGE_OUT_CHANNELS = {
    0.5: [-1, 24, 48, 96, 192, 1024],
    1.0: [-1, 24, 116, 232, 464, 1024],
    1.5: [-1, 24, 176, 352, 704, 1024],
    2.0: [-1, 24, 244, 488, 976, 2048],
}


# ------------------------------------------------------------------------------------------
# shufflenetv2.py: parameter holders
# ------------------------------------------------------------------------------------------
def conv_bn(inp, oup, stride):
    """shufflenetv2.py:11-16 (3x3 conv + BN + ReLU; stride lives in the engine call)."""
    c = ConvParams(inp, oup, (3, 3), bias=False)
    c.stride = stride
    return nn.Sequential(c, BatchNormParams(oup), Marker("ReLU"))


def conv_1x1_bn(inp, oup):
    """shufflenetv2.py:19-24."""
    return nn.Sequential(ConvParams(inp, oup, (1, 1), bias=False), BatchNormParams(oup), Marker("ReLU"))


def channel_shuffle(x, groups):
    """shufflenetv2.py:27-40: kept for API completeness; a pure index permutation (the engine's units store their outputs in
    this order directly)."""
    b, c, h, w = x.shape
    return x.view(b, groups, c // groups, h, w).transpose(1, 2).contiguous().view(b, -1, h, w)


def _dw(c):
    return ConvParams(1, c, (3, 3), bias=False)     # Conv2d(c, c, 3, groups=c): weight [c, 1, 3, 3]


class InvertedResidual(nn.Module):
    """shufflenetv2.py:42-105.  Eval-mode arithmetic runs through the owning Lipreading (ShuffleTrunk.run)."""

    def __init__(self, inp, oup, stride, benchmodel):
        super().__init__()
        self.benchmodel = benchmodel
        self.stride = stride
        assert stride in [1, 2]
        self.inp, self.oup = inp, oup
        oup_inc = oup // 2
        if benchmodel == 1:
            self.banch2 = nn.Sequential(
                ConvParams(oup_inc, oup_inc, (1, 1), bias=False), BatchNormParams(oup_inc), Marker("ReLU"),
                _dw(oup_inc), BatchNormParams(oup_inc),
                ConvParams(oup_inc, oup_inc, (1, 1), bias=False), BatchNormParams(oup_inc), Marker("ReLU"))
        else:
            self.banch1 = nn.Sequential(
                _dw(inp), BatchNormParams(inp),
                ConvParams(inp, oup_inc, (1, 1), bias=False), BatchNormParams(oup_inc), Marker("ReLU"))
            self.banch2 = nn.Sequential(
                ConvParams(inp, oup_inc, (1, 1), bias=False), BatchNormParams(oup_inc), Marker("ReLU"),
                _dw(oup_inc), BatchNormParams(oup_inc),
                ConvParams(oup_inc, oup_inc, (1, 1), bias=False), BatchNormParams(oup_inc), Marker("ReLU"))

    def forward(self, x):
        raise RuntimeError("InvertedResidual: the arithmetic runs in the owning Lipreading's engine (ShuffleTrunk.run)")


class ShuffleNetV2(nn.Module):
    """shufflenetv2.py:108-170 (same sub-modules; Lipreading keeps features, conv_last and globalpool)."""

    def __init__(self, n_class=1000, input_size=224, width_mult=2.):
        super().__init__()
        assert input_size % 32 == 0, "Input size needs to be divisible by 32"
        self.stage_repeats = [4, 8, 4]
        if width_mult not in STAGE_OUT_CHANNELS:
            raise ValueError(
                """Width multiplier should be in [0.5, 1.0, 1.5, 2.0]. Current value: {}""".format(width_mult))
        self.stage_out_channels = list(STAGE_OUT_CHANNELS[width_mult])
        input_channel = self.stage_out_channels[1]
        self.conv1 = conv_bn(3, input_channel, 2)
        self.maxpool = Marker("MaxPool2d(3, 2, 1)")
        features = []
        for idxstage, numrepeat in enumerate(self.stage_repeats):
            output_channel = self.stage_out_channels[idxstage + 2]
            for i in range(numrepeat):
                features.append(InvertedResidual(input_channel, output_channel, 2 if i == 0 else 1, 2 if i == 0 else 1))
                input_channel = output_channel
        self.features = nn.Sequential(*features)
        self.conv_last = conv_1x1_bn(input_channel, self.stage_out_channels[-1])
        self.globalpool = nn.Sequential(Marker(f"AvgPool2d({int(input_size / 32)})"))
        self.classifier = nn.Sequential(LinearParams(self.stage_out_channels[-1], n_class))

    def forward(self, x):
        raise NotImplementedError("standalone ShuffleNetV2 (the 3-channel image classifier) is not implemented; "
                                  "Lipreading(backbone_type='shufflenet') runs its features / conv_last / globalpool")


# ------------------------------------------------------------------------------------------
# layout + packing
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Layout:
    """Physical layout of a trunk tensor: ``C`` logical channels; ``half`` = 0 (stored as is) or h = C / 2 with each half padded
    to ``hp`` channels."""
    C: int
    half: int = 0
    hp: int = 0

    @property
    def pitch(self) -> int:
        return 2 * self.hp if self.half else self.C

    def phys(self) -> Tensor:
        """int64 [C]: physical channel of each logical channel (a bijection onto the non-padding channels)."""
        return phys_map(self.C, self.half, self.hp) if self.half else torch.arange(self.C)

    def to_logical(self, y: Tensor) -> Tensor:
        """[..., pitch] -> [..., C] in logical (channel_shuffle) order (taps and tests; not on the forward path)."""
        return y.index_select(-1, self.phys().to(y.device))


def unit_layout(oup: int) -> Layout:
    h = oup // 2
    return Layout(oup, h, packing.pad_channels(h, 4))


def phys_map(C: int, h: int, hp: int) -> Tensor:
    L = torch.arange(C)
    return torch.where(L < h, L, L - h + hp)


def shuffle_positions(K: int, hp: int, par: int) -> Tensor:
    """Physical channel that output channel j of a unit's branch (``par`` 0: first branch / x1, 1: banch2) is stored at."""
    return phys_map(2 * K, K, hp)[2 * torch.arange(K) + par]


def _round(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _gemm_weights(w_kc: Tensor, phys_in: Tensor, cin_phys: int) -> Tensor:
    """fp64 [K, C] (logical input channels) -> k-major [Cp, Kp] over the physical input channels (zeros elsewhere)."""
    K = w_kc.shape[0]
    out = torch.zeros(_round(cin_phys, 32), _round(K, 64), dtype=torch.float64)
    out[phys_in, :K] = w_kc.t()
    return out


def _dw_weights(conv, bn, phys_in: Tensor, cin_phys: int):
    """Depthwise 3x3 + BN folded -> ([9, cin_phys] tap-major, [cin_phys]) over the physical channels."""
    w, b = packing.fold(conv.weight, None, bn)               # [C, 1, 3, 3]
    ww = torch.zeros(9, cin_phys, dtype=torch.float64)
    bb = torch.zeros(cin_phys, dtype=torch.float64)
    ww[:, phys_in] = w.reshape(-1, 9).t()
    bb[phys_in] = b
    return ww, bb


def _pw_krsc(conv, bn, phys_in: Tensor, cin_phys: int, k_pad: int):
    """1x1 + BN folded -> dlip_conv_nhwc_f32 weights [k_pad, 1, 1, cin_phys] and bias [k_pad] (zero rows for the padding outputs)."""
    w, b = packing.fold(conv.weight, None, bn)                # [K, C, 1, 1]
    K = w.shape[0]
    ww = torch.zeros(k_pad, 1, 1, cin_phys, dtype=torch.float64)
    bb = torch.zeros(k_pad, dtype=torch.float64)
    ww[:K, 0, 0, phys_in] = w.reshape(K, -1)
    bb[:K] = b
    return ww, bb


@dataclass
class UnitPack:
    stride: int
    K: int                          # branch width h
    hp: int
    pw1: packing.Packed             # banch2's first 1x1 (dlip_conv_nhwc_f32), hp outputs
    b2: Dict[str, Tensor]           # banch2's tail: dw_w, dw_b, w, b
    b1: Optional[Dict[str, Tensor]] = None      # banch1 (stride 2)


def _f32(t: Tensor, device) -> Tensor:
    return t.to(dtype=torch.float32).contiguous().to(device)


def pack_unit(u: InvertedResidual, lin: Layout, device) -> UnitPack:
    lout = unit_layout(u.oup)
    h, hp = lout.half, lout.hp
    zero_slope = packing.const_slope(hp, 0.0, device)
    ident_h = torch.arange(h)
    # banch2 tail: depthwise over t [.., hp] (channels [0, h) live), then the 1x1 to h outputs
    dww, dwb = _dw_weights(u.banch2[3], u.banch2[4], ident_h, hp)
    w2, b2 = packing.fold(u.banch2[5].weight, None, u.banch2[6])
    b2 = {"dw_w": _f32(dww, device), "dw_b": _f32(dwb, device),
          "w": _f32(_gemm_weights(w2.reshape(h, h), ident_h, hp), device), "b": _f32(b2, device)}
    if u.benchmodel == 1:
        # x2 = logical [h, 2h) of the input = physical [hp, hp + h): read as the hp-channel slice [hp, 2hp) (zero padding included)
        w1, bias1 = _pw_krsc(u.banch2[0], u.banch2[1], ident_h, hp, hp)
        pw1 = packing.Packed(_f32(w1, device), _f32(bias1, device), zero_slope)
        return UnitPack(1, h, hp, pw1, b2)
    phys_in = lin.phys()
    w1, bias1 = _pw_krsc(u.banch2[0], u.banch2[1], phys_in, lin.pitch, hp)
    pw1 = packing.Packed(_f32(w1, device), _f32(bias1, device), zero_slope)
    dww, dwb = _dw_weights(u.banch1[0], u.banch1[1], phys_in, lin.pitch)
    wb1, bb1 = packing.fold(u.banch1[2].weight, None, u.banch1[3])
    b1 = {"dw_w": _f32(dww, device), "dw_b": _f32(dwb, device),
          "w": _f32(_gemm_weights(wb1.reshape(h, -1), phys_in, lin.pitch), device), "b": _f32(bb1, device)}
    return UnitPack(2, h, hp, pw1, b2, b1)


def pack_stem24(conv, bn, slope: Optional[Tensor], device) -> packing.Packed:
    """frontend3D.0 [24,1,5,7,7] + frontend3D.1 -> k-major [248, 32] (245 taps + 3 zero rows, channels 24..31 zero), bias [24]."""
    w, b = packing.fold(conv.weight, None, bn)
    K = w.shape[0]
    if K != 24:
        raise ValueError(f"pack_stem24: {K} output channels")
    wp = torch.zeros(248, 32, dtype=torch.float64)
    wp[:245, :K] = w.reshape(K, 245).t()
    return packing.Packed(_f32(wp, device), _f32(b, device), slope)


def run_unit(p: UnitPack, x: Tensor, lin: Layout) -> Tensor:
    """x [N,H,W,lin.pitch] -> the unit's output [N,Ho,Wo,2hp] (Layout unit_layout(2K))."""
    N, H, W, _ = x.shape
    if p.stride == 1:
        t = ops.conv_nhwc(x, p.pw1.w, p.pw1.b, slope=p.pw1.slope, in_channels=p.hp, in_channel_offset=p.hp)
        return ops.shuffle_dwpw(t, p.b2["w"], p.b2["b"], dw_w=p.b2["dw_w"], dw_b=p.b2["dw_b"], stride=1, hp=p.hp, par=1,
                                passthrough=x)
    y = ops.shuffle_dwpw(x, p.b1["w"], p.b1["b"], dw_w=p.b1["dw_w"], dw_b=p.b1["dw_b"], stride=2, hp=p.hp, par=0)
    t = ops.conv_nhwc(x, p.pw1.w, p.pw1.b, slope=p.pw1.slope)
    return ops.shuffle_dwpw(t, p.b2["w"], p.b2["b"], dw_w=p.b2["dw_w"], dw_b=p.b2["dw_b"], stride=2, hp=p.hp, par=1, out=y)


def final_map_size(H: int, W: int):
    """The last feature map of an H x W clip: stem (stride 2), max pool (stride 2), three stride-2 stages."""
    h, w = H // 2, W // 2
    for _ in range(4):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return h, w


def check_input_size(H: int, W: int) -> None:
    h, w = final_map_size(H, W)
    if not (3 <= h <= 5 and 3 <= w <= 5):
        raise ValueError(f"ShuffleNet trunk: a {H}x{W} clip leaves a {h}x{w} map, and AvgPool2d(3) (model.py:75, input_size 96) "
                         "gives one feature vector per frame only for maps of 3 to 5 pixels a side (e.g. 88 x 88 or 112 x 112)")


class ShuffleTrunk(nn.Sequential):
    """``Lipreading.trunk`` for the ShuffleNet backbone: Sequential(features, conv_last, globalpool) as model.py:74 builds it (keys
    trunk.0.* / trunk.1.*), plus pack() / run()."""

    @staticmethod
    def wants_split(packed) -> bool:
        return False           # exact fp32 only: no split-fp16 packing

    def exponent_groups(self):
        return []

    def units(self) -> List[InvertedResidual]:
        return list(self[0])

    def layouts(self) -> List[Layout]:
        """Layout of the trunk input (the 24-channel stem) and of every unit's output."""
        out = [Layout(self.units()[0].inp)]
        for u in self.units():
            out.append(unit_layout(u.oup))
        return out

    def pack(self, device):
        lays = self.layouts()
        units = [pack_unit(u, lin, device) for u, lin in zip(self.units(), lays[:-1])]
        conv, bn = self[1][0], self[1][1]
        K = conv.weight.shape[0]
        w, b = _pw_krsc(conv, bn, lays[-1].phys(), lays[-1].pitch, K)
        last = packing.Packed(_f32(w, device), _f32(b, device), packing.const_slope(K, 0.0, device))
        return {"units": units, "last": last, "layouts": lays}

    def run(self, x: Tensor, packed, taps: Optional[dict] = None) -> Tensor:
        """x [N,H,W,24] (the pooled stem) -> [N, backend_out]."""
        lays = packed["layouts"]
        for i, (p, lin) in enumerate(zip(packed["units"], lays[:-1])):
            x = run_unit(p, x, lin)
            if taps is not None and i in (3, 11, 15):
                taps[{3: "stage2", 11: "stage3", 15: "stage4"}[i]] = lays[i + 1].to_logical(x)
        last = packed["last"]
        y = ops.conv_nhwc(x, last.w, last.b, slope=last.slope)
        if taps is not None:
            taps["conv_last"] = y
        return ops.avgpool3(y)
