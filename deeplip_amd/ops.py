"""Thin tensor-level wrappers over the C ABI (include/deeplip_hip.h).

PyTorch is plumbing here: it owns the device memory (``torch.empty``) and the stream; every
arithmetic op is one ``dlip_*`` call on ``torch.cuda.current_stream()``.  Inputs must be fp32
CUDA tensors; nothing in this module computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import ConvDesc, call, lib
from ._lib import ptr, stream_handle    # noqa: F401  (tests import them from here)

Tensor = torch.Tensor

# Optional measurement hook (bench.py): an object with begin(kernel_name, flops) -> token and
# end(token), called around every MFMA kernel launch on the current stream.  None = no overhead.
LAUNCH_HOOK = None

# Set by deeplip_amd.plan.StepPlan while a step is warmed up / recorded: every result tensor then comes from
# the plan's arena (same blocks in both passes), so nothing is allocated while the stream is being captured.
ARENA = None


def _empty(shape, device, dtype=torch.float32) -> Tensor:
    a = ARENA
    if a is None:
        return torch.empty(shape, device=device, dtype=dtype)
    return a.take(tuple(shape), device, dtype)


def _req(t: Optional[Tensor], name: str, dtype=torch.float32) -> None:
    if t is None:
        return
    if not t.is_cuda:
        raise _lib.DeepLipHipError(f"{name}: expected a CUDA (ROCm) tensor; deeplip_amd has no CPU path")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous tensor")


def conv_out_size(n: int, k: int, stride: int, pad: int, dil: int) -> int:
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _conv_desc(N, H, W, C, K, R, S, stride, pad, dil, ldx=None, ldy=None, ldr=0) -> ConvDesc:
    return ConvDesc(N, H, W, C, K, R, S, stride[0], stride[1], pad[0], pad[1], dil[0], dil[1], conv_out_size(H, R, stride[0], pad[0], dil[0]),
                    conv_out_size(W, S, stride[1], pad[1], dil[1]), C if ldx is None else ldx, K if ldy is None else ldy, ldr)


def _conv_label(d: ConvDesc, mode: int, epilogue: int, tag: str = "", C2: int = 0, unaligned: bool = False) -> str:
    """The kernel instance this launch runs on, as a profiler names it: dlip_conv_route's answer (mode, epilogue: see the header)."""
    kind, bm, bn = C.c_int32(), C.c_int32(), C.c_int32()
    call("dlip_conv_route", C.byref(d), mode, epilogue, C2, int(unaligned), C.byref(kind), C.byref(bm), C.byref(bn))
    name = ("conv_igemm_f16x3_dma_kernel", "conv_win_f16x3_kernel", "conv_rows_f16x3_kernel", "conv_igemm_f16x3_kernel", "conv_igemm_f32_kernel")[kind.value]
    return f"{name}<{bm.value},{bn.value}{tag}>"


def conv_nhwc(x: Tensor, w_krsc: Tensor, bias: Optional[Tensor] = None, *, stride=(1, 1), pad=(0, 0),
              dil=(1, 1), residual: Optional[Tensor] = None, slope: Optional[Tensor] = None,
              post_scale: Optional[Tensor] = None, post_shift: Optional[Tensor] = None,
              out: Optional[Tensor] = None, out_channel_offset: int = 0,
              in_channels: Optional[int] = None, in_channel_offset: int = 0,
              w_scale: Optional[Tensor] = None, x_split: bool = False, out_split: bool = False,
              stats: Optional[Tensor] = None) -> Tensor:
    """x [N,H,W,Cx] (NHWC), w [K,R,S,C] -> y [N,Ho,Wo,Ky].

    ``out`` / ``out_channel_offset`` write the K result channels into a slice of a wider tensor
    (concat-free multibranch blocks); ``in_channels`` / ``in_channel_offset`` read a slice.
    With ``w_scale`` given, ``w_krsc`` is the split (hi, lo) fp16 packing of packing.split_weights
    ([K,R,S,C32] float32 view) and the launch goes to the 3 x f16-MFMA kernel; there ``x_split`` says
    x and residual hold the split activation format (``split_pack``) and ``out_split`` asks for it."""
    for t, n in ((x, "x"), (w_krsc, "w"), (bias, "bias"), (residual, "residual"), (slope, "slope"),
                 (post_scale, "post_scale"), (post_shift, "post_shift"), (out, "out")):
        _req(t, n)
    _req(w_scale, "w_scale")
    N, H, W, Cx = x.shape
    K, R, S, Cw = w_krsc.shape
    if w_scale is not None:        # split weights are channel-padded to a multiple of 32
        if in_channels is None:
            in_channels = min(Cx - in_channel_offset, Cw)
        if (in_channels + 31) // 32 * 32 != Cw:
            raise ValueError(f"conv_nhwc: split weights have C32={Cw}, input slice has {in_channels} channels")
        Cw = in_channels
    Cin = Cw if in_channels is None else in_channels
    if Cin != Cw or in_channel_offset + Cin > Cx:
        raise ValueError(f"conv_nhwc: weight C={Cw} does not match input slice [{in_channel_offset}:+{Cin}] of {Cx}")
    Ho = conv_out_size(H, R, stride[0], pad[0], dil[0])
    Wo = conv_out_size(W, S, stride[1], pad[1], dil[1])
    if out is None:
        out = _empty((N, Ho, Wo, K), x.device)
        out_channel_offset = 0
    if tuple(out.shape[:3]) != (N, Ho, Wo) or out_channel_offset + K > out.shape[3]:
        raise ValueError(f"conv_nhwc: bad output tensor {tuple(out.shape)} for result {(N, Ho, Wo, K)}")
    if residual is not None and (tuple(residual.shape[:3]) != (N, Ho, Wo) or residual.shape[3] < K):
        raise ValueError(f"conv_nhwc: residual {tuple(residual.shape)} does not match output {(N, Ho, Wo, K)}")
    for v, n in ((bias, "bias"), (slope, "slope"), (post_scale, "post_scale"), (post_shift, "post_shift")):
        if v is not None and v.numel() != K:
            raise ValueError(f"conv_nhwc: {n} has {v.numel()} elements, expected K={K}")
    if x_split or out_split:
        if w_scale is None:
            raise ValueError("conv_nhwc: the split activation format exists only on the f16x3 path (w_scale)")
        if x_split and (Cin % 32 or Cx % 32 or in_channel_offset % 32
                        or (residual is not None and (residual.shape[3] % 32 or K % 32))):
            raise ValueError("conv_nhwc: split input needs channel counts / offsets in multiples of 32")
        if out_split and (K % 32 or out.shape[3] % 32 or out_channel_offset % 32):
            raise ValueError("conv_nhwc: split output needs channel counts / offsets in multiples of 32")
    d = _conv_desc(N, H, W, Cin, K, R, S, stride, pad, dil, Cx, out.shape[3], residual.shape[3] if residual is not None else 0)
    xp = x.data_ptr() + 4 * in_channel_offset
    yp = out.data_ptr() + 4 * out_channel_offset
    hook = LAUNCH_HOOK
    if hook is not None:
        unaligned = yp % 16 != 0 or (residual is not None and residual.data_ptr() % 16 != 0)
        tok = hook.begin(_conv_label(d, 0 if w_scale is None else (3 if x_split else 1), 3 if stats is not None else int(out_split), unaligned=unaligned),
                         2.0 * N * Ho * Wo * K * R * S * Cin)
    if stats is not None:
        # the convolution's epilogue also leaves the column sums of y (dlip_conv_nhwc_stats_f16x3): conv_stats_chunks(...) said it can
        _req(stats, "stats", torch.float64)
        if not (x_split and w_scale is not None) or out_split or residual is not None or post_scale is not None or in_channel_offset or out_channel_offset:
            raise ValueError("conv_nhwc(stats=...): split input, fp32 output, no residual / post-affine / channel slices")
        _lib.ensure_conv_workspace()
        call("dlip_conv_nhwc_stats_f16x3", C.byref(d), xp, w_krsc, w_scale, bias, slope, yp, stats, stats.numel() * 8)
    elif w_scale is not None:
        if x_split:
            _lib.ensure_conv_workspace()
        call("dlip_conv_nhwc_f16x3", C.byref(d), xp, w_krsc, w_scale, bias, residual, slope, post_scale, post_shift, yp,
             int(x_split) | 2 * int(out_split))
    else:
        call("dlip_conv_nhwc_f32", C.byref(d), xp, w_krsc, bias, residual, slope, post_scale, post_shift, yp)
    if hook is not None:
        hook.end(tok)
    return out


def conv_stats_chunks(N, H, W, Cin, K, R, S, stride=(1, 1), pad=(0, 0), dil=(1, 1)) -> int:
    """How many partial rows conv_nhwc(..., stats=...) writes for this split-input, fp32-output launch (0: no statistics epilogue
    for the shape -- launch the plain convolution and let the BatchNorm make its own pass)."""
    return int(lib().dlip_conv_stats_chunks(C.byref(_conv_desc(N, H, W, Cin, K, R, S, stride, pad, dil))))


def conv2_nhwc(x: Tensor, x2: Tensor, w_split: Tensor, bias: Tensor, w_scale: Tensor, *, stride=(1, 1), pad=(0, 0),
               dil=(1, 1), stride2=(2, 2), residual: Optional[Tensor] = None, slope: Optional[Tensor] = None,
               out_split: bool = True) -> Tensor:
    """One reduction over two sources (dlip_conv2_nhwc_f16x3): y = act(conv(x, w[..., taps]) + conv1x1(x2[::s2], w[..., tail])
    + bias).  x [N,H,W,C], x2 [N,H2,W2,C2], both in the split activation format; ``w_split`` [K, R*S*C32 + C2] float32 view
    of the jointly scaled split weights (packing.pack_conv2d_shortcut).  The BasicBlock shortcut (resnet.py:13-17,62-66)."""
    for t, n in ((x, "x"), (x2, "x2"), (w_split, "w"), (bias, "bias"), (w_scale, "w_scale"), (residual, "residual"), (slope, "slope")):
        _req(t, n)
    N, H, W, Cx = x.shape
    N2, H2, W2, C2 = x2.shape
    K, RSC = w_split.shape
    R = S = 3 if (RSC - C2) == 9 * Cx else 1
    if N2 != N or RSC != R * S * Cx + C2 or Cx % 32 or C2 % 32:
        raise ValueError(f"conv2_nhwc: weights {tuple(w_split.shape)} do not match x {tuple(x.shape)} + x2 {tuple(x2.shape)}")
    d = _conv_desc(N, H, W, Cx, K, R, S, stride, pad, dil, ldr=K if residual is not None else 0)
    Ho, Wo = d.Ho, d.Wo
    if (Ho - 1) * stride2[0] >= H2 or (Wo - 1) * stride2[1] >= W2:
        raise ValueError("conv2_nhwc: the shortcut source does not cover the output grid")
    if out_split and K % 32:
        raise ValueError("conv2_nhwc: split output needs K % 32 == 0")
    out = _empty((N, Ho, Wo, K), x.device)
    if residual is not None and tuple(residual.shape) != (N, Ho, Wo, K):
        raise ValueError("conv2_nhwc: residual shape")
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin(_conv_label(d, 3, int(out_split), ",dual", C2), 2.0 * N * Ho * Wo * K * (R * S * Cx + C2))
    _lib.ensure_conv_workspace()
    call("dlip_conv2_nhwc_f16x3", C.byref(d), x, x2, H2, W2, C2, C2, stride2[0], stride2[1], w_split, w_scale, bias, residual, slope, None, None, out,
         1 | 2 * int(out_split))
    if hook is not None:
        hook.end(tok)
    return out


class Pooled:
    """Partial column sums of a pooled convolution (conv_pool) + what pool_finish needs to read them.  ``lengths`` (int32 CUDA
    [G] or None) with ``len_mul`` / ``len_add``: a ragged batch -- group g is valid for its first lengths[g] * len_mul + len_add rows."""
    __slots__ = ("partials", "M", "K", "tile_rows", "group_rows", "lengths", "len_mul", "len_add")

    def __init__(self, partials, M, K, tile_rows, group_rows, lengths=None, len_mul=1, len_add=0):
        self.partials, self.M, self.K, self.tile_rows, self.group_rows = partials, M, K, tile_rows, group_rows
        self.lengths, self.len_mul, self.len_add = lengths, len_mul, len_add


def lengths_i32(lengths, device, n: Optional[int] = None, lo: int = 1, hi: Optional[int] = None) -> Optional[Tensor]:
    """The length vector of a ragged batch as the int32 device tensor the kernels read.  A CUDA int32 tensor passes through
    untouched (what a recorded step plan needs: no host->device copy inside the step; its values are clamped on the device and
    are the caller's responsibility); host lists / arrays / CPU tensors are validated here -- ``n`` entries in [lo, hi]."""
    if lengths is None:
        return None
    if isinstance(lengths, Tensor) and lengths.is_cuda:
        if lengths.dtype != torch.int32:
            raise TypeError("lengths: a device tensor must be int32")
        if n is not None and lengths.numel() != n:
            raise ValueError(f"lengths: {lengths.numel()} entries for a batch of {n}")
        return lengths.contiguous()
    vals = [int(l) for l in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if n is not None and len(vals) != n:
        raise ValueError(f"lengths: {len(vals)} entries for a batch of {n}")
    if vals and (min(vals) < lo or (hi is not None and max(vals) > hi)):
        raise ValueError(f"lengths: values must lie in [{lo}, {hi}] (got {min(vals)} .. {max(vals)})")
    return torch.tensor(vals, dtype=torch.int32).to(device)


def conv_pool_tile_rows(x: Tensor, w_krsc: Tensor, *, stride=(1, 1), pad=(0, 0), dil=(1, 1)) -> int:
    """Rows of the workgroup tile conv_pool would use for this launch (group_rows must be >= it)."""
    N, H, W, Cx = x.shape
    K, R, S, Cw = w_krsc.shape
    d = _conv_desc(N, H, W, Cx, K, R, S, stride, pad, dil)
    bm = C.c_int32()
    if int(lib().dlip_conv_pool_partial_bytes(C.byref(d), C.byref(bm))) <= 0:
        raise _lib.DeepLipHipError("dlip_conv_pool_partial_bytes failed")
    return bm.value


def conv_pool(x: Tensor, w_krsc: Tensor, bias: Optional[Tensor], w_scale: Tensor, group_rows: int, *, stride=(1, 1),
              pad=(0, 0), dil=(1, 1), residual: Optional[Tensor] = None, slope: Optional[Tensor] = None,
              post_scale: Optional[Tensor] = None, post_shift: Optional[Tensor] = None,
              lengths: Optional[Tensor] = None, len_mul: int = 1, len_add: int = 0) -> Pooled:
    """dlip_conv_pool_f16x3: the convolution of conv_nhwc (split-format x / residual) whose output is never written --
    per workgroup tile only the fp64 column sums of y and y^2, cut at the boundaries of consecutive ``group_rows``-row
    groups.  pool_finish turns them into group means (AdaptiveAvgPool + temporal mean, resnet.py:125-126 +
    train_fusion.py:348) or mean | std (MeanStdPooling, pooling.py:24-26).  ``lengths`` (int32 CUDA, one per group): a
    ragged batch -- only the first lengths[g] * len_mul + len_add rows of group g are summed (and counted by pool_finish)."""
    for t, n in ((x, "x"), (w_krsc, "w"), (bias, "bias"), (w_scale, "w_scale"), (residual, "residual"), (slope, "slope"),
                 (post_scale, "post_scale"), (post_shift, "post_shift")):
        _req(t, n)
    _req(lengths, "lengths", torch.int32)
    N, H, W, Cx = x.shape
    K, R, S, Cw = w_krsc.shape
    if Cx % 32 or Cw != Cx:
        raise ValueError("conv_pool: split-format input with C % 32 == 0 and matching split weights required")
    d = _conv_desc(N, H, W, Cx, K, R, S, stride, pad, dil, ldr=K if residual is not None else 0)
    Ho, Wo = d.Ho, d.Wo
    if residual is not None and (tuple(residual.shape[:3]) != (N, Ho, Wo) or residual.shape[3] != K or K % 32):
        raise ValueError("conv_pool: residual shape")
    bm = C.c_int32()
    nbytes = int(lib().dlip_conv_pool_partial_bytes(C.byref(d), C.byref(bm)))
    if nbytes <= 0:
        raise _lib.DeepLipHipError("dlip_conv_pool_partial_bytes failed")
    if group_rows < bm.value:
        raise ValueError(f"conv_pool: group_rows {group_rows} < tile rows {bm.value}; use the unfused path")
    part = _empty((nbytes // 8,), x.device, torch.float64)
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin(_conv_label(d, 3, 2, ",pool"), 2.0 * N * Ho * Wo * K * R * S * Cx)
    _lib.ensure_conv_workspace()
    call("dlip_conv_pool_f16x3", C.byref(d), x, w_krsc, w_scale, bias, residual, slope, post_scale, post_shift, part, nbytes, group_rows, lengths,
         len_mul, len_add)
    if hook is not None:
        hook.end(tok)
    M = N * Ho * Wo
    if lengths is not None and lengths.numel() != (M + group_rows - 1) // group_rows:
        raise ValueError(f"conv_pool: {lengths.numel()} lengths for {(M + group_rows - 1) // group_rows} groups")
    return Pooled(part, M, K, bm.value, group_rows, lengths, len_mul, len_add)


def pool_finish(p: Pooled, mode: str = "mean", out_split: bool = False) -> Tensor:
    """Pooled partial sums -> [G,K] group means ('mean') or [G,2K] mean | unbiased std ('meanstd'; ``out_split``: [G, 2K
    rounded up to 32] in the split activation format)."""
    G = (p.M + p.group_rows - 1) // p.group_rows
    if mode == "mean":
        y = _empty((G, p.K), p.partials.device)
    else:
        y = _empty((G, (2 * p.K + 31) // 32 * 32 if out_split else 2 * p.K), p.partials.device)
    call("dlip_pool_finish_f32", p.partials, p.M, p.K, p.tile_rows, p.group_rows, p.lengths, p.len_mul, p.len_add, 0 if mode == "mean" else 1,
         int(out_split), y)
    return y


def linear(x: Tensor, w_kc: Tensor, bias: Optional[Tensor] = None, **kw) -> Tensor:
    """x [M,C] @ w [K,C]^T (+ epilogue) -> [M,K], through the same implicit-GEMM kernel."""
    M, Cx = x.shape
    K, Cw = w_kc.shape
    y = conv_nhwc(x.view(1, 1, M, Cx), w_kc.view(K, 1, 1, Cw), bias, **kw)
    return y.view(M, K)


def conv1d_ntc(x: Tensor, w_ksc: Tensor, bias: Optional[Tensor] = None, *, dilation: int = 1, pad: int = 0,
               **kw) -> Tensor:
    """x [B,T,C] (time-major, channels-last), w [K,S,C] -> [B,T',K]."""
    B, T, Cx = x.shape
    K, S, Cw = w_ksc.shape
    res = kw.pop("residual", None)
    out = kw.pop("out", None)
    if res is not None:
        res = res.view(B, 1, res.shape[1], res.shape[2])
    if out is not None:
        out = out.view(B, 1, out.shape[1], out.shape[2])
    y = conv_nhwc(x.view(B, 1, T, Cx), w_ksc.view(K, 1, S, Cw), bias, dil=(1, dilation), pad=(0, pad),
                  residual=res, out=out, **kw)
    return y.view(B, y.shape[2], y.shape[3])


def stem3d(x_bthw: Tensor, w_248xk: Tensor, bias: Tensor, slope: Optional[Tensor],
           w_scale: Optional[Tensor] = None) -> Tensor:
    """x [B,T,H,W] -> [(B*T), H/2, W/2, 64] (Conv3d 5x7x7 + folded BN + PReLU/ReLU).  With ``w_scale``
    the weights are the split-fp16 image of packing.split_stem_weights (3 x f16 MFMA kernel)."""
    for t, n in ((x_bthw, "x"), (w_248xk, "w"), (bias, "bias"), (slope, "slope"), (w_scale, "w_scale")):
        _req(t, n)
    B, T, H, W = x_bthw.shape
    if w_scale is not None:
        y = _empty((B * T, H // 2, W // 2, 64), x_bthw.device)
        hook = LAUNCH_HOOK
        if hook is not None:
            tok = hook.begin("stem3d_f16x3_kernel", 2.0 * B * T * (H // 2) * (W // 2) * 64 * 245)
        call("dlip_stem3d_bn_act_f16x3", x_bthw, w_248xk, w_scale, bias, slope, y, B, T, H, W, 64)
        if hook is not None:
            hook.end(tok)
        return y
    K = w_248xk.shape[1]
    if w_248xk.shape[0] != 248:
        raise ValueError("stem3d: weights must be packed [248, K]")
    y = _empty((B * T, H // 2, W // 2, K), x_bthw.device)
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin("stem3d_f32_kernel", 2.0 * B * T * (H // 2) * (W // 2) * K * 245)
    call("dlip_stem3d_bn_act_f32", x_bthw, w_248xk, bias, slope, y, B, T, H, W, K)
    if hook is not None:
        hook.end(tok)
    return y


def stem3d_pool(x_bthw: Tensor, w_img: Tensor, bias: Tensor, slope: Optional[Tensor], w_scale: Tensor,
                lengths: Optional[Tensor] = None) -> Tensor:
    """x [B,T,H,W] -> [(B*T), Hp, Wp, 64] in the split activation format: Conv3d 5x7x7 + folded BN +
    PReLU/ReLU + MaxPool3d((1,3,3),(1,2,2),(0,1,1)) in one kernel (split-fp16 weights image only).  ``lengths`` (int32 CUDA [B]):
    a zero-padded ragged batch (dataset.py:123-139) -- frames t >= lengths[b] are read as zeros whatever x holds there."""
    for t, n in ((x_bthw, "x"), (w_img, "w"), (bias, "bias"), (slope, "slope"), (w_scale, "w_scale")):
        _req(t, n)
    _req(lengths, "lengths", torch.int32)
    B, T, H, W = x_bthw.shape
    if lengths is not None and lengths.numel() != B:
        raise ValueError(f"stem3d_pool: {lengths.numel()} lengths for {B} clips")
    Ho, Wo = H // 2, W // 2
    y = _empty((B * T, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, 64), x_bthw.device)
    ws = _empty((int(lib().dlip_stem3d_pool_workspace_bytes(B, T, H, W)) // 4,), x_bthw.device)   # the clip as (hi, lo) pairs
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin("stem3d_pool_f16x3_kernel", 2.0 * B * T * Ho * Wo * 64 * 245)
    call("dlip_stem3d_pool_f16x3", x_bthw, lengths, ws, w_img, w_scale, bias, slope, y, B, T, H, W, 64)
    if hook is not None:
        hook.end(tok)
    return y


def shuffle_stem24(x_bthw: Tensor, w_248x32: Tensor, bias: Tensor, slope: Optional[Tensor]) -> Tensor:
    """x [B,T,H,W] -> [(B*T), H/2, W/2, 24]: the ShuffleNet lip-clip stem, Conv3d(1->24, 5x7x7) + folded BN + PReLU/ReLU in exact
    fp32 (dlip_shuffle_stem24_f32; weights of deeplip_amd.shufflenet.pack_stem24)."""
    for t, n in ((x_bthw, "x"), (w_248x32, "w"), (bias, "bias"), (slope, "slope")):
        _req(t, n)
    B, T, H, W = x_bthw.shape
    if tuple(w_248x32.shape) != (248, 32) or bias.numel() != 24 or (slope is not None and slope.numel() != 24):
        raise ValueError("shuffle_stem24: weights [248, 32], bias and slope [24]")
    y = _empty((B * T, H // 2, W // 2, 24), x_bthw.device)
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin("shuffle_stem24_f32_kernel", 2.0 * B * T * (H // 2) * (W // 2) * 24 * 245)
    call("dlip_shuffle_stem24_f32", x_bthw, w_248x32, bias, slope, y, B, T, H, W)
    if hook is not None:
        hook.end(tok)
    return y


def shuffle_dwpw(x: Tensor, w: Tensor, bias: Tensor, *, dw_w: Optional[Tensor] = None, dw_b: Optional[Tensor] = None,
                 stride: int = 1, in_channels: Optional[int] = None, in_channel_offset: int = 0, out: Optional[Tensor] = None,
                 hp: int = 0, par: int = 0, passthrough: Optional[Tensor] = None) -> Tensor:
    """ReLU(w^T A + bias) per pixel (dlip_shuffle_dwpw_f32), A = the channel slice [in_channel_offset : +in_channels] of x
    [N,H,W,Cx] (NHWC) or, with ``dw_w`` [9, Cin] / ``dw_b`` [Cin], its depthwise 3x3 (pad 1, ``stride``) computed on load.
    ``w`` [Cp, Kp] k-major (Cp = Cin rounded up to 32, Kp a multiple of 64), ``bias`` [K].

    ``hp`` = 0: y [N,Ho,Wo,K] (or channels [0, K) of ``out``).  ``hp`` > 0: output channel j lands at logical channel 2j + ``par``
    of a 2K-channel InvertedResidual output stored as two halves padded to ``hp`` channels (``out`` [N,Ho,Wo,>= 2hp]:
    deeplip_amd.shufflenet.phys_map); ``par`` = 1 also zeroes the padding channels.  ``passthrough`` [N,H,W,*] (stride 1):
    its channels [0, K) -- a unit's x1 -- go to the other parity in the same launch."""
    for t, n in ((x, "x"), (w, "w"), (bias, "bias"), (dw_w, "dw_w"), (dw_b, "dw_b"), (out, "out"), (passthrough, "passthrough")):
        _req(t, n)
    N, H, W, Cx = x.shape
    Cin = Cx - in_channel_offset if in_channels is None else in_channels
    K = bias.numel()
    Cp, Kp = w.shape
    if in_channel_offset + Cin > Cx or Cin % 4 or Cx % 4 or in_channel_offset % 4:
        raise ValueError(f"shuffle_dwpw: input slice [{in_channel_offset}:+{Cin}] of {Cx} channels (multiples of 4)")
    if Cp != (Cin + 31) // 32 * 32 or Kp % 64 or Kp < K:
        raise ValueError(f"shuffle_dwpw: weights {tuple(w.shape)} for Cin={Cin}, K={K}")
    if (dw_w is None) != (dw_b is None) or (dw_w is not None and (tuple(dw_w.shape) != (9, Cin) or dw_b.numel() != Cin)):
        raise ValueError("shuffle_dwpw: depthwise weights [9, Cin] and bias [Cin] go together")
    if stride not in (1, 2) or (stride == 2 and dw_w is None):
        raise ValueError("shuffle_dwpw: stride 2 needs the depthwise stage")
    Ho, Wo = (H, W) if stride == 1 else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    Ky = 2 * hp if hp else K
    if out is None:
        out = _empty((N, Ho, Wo, Ky), x.device)
    if tuple(out.shape[:3]) != (N, Ho, Wo) or out.shape[3] < Ky or (hp and hp < K):
        raise ValueError(f"shuffle_dwpw: output {tuple(out.shape)} for {(N, Ho, Wo, Ky)} (hp={hp}, K={K})")
    ldp = 0
    if passthrough is not None:
        if not hp or stride != 1 or tuple(passthrough.shape[:3]) != (N, H, W) or passthrough.shape[3] < K:
            raise ValueError("shuffle_dwpw: passthrough needs a shuffled stride-1 output and >= K channels per pixel")
        ldp = passthrough.shape[3]
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin("shuffle_dwpw_f32_kernel", 2.0 * N * Ho * Wo * K * Cin + (18.0 * N * Ho * Wo * Cin if dw_w is not None else 0.0))
    call("dlip_shuffle_dwpw_f32", x.data_ptr() + 4 * in_channel_offset, dw_w, dw_b, w, bias, passthrough, out, N, H, W, stride, Cin, K, Kp, Cx, ldp,
         out.shape[3], hp, par)
    if hook is not None:
        hook.end(tok)
    return out


def _dw_geometry(what: str, x_shape, ws, k_list, pads, t_outs, d: int):
    B, T, Cc = x_shape
    if Cc % 4:
        raise ValueError(f"{what}: C = {Cc} must be a multiple of 4")
    if not 1 <= len(ws) <= 4 or not (len(ws) == len(k_list) == len(pads) == len(t_outs)):
        raise ValueError(f"{what}: 1..4 branches with one weight, k, pad and output length each")
    if d < 1:
        raise ValueError(f"{what}: dilation {d} < 1")
    for w, k, P, To in zip(ws, k_list, pads, t_outs):
        if tuple(w.shape) != (k, Cc):
            raise ValueError(f"{what}: depthwise weights {tuple(w.shape)}, expected tap-major [k={k}, C={Cc}]")
        if k < 1 or k > 64 or P < 0 or To < 1:
            raise ValueError(f"{what}: k = {k}, pad = {P}, output length {To}")


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


def tcn_dw(x: Tensor, ws: Sequence[Tensor], d: int, *, pads: Sequence[int], t_outs: Sequence[int],
           biases: Optional[Sequence[Tensor]] = None, slopes: Optional[Sequence[Tensor]] = None) -> list:
    """Depthwise dilated temporal convolution (dlip_tcn_dw_fwd_f32), one launch for every branch: x [B,T,C] channels-last,
    ws[r] [k_r, C] tap-major -> [act(z_r + bias_r)] with z_r[b,t,c] = sum_j ws[r][j,c] x[b, t - pads[r] + j d, c], t < t_outs[r].
    Eval: pads = (k-1)d/2, t_outs = T, folded BatchNorm in ws / biases, slopes = PReLU weights or zeros (ReLU).  Train: pads =
    (k-1)d, t_outs = T + (k-1)d, no bias or slope (raw z)."""
    _req(x, "x")
    ks = [int(w.shape[0]) for w in ws]
    for i, w in enumerate(ws):
        _req(w, f"ws[{i}]")
    for grp, n in ((biases, "biases"), (slopes, "slopes")):
        if grp is not None:
            if len(grp) != len(ws):
                raise ValueError(f"tcn_dw: {len(grp)} {n} for {len(ws)} branches")
            for t in grp:
                _req(t, n)
                if t.numel() != x.shape[2]:
                    raise ValueError(f"tcn_dw: {n} entries must have C = {x.shape[2]} elements")
    _dw_geometry("tcn_dw", x.shape, ws, ks, pads, t_outs, d)
    B, T, Cc = x.shape
    ys = [_empty((B, int(To), Cc), x.device) for To in t_outs]
    n = len(ws)
    call("dlip_tcn_dw_fwd_f32", x, n, _arr(C.c_void_p, [w.data_ptr() for w in ws]),
         _arr(C.c_void_p, [b.data_ptr() for b in biases]) if biases is not None else None,
         _arr(C.c_void_p, [s.data_ptr() for s in slopes]) if slopes is not None else None, _arr(C.c_void_p, [y.data_ptr() for y in ys]),
         _arr(C.c_int32, ks), _arr(C.c_int32, list(pads)), _arr(C.c_int32, list(t_outs)), B, T, Cc, int(d))
    return ys


def tcn_dw_dgrad(dzs: Sequence[Tensor], ws: Sequence[Tensor], d: int, *, pads: Sequence[int], T: int) -> Tensor:
    """The data gradient of tcn_dw over every branch at once: dx [B,T,C] = sum_r sum_j ws[r][j,c] dzs[r][b, s + pads[r] - j d, c]
    (dlip_tcn_dw_dgrad_f32; dzs[r] [B, T_out_r, C])."""
    for i, (g, w) in enumerate(zip(dzs, ws)):
        _req(g, f"dzs[{i}]")
        _req(w, f"ws[{i}]")
    if len(dzs) != len(ws) or not dzs:
        raise ValueError("tcn_dw_dgrad: one gradient per branch weight")
    B, _, Cc = dzs[0].shape
    ks = [int(w.shape[0]) for w in ws]
    t_outs = [int(g.shape[1]) for g in dzs]
    if any(g.dim() != 3 or g.shape[0] != B or g.shape[2] != Cc for g in dzs):
        raise ValueError("tcn_dw_dgrad: gradients [B, T_out, C] with one B and C")
    _dw_geometry("tcn_dw_dgrad", (B, T, Cc), ws, ks, pads, t_outs, d)
    dx = _empty((B, T, Cc), dzs[0].device)
    call("dlip_tcn_dw_dgrad_f32", _arr(C.c_void_p, [g.data_ptr() for g in dzs]), len(dzs), _arr(C.c_void_p, [w.data_ptr() for w in ws]),
         _arr(C.c_int32, ks), _arr(C.c_int32, list(pads)), _arr(C.c_int32, t_outs), dx, B, T, Cc, int(d))
    return dx


def tcn_dw_wgrad(x: Tensor, dzs: Sequence[Tensor], ks: Sequence[int], d: int, *, pads: Sequence[int]) -> list:
    """The weight gradients of tcn_dw: [dw_r [k_r, C]], dw_r[j,c] = sum_{b,t} dzs[r][b,t,c] x[b, t - pads[r] + j d, c]
    (dlip_tcn_dw_wgrad_f32: fp64 chunk sums, then a fixed-order sum of the chunks -- deterministic, two launches)."""
    _req(x, "x")
    for i, g in enumerate(dzs):
        _req(g, f"dzs[{i}]")
    B, T, Cc = x.shape
    t_outs = [int(g.shape[1]) for g in dzs]
    if any(g.dim() != 3 or g.shape[0] != B or g.shape[2] != Cc for g in dzs):
        raise ValueError("tcn_dw_wgrad: gradients [B, T_out, C] matching x [B, T, C]")
    dws = [_empty((int(k), Cc), x.device) for k in ks]
    _dw_geometry("tcn_dw_wgrad", x.shape, dws, list(ks), pads, t_outs, d)
    n_ws = sum(int(lib().dlip_tcn_dw_wgrad_chunks(B * To)) * int(k) * Cc for k, To in zip(ks, t_outs))
    ws = _empty((n_ws,), x.device, torch.float64)
    call("dlip_tcn_dw_wgrad_f32", x, len(dzs), _arr(C.c_void_p, [g.data_ptr() for g in dzs]), _arr(C.c_void_p, [w.data_ptr() for w in dws]),
         _arr(C.c_int32, [int(k) for k in ks]), _arr(C.c_int32, list(pads)), _arr(C.c_int32, t_outs), B, T, Cc, int(d), ws, n_ws)
    return dws


def add_prelu(a: Tensor, b: Tensor, slope: Tensor) -> Tensor:
    """prelu(a + b) with per-channel slopes (dlip_add_prelu_rows_fwd_f32): an identity residual's end of block in eval mode."""
    for t, n in ((a, "a"), (b, "b"), (slope, "slope")):
        _req(t, n)
    if a.shape != b.shape or a.shape[-1] % 4 or slope.numel() != a.shape[-1]:
        raise ValueError(f"add_prelu: a {tuple(a.shape)}, b {tuple(b.shape)}, slope {slope.numel()} (channels a multiple of 4)")
    Cc = a.shape[-1]
    s_ = _empty(a.shape, a.device)
    y = _empty(a.shape, a.device)
    call("dlip_add_prelu_rows_fwd_f32", a, b, slope, s_, y, a.numel() // Cc, Cc)
    return y


def avgpool3(x: Tensor) -> Tensor:
    """AvgPool2d(3) of x [N,H,W,C] -> [N,C]: the mean of the top-left 3x3 window (stride 3, no padding: a 3..5 pixel map gives
    exactly one output pixel, dlip_avgpool3_nhwc_f32).  Other map sizes raise ValueError (the reference cannot view them as
    [-1, C] per frame either)."""
    _req(x, "x")
    N, H, W, Cc = x.shape
    if not (3 <= H <= 5 and 3 <= W <= 5):
        raise ValueError(f"avgpool3: AvgPool2d(3) of a {H}x{W} map does not give one pixel per frame")
    y = _empty((N, Cc), x.device)
    call("dlip_avgpool3_nhwc_f32", x, y, N, H, W, Cc)
    return y


def center_crop_origin(size: int, crop: int) -> int:
    """CenterCrop's offset (models/video_models/preprocess.py:89-90): ``int(round(w - tw) / 2.)`` -- the round() is of the
    integer margin (a no-op), the division's result is truncated: FLOOR of half the margin, as dlip_crop_normalize_u8 does.
    (Round 3 had int(round(margin / 2)), Python's round-half-even: one pixel off for margins of 3, 7, 11 ... -- 91- or
    95-pixel frames.)"""
    return (size - crop) // 2


def draw_clip_params(n_clips: int, Hs: int, Ws: int, crop: int = 88, flip_ratio: float = 0.5, rng=None):
    """One (oy, ox, flip, 0) row per clip as the reference's train pipeline draws them (dataloaders.py:13-17): RandomCrop's
    ``random.randint(0, w - tw)`` then ``randint(0, h - th)`` (preprocess.py:110-111, inclusive bounds), then HorizontalFlip's
    ``random.random() < flip_ratio`` (:134), per clip, from ``rng`` (a ``random.Random``; the module-level generator when None --
    what the reference uses, seeded by the trainer).  Returns an int32 numpy array [n_clips, 4] (host; ``.to(device)`` it)."""
    import random as _random
    import numpy as _np
    r = rng if rng is not None else _random
    out = _np.zeros((n_clips, 4), dtype=_np.int32)
    for i in range(n_clips):
        ox = r.randint(0, Ws - crop)
        oy = r.randint(0, Hs - crop)
        out[i, 0], out[i, 1], out[i, 2] = oy, ox, int(r.random() < flip_ratio)
    return out


def stem3d_pool_u8(frames: Tensor, w_img: Tensor, bias: Tensor, slope: Optional[Tensor], w_scale: Tensor, crop: int = 88,
                   lengths: Optional[Tensor] = None, clip_params: Optional[Tensor] = None) -> Tensor:
    """uint8 frames [B,T,Hs,Ws] (gray) or [B,T,3,Hs,Ws] (RGB) -> [(B*T), Hp, Wp, 64] split format: centre crop + gray +
    (x/255 - 0.421)/0.165 inside the stem's pre-pass (dlip_stem3d_pool_u8_f16x3) -- no fp32 clip in HBM or over PCIe.
    ``lengths`` (int32 CUDA [B]): ragged batch, frames t >= lengths[b] become zeros of the normalised clip.  ``clip_params``
    (int32 CUDA [B,4] = (oy, ox, flip, 0) per clip): the train pipeline's RandomCrop + HorizontalFlip (preprocess.py:95-138)
    instead of the centre crop -- see draw_clip_params."""
    _req(frames, "frames", torch.uint8)
    for t, n in ((w_img, "w"), (bias, "bias"), (slope, "slope"), (w_scale, "w_scale")):
        _req(t, n)
    _req(lengths, "lengths", torch.int32)
    _req(clip_params, "clip_params", torch.int32)
    if lengths is not None and lengths.numel() != frames.shape[0]:
        raise ValueError(f"stem3d_pool_u8: {lengths.numel()} lengths for {frames.shape[0]} clips")
    if clip_params is not None and tuple(clip_params.shape) != (frames.shape[0], 4):
        raise ValueError(f"stem3d_pool_u8: clip_params must be [B,4] = (oy, ox, flip, 0), got {tuple(clip_params.shape)}")
    if frames.dim() not in (4, 5) or (frames.dim() == 5 and frames.shape[2] != 3):
        raise ValueError("stem3d_pool_u8: expected uint8 [B,T,H,W] or [B,T,3,H,W]")
    ch = 3 if frames.dim() == 5 else 1
    B, T = frames.shape[0], frames.shape[1]
    Hs, Ws = frames.shape[-2], frames.shape[-1]
    H = W = crop
    if Hs < H or Ws < W:
        raise ValueError(f"stem3d_pool_u8: frames {Hs}x{Ws} are smaller than the {crop}x{crop} crop")
    oy, ox = center_crop_origin(Hs, H), center_crop_origin(Ws, W)
    Ho, Wo = H // 2, W // 2
    y = _empty((B * T, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, 64), frames.device)
    ws = _empty((int(lib().dlip_stem3d_pool_workspace_bytes(B, T, H, W)) // 4,), frames.device)
    hook = LAUNCH_HOOK
    if hook is not None:
        tok = hook.begin("stem3d_pool_f16x3_kernel", 2.0 * B * T * Ho * Wo * 64 * 245)
    call("dlip_stem3d_pool_u8_f16x3", frames, ch, Hs, Ws, oy, ox, clip_params, lengths, ws, w_img, w_scale, bias, slope, y, B, T, H, W, 64)
    if hook is not None:
        hook.end(tok)
    return y


def split_pack(x: Tensor) -> Tensor:
    """fp32 [..., C] -> split activation format (same shape / dtype container; C % 32 == 0)."""
    _req(x, "x")
    y = _empty(x.shape, x.device)
    Cc = x.shape[-1]
    call("dlip_split_pack_f32", x, y, x.numel() // Cc, Cc)
    return y


def split_pack_scaled(x: Tensor, scale: Tensor) -> Tensor:
    """split_pack(x * scale[0]) -- ``scale``: a device scalar holding a power of two (the activation exponent of a model input whose
    gain lies outside the split format, packing.act_exponents; the multiplication is exact)."""
    _req(x, "x"); _req(scale, "scale")
    y = _empty(x.shape, x.device)
    Cc = x.shape[-1]
    call("dlip_split_pack_scaled_f32", x, y, scale, x.numel() // Cc, Cc)
    return y


def channel_scale(x: Tensor, scale_vec: Tensor, zero_vec: Tensor) -> Tensor:
    """y[..., c] = x[..., c] * scale_vec[c] (dlip_affine_act_f32 with a unit slope): how an fp32 output leaves a model whose last
    split tensor carries an activation exponent -- scale_vec = 2^-e, exact."""
    C_ = x.shape[-1]
    return affine_act(x.reshape(-1, C_), scale_vec, zero_vec, slope=1.0).view(x.shape)


def split_unpack(x: Tensor) -> Tensor:
    """Inverse of split_pack (hi + lo in fp32)."""
    _req(x, "x")
    y = _empty(x.shape, x.device)
    Cc = x.shape[-1]
    call("dlip_split_unpack_f32", x, y, x.numel() // Cc, Cc)
    return y


def maxpool3x3s2(x: Tensor, out_split: bool = False) -> Tensor:
    _req(x, "x")
    N, H, W, Cc = x.shape
    y = _empty((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), x.device)
    call("dlip_maxpool3x3s2_nhwc_f32", x, y, N, H, W, Cc, int(out_split))
    return y


def avgpool(x: Tensor) -> Tensor:
    _req(x, "x")
    N, H, W, Cc = x.shape
    y = _empty((N, Cc), x.device)
    call("dlip_avgpool_nhwc_f32", x, y, N, H * W, Cc)
    return y


def time_mean(x: Tensor, lengths: Optional[Tensor] = None, len_add: int = 0) -> Tensor:
    """x [B,T,C] -> [B,C]; ``lengths`` int32 [B] masks the mean to t < len + len_add (model.py:16-17)."""
    _req(x, "x")
    _req(lengths, "lengths", torch.int32)
    B, T, Cc = x.shape
    y = _empty((B, Cc), x.device)
    call("dlip_time_mean_f32", x, lengths, len_add, y, B, T, Cc, Cc)
    return y


def mask_frames(x: Tensor, lengths: Tensor) -> Tensor:
    """x [B,T,E] -> same with frames t >= lengths[b] zeroed (the padding of a ragged batch; dlip_mask_frames_f32)."""
    _req(x, "x")
    _req(lengths, "lengths", torch.int32)
    B, T, E = x.shape
    if lengths.numel() != B or E % 4:
        raise ValueError("mask_frames: one length per row of x [B,T,E], E % 4 == 0")
    y = _empty(x.shape, x.device)
    call("dlip_mask_frames_f32", x, lengths, y, B, T, E)
    return y


def _time_ragged_args(x: Tensor, lengths: Tensor, shift: int, name: str):
    _req(x, "x")
    _req(lengths, "lengths", torch.int32)
    if lengths is None or x.dim() != 4 or lengths.numel() != x.shape[0] or x.shape[3] % 4 or not 0 <= int(shift) <= 16:
        raise ValueError(f"{name}: x [N,H,W,C] with C % 4 == 0, one int32 length per image, 0 <= shift <= 16")
    return x.shape


def time_tail_zero(x: Tensor, lengths: Tensor, shift: int = 0) -> Tensor:
    """x [N,H,W,C] (W = time; fp32 or the split activation format), IN PLACE: frames w >= ((clamp(lengths[n], 1, W << shift) - 1) >> shift)
    + 1 of image n become zeros -- the padding of a ragged batch behind ``shift`` stride-2 stages (dlip_time_tail_zero_f32: store-only,
    the lengths stay on the device).  Returns x."""
    N, H, W, Cc = _time_ragged_args(x, lengths, shift, "time_tail_zero")
    call("dlip_time_tail_zero_f32", x, lengths, int(shift), N, H, W, Cc)
    return x


def avgpool_time_ragged(x: Tensor, lengths: Tensor, shift: int = 0) -> Tensor:
    """x [N,H,W,C] fp32 -> [N,C]: the mean over every h and the valid frames w < Lk of image n (Lk as time_tail_zero): AdaptiveAvgPool2d(1)
    of each utterance at its own length (dlip_avgpool_time_ragged_f32)."""
    N, H, W, Cc = _time_ragged_args(x, lengths, shift, "avgpool_time_ragged")
    y = _empty((N, Cc), x.device)
    call("dlip_avgpool_time_ragged_f32", x, lengths, int(shift), y, N, H, W, Cc)
    return y


def statpool_nhwc(x: Tensor, lengths: Optional[Tensor] = None, shift: int = 0, eps: float = 1e-5) -> Tensor:
    """x [N,H,W,C] fp32 (W = time) -> [N, 2 H C] = cat(mean, sqrt(unbiased variance + eps)) over the valid frames w < Wb of image n, per
    feature j = h C + c (dlip_statpool_nhwc_f32).  ``lengths`` (int32 CUDA [N], input frames) / ``shift``: Wb as time_tail_zero; None:
    Wb = W, which must be >= 2."""
    _req(x, "x")
    _req(lengths, "lengths", torch.int32)
    if x.dim() != 4 or x.shape[3] % 4 or not 0 <= int(shift) <= 16 or (lengths is not None and lengths.numel() != x.shape[0]):
        raise ValueError("statpool_nhwc: x [N,H,W,C] with C % 4 == 0, one int32 length per image or none, 0 <= shift <= 16")
    N, H, W, Cc = x.shape
    if W < 2:
        raise ValueError(f"statpool_nhwc: the unbiased standard deviation needs >= 2 frames, the map has {W}")
    y = _empty((N, 2 * H * Cc), x.device)
    call("dlip_statpool_nhwc_f32", x, lengths, int(shift), float(eps), y, N, H, W, Cc)
    return y


def swap_axes_nhwc(x: Tensor) -> Tensor:
    """x [N,A,B,C] -> [N,B,A,C] (dlip_swap_axes_nhwc_f32): [N,H,W,C] -> [N,W,H,C], each frame's H C features contiguous, and back."""
    _req(x, "x")
    if x.dim() != 4 or x.shape[3] % 4:
        raise ValueError("swap_axes_nhwc: x [N,A,B,C] with C % 4 == 0")
    N, A, B, Cc = x.shape
    y = _empty((N, B, A, Cc), x.device)
    call("dlip_swap_axes_nhwc_f32", x, y, N, A, B, Cc)
    return y


def time_valid_lengths(lengths: Tensor, shift: int, W: int) -> Tensor:
    """int32 CUDA [N] input lengths -> the valid frames ((clamp(L, 1, W << shift) - 1) >> shift) + 1 on a W-frame axis behind ``shift``
    stride-2 stages, formed on the device (dlip_time_valid_lengths_i32)."""
    _req(lengths, "lengths", torch.int32)
    if lengths is None or not 0 <= int(shift) <= 16 or W < 1:
        raise ValueError("time_valid_lengths: int32 lengths, 0 <= shift <= 16, W >= 1")
    out = _empty((lengths.numel(),), lengths.device, torch.int32)
    call("dlip_time_valid_lengths_i32", lengths, int(shift), int(W), out, lengths.numel())
    return out


# ---- attentive statistics pooling, one head or several (csrc/mh_attn_pool_ops.hip, ABI 64 / 67):
# ---- deeplip_amd.audio.AttentiveStatPooling (n = 1) and deeplip_amd.audio.MultiHeadAttention
MH_MAX_HEADS = 8
MH_LDS_BYTES = 160 * 1024        # 3 n C floats of the backward's first pass


def mh_attn_check(n: int, T: int, C: int) -> None:
    """The limits of the dlip_mh_attn_* entry points as a ValueError that names them (the library answers DLIP_EINVAL)."""
    if not 1 <= n <= MH_MAX_HEADS:
        raise ValueError(f"attentive pooling: 1 <= heads <= {MH_MAX_HEADS}, got {n}")
    if T > 16000:
        raise ValueError(f"attentive pooling: at most 16000 frames, got {T}")
    if C % 4 or 12 * n * C > MH_LDS_BYTES:
        raise ValueError(f"attentive pooling: C % 4 == 0 and 12 heads C <= {MH_LDS_BYTES} bytes of LDS, got heads {n}, C {C}")


def mh_attn_scores(hidden: Tensor, v: Tensor, k: Tensor, head_off: Optional[Tensor], lengths: Optional[Tensor] = None,
                   len_add: int = 0) -> Tensor:
    """hidden [B,T,S] (= x W^T + b of all heads), v [S], k [n], head_off int32 CUDA [n+1] (prefix sums of the head widths; None for one
    head, which owns every column) -> alpha [B,n,T]: per head the softmax over the first lengths[b] + len_add frames of
    relu(hidden[..., head]) v[head] + k[h]; zeros behind (dlip_mh_attn_scores_f32)."""
    for t, nm in ((hidden, "hidden"), (v, "v"), (k, "k")):
        _req(t, nm)
    _req(head_off, "head_off", torch.int32)
    _req(lengths, "lengths", torch.int32)
    B, T, S = hidden.shape
    n = k.numel()
    if ((head_off is None and n != 1) or (head_off is not None and head_off.numel() != n + 1) or v.numel() != S
            or (lengths is not None and lengths.numel() != B)):
        raise ValueError("mh_attn_scores: hidden [B,T,S], v [S], k [n], head_off [n+1] (or None with n = 1), one length per utterance or none")
    alpha = _empty((B, n, T), hidden.device)
    call("dlip_mh_attn_scores_f32", hidden, v, k, head_off, lengths, int(len_add), alpha, B, T, S, n)
    return alpha


def mh_attn_stat_pool(x: Tensor, alpha: Tensor, eps: float, lengths: Optional[Tensor] = None, len_add: int = 0) -> Tensor:
    """x [B,T,C], alpha [B,n,T] -> [B, n 2C] = cat over heads of (sum alpha x | sqrt(max(sum alpha x^2 - mean^2, 0) + eps)), x read once
    for all heads (dlip_mh_attn_stat_pool_f32).  eps = 0: the reference's unfloored sqrt(sum alpha x^2 - mean^2) (pooling.py:106)."""
    _req(x, "x")
    _req(alpha, "alpha")
    _req(lengths, "lengths", torch.int32)
    B, T, Cc = x.shape
    if alpha.dim() != 3 or alpha.shape[0] != B or alpha.shape[2] != T or (lengths is not None and lengths.numel() != B):
        raise ValueError("mh_attn_stat_pool: x [B,T,C], alpha [B,n,T], one length per utterance or none")
    n = alpha.shape[1]
    y = _empty((B, n * 2 * Cc), x.device)
    call("dlip_mh_attn_stat_pool_f32", x, alpha, lengths, int(len_add), float(eps), y, B, T, Cc, n)
    return y


def l1_sum(w: Tensor) -> Tensor:
    """sum |w| as a 0-d device tensor (dlip_l1_sum_f32: fp64 accumulation, fixed order)."""
    _req(w, "w")
    out = torch.empty((1,), device=w.device, dtype=torch.float32)
    call("dlip_l1_sum_f32", w.contiguous(), out, w.numel())
    return out[0]


def group_mean(x: Tensor, group_ptr: Tensor) -> Tensor:
    _req(x, "x")
    _req(group_ptr, "group_ptr", torch.int32)
    U = group_ptr.numel() - 1
    y = _empty((U, x.shape[1]), x.device)
    call("dlip_group_mean_f32", x, group_ptr, y, U, x.shape[1])
    return y


def meanstd_pool(x: Tensor, out_split: bool = False, lengths: Optional[Tensor] = None, len_add: int = 0) -> Tensor:
    """x [B,T,C] -> [B,2C] = cat(mean_t, unbiased std_t)  (pooling.py:24-26).  ``out_split``: the
    result is [B, 2C rounded up to 32] in the split activation format (zero padded).  ``lengths`` (int32 CUDA [B]): ragged
    batch, utterance b's statistics cover its first lengths[b] + len_add frames."""
    _req(x, "x")
    _req(lengths, "lengths", torch.int32)
    B, T, Cc = x.shape
    if lengths is not None and lengths.numel() != B:
        raise ValueError(f"meanstd_pool: {lengths.numel()} lengths for {B} utterances")
    if Cc % 4:
        raise ValueError("meanstd_pool: C must be a multiple of 4")
    width = (2 * Cc + 31) // 32 * 32 if out_split else 2 * Cc
    y = _empty((B, width), x.device)
    call("dlip_meanstd_pool_f32", x, lengths, len_add, y, B, T, Cc, int(out_split))
    return y


def nct_to_ntc(x: Tensor, pad_to: Optional[int] = None, out_split: bool = False) -> Tensor:
    """[B,C,T] -> [B,T,Cp] channels-last, zero-padded to Cp; ``out_split``: in the split activation format (Cp % 32 == 0)."""
    _req(x, "x")
    B, Cc, T = x.shape
    Cp = Cc if pad_to is None else pad_to
    y = _empty((B, T, Cp), x.device)
    if out_split:
        call("dlip_nct_to_ntc_split_f32", x, y, B, Cc, T, Cp)
        return y
    call("dlip_nct_to_ntc_f32", x, y, B, Cc, T, Cp)
    return y


def ntc_to_nct(x: Tensor) -> Tensor:
    _req(x, "x")
    B, T, Cc = x.shape
    y = _empty((B, Cc, T), x.device)
    call("dlip_ntc_to_nct_f32", x, y, B, T, Cc)
    return y


def ingest_rgb_u8(frames: Tensor) -> Tensor:
    """[B,T,3,H,W] uint8 -> [B,1,T,H,W] float32 normalised gray."""
    _req(frames, "frames", torch.uint8)
    B, T, three, H, W = frames.shape
    if three != 3:
        raise ValueError("ingest_rgb_u8: expected [B,T,3,H,W]")
    y = _empty((B, 1, T, H, W), frames.device)
    call("dlip_ingest_rgb_u8", frames, y, B * T, H, W)
    return y


def affine_act(x: Tensor, scale: Tensor, shift: Tensor, slope: float = 0.2, act_first: bool = False) -> Tensor:
    """[M,C]: lrelu(x*scale+shift) or lrelu(x)*scale+shift (eval BatchNorm1d + LeakyReLU)."""
    _req(x, "x"); _req(scale, "scale"); _req(shift, "shift")
    y = _empty(x.shape, x.device)
    call("dlip_affine_act_f32", x, scale, shift, y, x.numel() // x.shape[-1], x.shape[-1], slope, int(act_first))
    return y


def znorm_cat(a: Optional[Tensor], v: Optional[Tensor], biased: bool = False) -> Tensor:
    _req(a, "a"); _req(v, "v")
    U = (a if a is not None else v).shape[0]
    Da = a.shape[1] if a is not None else 0
    Dv = v.shape[1] if v is not None else 0
    y = _empty((U, Da + Dv), (a if a is not None else v).device)
    call("dlip_znorm_cat_f32", a, Da, v, Dv, y, U, int(biased))
    return y


def znorm_cat_pooled(a: Optional[Tensor], p: "Pooled", biased: bool = False) -> Tensor:
    """znorm_cat(a, pool_finish(p, 'mean')) in one launch (bit-identical to the two)."""
    _req(a, "a")
    U = (p.M + p.group_rows - 1) // p.group_rows
    Da = a.shape[1] if a is not None else 0
    if a is not None and a.shape[0] != U:
        raise ValueError(f"znorm_cat_pooled: {a.shape[0]} rows of a, {U} pooled groups")
    y = _empty((U, Da + p.K), p.partials.device)
    call("dlip_znorm_cat_pooled_f32", a, Da, p.partials, p.M, p.K, p.tile_rows, p.group_rows, p.lengths, p.len_mul, p.len_add, y, U, int(biased))
    return y


def l2_normalize(x: Tensor, eps: float = 1e-12) -> Tensor:
    _req(x, "x")
    y = _empty(x.shape, x.device)
    call("dlip_l2_normalize_f32", x, y, x.shape[0], x.shape[1], eps)
    return y


def pair_cosine(emb: Tensor, idx_a: Tensor, idx_b: Tensor, mode: int = 0, eps: float = 1e-8,
                weight: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    _req(emb, "emb"); _req(idx_a, "idx_a", torch.int32); _req(idx_b, "idx_b", torch.int32)
    n = idx_a.numel()
    acc = out is not None
    if out is None:
        out = _empty((n,), emb.device)
    _req(out, "out")
    call("dlip_pair_cosine_f32", emb, emb.shape[0], emb.shape[1], idx_a, idx_b, out, n, mode, eps, weight, int(acc))
    return out


# ---- cohort score normalisation (csrc/score_norm_ops.hip, ABI 58) ----
TOPK_MAX_N = 32768                      # a row of the score matrix lives in LDS (dlip_topk_stats_f32)
SCORE_NORM_MODES = {"z": 0, "t": 1, "s": 2}
_COHORT_SCRATCH_BYTES = 256 << 20       # cohort_stats: the score-matrix chunk stays at or below this


def topk_stats(s: Tensor, k: int, n: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """s [R, ld] -> (mean [R], sd [R]): mean and population deviation (divisor k) of the k largest of each row's first ``n``
    values (default: all ld of them; columns [n, ld) are never read).  Exact selection, ties at the k-th value counted exactly,
    fp64 statistics rounded to fp32 once.  1 <= k <= n <= 32768."""
    if s.dim() != 2:
        raise ValueError("topk_stats: s must be [R, ld]")
    R, ld = s.shape
    n = ld if n is None else int(n)
    if not 1 <= n <= ld:
        raise ValueError(f"topk_stats: n={n} outside [1, {ld}]")
    if n > TOPK_MAX_N:
        raise ValueError(f"topk_stats: rows of {n} values exceed the kernel's {TOPK_MAX_N}")
    if not 1 <= int(k) <= n:
        raise ValueError(f"topk_stats: k={k} outside [1, {n}]")
    if R < 1:
        raise ValueError("topk_stats: no rows")
    _req(s, "s")                          # behind the shape checks: those are refused the same way on a box without a GPU
    mean, sd = _empty((R,), s.device), _empty((R,), s.device)
    call("dlip_topk_stats_f32", s, R, n, ld, int(k), mean, sd)
    return mean, sd


def score_norm(scores: Tensor, idx_a: Tensor, idx_b: Tensor, mu: Tensor, sd: Tensor, mode: str = "s", eps: float = 1e-6,
               weight: float = 1.0, out: Optional[Tensor] = None) -> Tensor:
    """weight * z(scores[i]) with za = (s - mu[idx_a[i]]) / max(sd[idx_a[i]], eps), zb likewise through idx_b; mode "z" -> za,
    "t" -> zb, "s" -> (za + zb) / 2.  With ``out`` the result is ADDED to it (pair_cosine's convention: the halves of a score
    fusion are normalised separately and summed)."""
    _req(scores, "scores"); _req(idx_a, "idx_a", torch.int32); _req(idx_b, "idx_b", torch.int32); _req(mu, "mu"); _req(sd, "sd")
    if mode not in SCORE_NORM_MODES:
        raise ValueError(f"score_norm: mode {mode!r} is none of {sorted(SCORE_NORM_MODES)}")
    n = scores.numel()
    if idx_a.numel() != n or idx_b.numel() != n:
        raise ValueError(f"score_norm: {n} scores, {idx_a.numel()} / {idx_b.numel()} indices")
    if mu.numel() != sd.numel() or mu.numel() < 1 or n < 1:
        raise ValueError(f"score_norm: mu has {mu.numel()} entries, sd {sd.numel()}, {n} scores")
    acc = out is not None
    if out is None:
        out = _empty((n,), scores.device)
    _req(out, "out")
    if out.numel() != n:
        raise ValueError(f"score_norm: out has {out.numel()} entries for {n} scores")
    call("dlip_score_norm_f32", scores, idx_a, idx_b, n, mu, sd, mu.numel(), SCORE_NORM_MODES[mode], eps, weight, int(acc), out)
    return out


def cohort_chunk_rows(n_rows: int, n_cohort: int, chunk_rows: Optional[int] = None) -> int:
    """Rows of the embedding table per chunk of cohort_stats: the caller's, else as many as keep the fp32 score-matrix chunk
    [rows, n_cohort] at or below 256 MiB."""
    if chunk_rows is None:
        chunk_rows = max(1, _COHORT_SCRATCH_BYTES // (4 * n_cohort))
    if int(chunk_rows) < 1:
        raise ValueError(f"cohort_stats: chunk_rows={chunk_rows}")
    return min(int(chunk_rows), n_rows)


def cohort_stats(emb: Tensor, cohort: Tensor, top_k: Optional[int] = None, chunk_rows: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """emb [U, D], cohort [Nc, D] -> (mu [U], sd [U]): per row of ``emb`` the mean and population deviation of its ``top_k``
    largest cosine scores against the cohort (None: all Nc).  Both tables are L2-normalised (eps 1e-12, as all_pairs_cosine does);
    ``emb`` is then walked in row chunks, each one exact-fp32 GEMM into a scratch block followed by one topk_stats launch.  The
    scratch comes from ``_empty`` (a StepPlan's arena while one records) and nothing here synchronises or reads the device."""
    if emb.dim() != 2 or cohort.dim() != 2:
        raise ValueError("cohort_stats: emb must be [U, D] and cohort [Nc, D]")
    (U, D), (Nc, Dc) = emb.shape, cohort.shape
    if D != Dc:
        raise ValueError(f"cohort_stats: embeddings have D={D}, the cohort D={Dc}")
    if D % 4:
        raise ValueError("cohort_stats: embedding dimension must be a multiple of 4")
    if U < 1 or Nc < 1:
        raise ValueError(f"cohort_stats: {U} embeddings, {Nc} cohort rows")
    if Nc > TOPK_MAX_N:
        raise ValueError(f"cohort_stats: a cohort of {Nc} exceeds the selection kernel's {TOPK_MAX_N} (DESIGN.md 3f)")
    k = Nc if top_k is None else int(top_k)
    if not 1 <= k <= Nc:
        raise ValueError(f"cohort_stats: top_k={top_k} outside [1, {Nc}]")
    rows = cohort_chunk_rows(U, Nc, chunk_rows)
    _req(emb, "emb"); _req(cohort, "cohort")      # behind the shape checks (as topk_stats)
    e, c = l2_normalize(emb), l2_normalize(cohort)
    mu, sd = _empty((U,), emb.device), _empty((U,), emb.device)
    scratch = _empty((rows, Nc), emb.device)
    for r0 in range(0, U, rows):
        r = min(rows, U - r0)
        linear(e[r0:r0 + r], c, out=scratch[:r].view(1, 1, r, Nc))
        call("dlip_topk_stats_f32", scratch, r, Nc, Nc, k, mu.data_ptr() + 4 * r0, sd.data_ptr() + 4 * r0)
    return mu, sd


def logits_argmax(e: Tensor, W: Tensor, bias: Optional[Tensor] = None, cosine: bool = False) -> Tuple[Tensor, Tensor]:
    _req(e, "e"); _req(W, "W"); _req(bias, "bias")
    B, D = e.shape
    K = W.shape[0]
    logits = _empty((B, K), e.device)
    amax = _empty((B,), e.device, torch.int64)
    call("dlip_logits_argmax_f32", e, W, bias, logits, amax, B, D, K, int(cosine))
    return logits, amax


def margin_ce_loss(logits: Tensor, labels: Tensor, scale: float = 1.0, margin: float = 0.0) -> Tensor:
    _req(logits, "logits"); _req(labels, "labels", torch.int64)
    loss = _empty((1,), logits.device)
    call("dlip_margin_ce_loss_f32", logits, labels, loss, logits.shape[0], logits.shape[1], scale, margin)
    return loss[0]


def row_norm(x: Tensor, eps: float = 1e-12) -> Tensor:
    """r [U] = max(|x_u|, eps): the norm ``l2_normalize`` divides by, the same bits."""
    _req(x, "x")
    r = _empty((x.shape[0],), x.device)
    call("dlip_row_norm_f32", x, r, x.shape[0], x.shape[1], eps)
    return r


def asoftmax_logits(logits: Tensor, r: Tensor, labels: Tensor, lam: Tensor, m: int, r_floor: float = 1e-12) -> Tensor:
    """The A-Softmax logits z [B,K] from cosine logits, the rows' norms, int64 labels and the 1-element device buffer ``lam``
    (dlip_asoftmax_logits_f32, forward mode)."""
    _req(logits, "logits"); _req(r, "r"); _req(labels, "labels", torch.int64); _req(lam, "lam")
    z = _empty(logits.shape, logits.device)
    call("dlip_asoftmax_logits_f32", logits, r, labels, lam, None, z, None, logits.shape[0], logits.shape[1], int(m), float(r_floor), 0)
    return z


def lowfer_cat(e1: Tensor, e2: Tensor) -> Tensor:
    _req(e1, "e1"); _req(e2, "e2")
    B, D = e1.shape
    y = _empty((B, 3 * D), e1.device)
    call("dlip_lowfer_cat_f32", e1, e2, y, B, D)
    return y


# ---- low-rank bilinear pooling (csrc/bilinear_ops.hip, ABI 54): the product of deeplip_amd.fusion.BNBilinear ----
def bilinear_check(e1: Tensor, e2: Tensor, U: Tensor, V: Tensor, k: int):
    """The kernels' limits, refused on the host before any launch: fp32 contiguous device tensors, e1 [B,d1], e2 [B,d2] of one
    batch size, U [d1, k o], V [d2, k o], d1 % 4 == 0, d2 % 4 == 0 (16-byte loads along the embeddings).  Returns (B, d1, d2, o)."""
    for t, name in ((e1, "e1"), (e2, "e2"), (U, "U"), (V, "V")):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise _lib.DeepLipHipError(f"{name}: expected a CUDA (ROCm) tensor; deeplip_amd has no CPU path")
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous float32 matrix, got {t.dtype} {tuple(t.shape)}")
    (B, d1), (B2, d2) = e1.shape, e2.shape
    if B != B2:
        raise ValueError(f"bilinear pooling: e1 has {B} rows, e2 {B2}")
    if B < 1 or d1 < 4 or d2 < 4 or d1 % 4 or d2 % 4:
        raise ValueError(f"bilinear pooling: embedding widths ({d1}, {d2}) must be positive multiples of 4 and the batch non-empty")
    k = int(k)
    if k < 1 or U.shape[0] != d1 or V.shape[0] != d2 or U.shape[1] != V.shape[1] or U.shape[1] % k or U.shape[1] == 0:
        raise ValueError(f"bilinear pooling: U {tuple(U.shape)} / V {tuple(V.shape)} do not fit e1 [*,{d1}], e2 [*,{d2}] and k = {k}")
    return B, d1, d2, U.shape[1] // k


def bilinear_pool(e1: Tensor, e2: Tensor, U: Tensor, V: Tensor, k: int, save: bool = False):
    """z [B,o] = mean over k of (e1 U) * (e2 V) in one launch.  ``save``: also returns P = e1 U and Q = e2 V [B, k o]."""
    B, d1, d2, o = bilinear_check(e1, e2, U, V, k)
    z = _empty((B, o), e1.device)
    P = _empty((B, k * o), e1.device) if save else None
    Q = _empty((B, k * o), e1.device) if save else None
    call("dlip_bilinear_pool_f32", e1, e2, U, V, z, P, Q, B, d1, d2, o, int(k))
    return (z, P, Q) if save else z


def bilinear_pool_bwd_w(e1: Tensor, e2: Tensor, P: Tensor, Q: Tensor, dz: Tensor, k: int):
    """(dU [d1, k o], dV [d2, k o]) of bilinear_pool."""
    B, d1 = e1.shape
    d2, o = e2.shape[1], dz.shape[1]
    _req(dz, "dz")
    dU = _empty((d1, k * o), e1.device)
    dV = _empty((d2, k * o), e1.device)
    call("dlip_bilinear_pool_bwd_w_f32", e1, e2, P, Q, dz, dU, dV, B, d1, d2, o, int(k))
    return dU, dV


def bilinear_pool_bwd_x(P: Tensor, Q: Tensor, dz: Tensor, U: Tensor, V: Tensor, k: int, want1: bool = True, want2: bool = True):
    """(de1 [B,d1], de2 [B,d2]) of bilinear_pool; an output that is not wanted is None and not computed."""
    B, o = dz.shape
    d1, d2 = U.shape[0], V.shape[0]
    _req(dz, "dz")
    de1 = _empty((B, d1), dz.device) if want1 else None
    de2 = _empty((B, d2), dz.device) if want2 else None
    if want1 or want2:
        call("dlip_bilinear_pool_bwd_x_f32", P, Q, dz, U, V, de1, de2, B, d1, d2, o, int(k))
    return de1, de2


def bilinear_finish(z: Tensor, scale: Tensor, shift: Tensor, eps: float = 1e-12) -> Tensor:
    """F.normalize(z) * scale + shift on [B,o]: the row norm and the folded eval-mode BatchNorm1d in one launch."""
    _req(z, "z"); _req(scale, "scale"); _req(shift, "shift")
    B, o = z.shape
    out = _empty((B, o), z.device)
    call("dlip_bilinear_finish_f32", z, scale, shift, out, B, o, float(eps))
    return out


# ---- compact bilinear pooling (csrc/compact_bilinear_ops.hip, ABI 55): deeplip_amd.fusion.CompactBilinearPooling ----
CBP_MAX_D = 4096


def compact_bilinear_pack(sketch: Tensor, name: str = "tensor_sketch") -> dict:
    """What the kernels read instead of the dense count sketch [C, D]: h [C] (the column of row i's nonzero) and s [C] (its sign), and
    the same sorted by bin: rowptr [D+1], idx [C] (ascending within a bin), sgn [C] = s[idx].  Built on the sketch's own device at
    pack time.  A sketch that is not exactly one +-1 per row (a loaded checkpoint, say) raises ValueError naming the first such row:
    there is no dense fallback."""
    S = sketch.detach()
    if S.dim() != 2 or S.dtype != torch.float32 or S.shape[0] < 1 or not 1 <= S.shape[1] <= CBP_MAX_D:
        raise ValueError(f"{name}: expected a float32 count sketch [C >= 1, 1 <= D <= {CBP_MAX_D}], got {S.dtype} {tuple(S.shape)}")
    C, D = S.shape
    nz = (S != 0).sum(dim=1)
    h = S.abs().argmax(dim=1)
    s = S.gather(1, h[:, None])[:, 0]
    bad = ((nz != 1) | (s.abs() != 1)).nonzero()
    if bad.numel():
        i = int(bad[0])
        raise ValueError(f"{name}: row {i} holds {int(nz[i])} nonzero(s), largest {float(s[i])}; a count sketch row is a single +1 or -1")
    idx = torch.sort(h, stable=True).indices
    rowptr = torch.zeros(D + 1, dtype=torch.int64, device=S.device)
    rowptr[1:] = torch.cumsum(torch.bincount(h, minlength=D), 0)
    i32 = lambda t: t.to(torch.int32).contiguous()
    return {"h": i32(h), "s": s.contiguous(), "rowptr": i32(rowptr), "idx": i32(idx), "sgn": s[idx].contiguous(), "C": C, "D": D}


def compact_bilinear_check(x1: Tensor, x2: Tensor, p1: dict, p2: dict):
    """The kernels' limits, refused on the host before any launch: fp32 contiguous device tensors [B,C,H,W] (or [B,C]: one position)
    of equal B, H, W, channel counts that are the sketches' and one D in 1 .. 4096.  Returns (B, C1, C2, P, D)."""
    for t, name in ((x1, "x1"), (x2, "x2")):
        if not isinstance(t, Tensor) or not t.is_cuda:
            raise _lib.DeepLipHipError(f"{name}: expected a CUDA (ROCm) tensor; deeplip_amd has no CPU path")
        if t.dtype != torch.float32 or t.dim() not in (2, 4) or not t.is_contiguous():
            raise ValueError(f"{name}: expected a contiguous float32 [B,C,H,W] or [B,C] tensor, got {t.dtype} {tuple(t.shape)}")
    if x1.dim() != x2.dim() or x1.shape[0] != x2.shape[0] or x1.shape[2:] != x2.shape[2:] or x1.numel() == 0 or x2.numel() == 0:
        raise ValueError(f"compact bilinear pooling: x1 {tuple(x1.shape)} and x2 {tuple(x2.shape)} differ in B, H or W (or are empty)")
    if x1.shape[1] != p1["C"] or x2.shape[1] != p2["C"]:
        raise ValueError(f"compact bilinear pooling: {x1.shape[1]} and {x2.shape[1]} channels, the sketches take {p1['C']} and {p2['C']}")
    D = p1["D"]
    if D != p2["D"] or not 1 <= D <= CBP_MAX_D:
        raise ValueError(f"compact bilinear pooling: sketch widths {p1['D']} and {p2['D']} must be one D in 1 .. {CBP_MAX_D}")
    for p in (p1, p2):
        if p["h"].device != x1.device:
            raise ValueError("compact bilinear pooling: the sketch pack lives on another device than the inputs")
    P = x1[0, 0].numel()
    return x1.shape[0], x1.shape[1], x2.shape[1], P, D


def compact_bilinear(x1: Tensor, x2: Tensor, p1: dict, p2: dict, sum_pool: bool = True, save: bool = False):
    """cbp [B,D] (sum over positions) or [B,H,W,D] in one launch.  ``save``: also returns psi1, psi2 [B,P,D] for the backward."""
    B, C1, C2, P, D = compact_bilinear_check(x1, x2, p1, p2)
    out = _empty((B, D) if sum_pool or x1.dim() == 2 else (B,) + tuple(x1.shape[2:]) + (D,), x1.device)
    psi1 = _empty((B, P, D), x1.device) if save else None
    psi2 = _empty((B, P, D), x1.device) if save else None
    call("dlip_compact_bilinear_f32", x1, x2, p1["rowptr"], p1["idx"], p1["sgn"], p2["rowptr"], p2["idx"], p2["sgn"], out, psi1, psi2, B, C1, C2, P,
         D, int(bool(sum_pool)))
    return (out, psi1, psi2) if save else out


def compact_bilinear_bwd(g: Tensor, psi1: Tensor, psi2: Tensor, p1: dict, p2: dict, shape1, shape2, sum_pool: bool = True,
                         want1: bool = True, want2: bool = True):
    """(dx1, dx2) of compact_bilinear in the inputs' own shapes; an output that is not wanted is None, and nothing is launched when
    neither is."""
    if not (want1 or want2):
        return None, None
    _req(g, "g"); _req(psi1, "psi1"); _req(psi2, "psi2")
    B, P, D = psi1.shape
    if g.numel() != (B * D if sum_pool else B * P * D):
        raise ValueError(f"compact bilinear pooling: g {tuple(g.shape)} does not fit B = {B}, P = {P}, D = {D}, sum_pool = {sum_pool}")
    dx1 = _empty(tuple(shape1), g.device) if want1 else None
    dx2 = _empty(tuple(shape2), g.device) if want2 else None
    call("dlip_compact_bilinear_bwd_f32", g, psi1, psi2, p1["h"], p1["s"], p2["h"], p2["s"], dx1, dx2, B, p1["C"], p2["C"], P, D, int(bool(sum_pool)))
    return dx1, dx2


# ---- the factorized TDNN (`arch: ftdnn`, conf/audio_config.yaml:84-92) ----
SEMI_ORTH_MAX_ROWS, SEMI_ORTH_MAX_MATS = _lib.HEADER["DLIP_SEMI_ORTH_MAX_ROWS"], _lib.HEADER["DLIP_SEMI_ORTH_MAX_MATS"]


def _bypass_check(y: Tensor, x: Tensor, shift: int, what: str):
    _req(y, "y"); _req(x, "x")
    if y.dim() != 3 or x.dim() != 3 or x.shape[0] != y.shape[0] or x.shape[2] != y.shape[2]:
        raise ValueError(f"{what}: y [B,T',C] and x [B,T,C] of one batch and width, got {tuple(y.shape)} and {tuple(x.shape)}")
    B, Tp, C_ = y.shape
    T = x.shape[1]
    if C_ % 4 or shift < 0 or shift + Tp > T:
        raise ValueError(f"{what}: C % 4 == 0 and 0 <= shift, shift + T' <= T (C {C_}, shift {shift}, T' {Tp}, T {T})")
    return B, T, Tp, C_


def ftdnn_bypass(y: Tensor, x: Tensor, scale: float, shift: int, x_split: bool = False, out_split: bool = False) -> Tensor:
    """y [B,T',C] fp32 + scale * x[:, shift:shift + T'] -> [B,T',C]; ``x_split`` / ``out_split``: x is / the result comes in the split
    activation format (C % 32 == 0)."""
    B, T, Tp, C_ = _bypass_check(y, x, shift, "ftdnn_bypass")
    if (x_split or out_split) and C_ % 32:
        raise ValueError("ftdnn_bypass: the split activation format needs C % 32 == 0")
    out = _empty((B, Tp, C_), y.device)
    call("dlip_ftdnn_bypass_f32", y, x, out, B, T, Tp, C_, int(shift), float(scale), int(bool(x_split)) | 2 * int(bool(out_split)))
    return out


def ftdnn_bypass_bwd(dy: Tensor, dx: Tensor, scale: float, shift: int) -> Tensor:
    """dx[:, shift:shift + T'] += scale * dy, IN PLACE on dx [B,T,C] (the factor convolution's data gradient); returns dx."""
    B, T, Tp, C_ = _bypass_check(dy, dx, shift, "ftdnn_bypass_bwd")
    call("dlip_ftdnn_bypass_bwd_f32", dy, dx, B, T, Tp, C_, int(shift), float(scale))
    return dx


def semi_orth_workspace(n_mats: int, device) -> Tensor:
    """The zeroed workspace dlip_semi_orth_step_f32 keeps for ``n_mats`` matrices (ticket words + partial Gram matrices)."""
    nbytes = int(lib().dlip_semi_orth_workspace_bytes(int(n_mats)))
    if nbytes <= 0:
        raise ValueError(f"semi-orthogonal step: 1 .. {SEMI_ORTH_MAX_MATS} matrices, got {n_mats}")
    return torch.zeros(nbytes, dtype=torch.uint8, device=device)


def semi_orth_table(mats: Sequence[Tensor]) -> Tuple[Tensor, int, int]:
    """(device table, max rows, max cols) of the matrices ``mats``: each a contiguous fp32 CUDA tensor whose first axis is the rows
    (a factor weight [Bn, Cin, k] is the matrix [Bn, Cin k])."""
    import numpy as np
    if not 1 <= len(mats) <= SEMI_ORTH_MAX_MATS:
        raise ValueError(f"semi-orthogonal step: 1 .. {SEMI_ORTH_MAX_MATS} matrices, got {len(mats)}")
    dt = np.dtype([("M", "<u8"), ("rows", "<i4"), ("cols", "<i4")])
    tab = np.zeros(len(mats), dtype=dt)
    for i, m in enumerate(mats):
        _req(m, f"matrix {i}")
        rows, cols = int(m.shape[0]), int(m.numel() // max(int(m.shape[0]), 1))
        if m.dim() < 2 or not 1 <= rows <= SEMI_ORTH_MAX_ROWS or cols < rows:
            raise ValueError(f"semi-orthogonal step: matrix {i} is {rows} x {cols}; 1 <= rows <= {SEMI_ORTH_MAX_ROWS} and rows <= cols")
        tab[i] = (m.data_ptr(), rows, cols)
    dev = torch.from_numpy(tab.view(np.uint8).copy()).to(mats[0].device)
    return dev, int(tab["rows"].max()), int(tab["cols"].max())


def semi_orth_step(table: Tensor, n_mats: int, max_rows: int, max_cols: int, counter: Tensor, every: int, workspace: Tensor) -> None:
    """One call of the semi-orthogonal step (launches only): advances ``counter`` (int32 [2] on the device) and, when the step it then
    counts is a multiple of ``every`` > 0, updates every matrix of ``table`` in place."""
    _req(counter, "counter", torch.int32)
    _req(table, "table", torch.uint8); _req(workspace, "workspace", torch.uint8)
    if counter.numel() != 2 or table.numel() != 16 * n_mats:
        raise ValueError("semi-orthogonal step: counter is int32 [2], the table holds 16 bytes per matrix")
    call("dlip_semi_orth_step_f32", table, int(n_mats), int(max_rows), int(max_cols), counter, int(every), workspace, workspace.numel())
