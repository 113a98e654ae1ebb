"""Training under ``--arith f32`` (-m gpu): the kernel-level gradient checks, the golden steps and the recorded step of the two
encoders run again with ``autograd_video.TRAIN_CONV == "f32"`` -- the session's baseline pins the split-fp16 routes, so the other
modules never take the exact mode's ones (ConvTrainFn / StemConvTrainFn / TDNNBlockTrainFn in mode 0, conv_train's permuted
weight banks, dlip_upsample_zero_f32, wgrad_conv_fused, the stem's GEMM weight-gradient route) -- and the mode's promise across
input magnitudes: forward and data gradient are the exact fp32 kernel; the weight gradient is a split-fp16 GEMM whose BOTH
operands carry a power-of-two lift of their own, so no magnitude of the layer input may raise DeepLipRangeError or cost accuracy.

The reference is always the same operation under torch-CPU autograd in fp64; where a bar depends on the magnitude it is
max(project bar, 2 x floor), floor = the same torch-CPU operation in fp32 against fp64 (as test_full_size_training_step_vs_fp64_oracle).
Project bars (test_conv_train_fn_gradients, test_tdnn_block_train_fn_gradients): 2e-5 on outputs, 1e-4 on every gradient."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_OUT, BAR_GRAD = 2e-5, 1e-4


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@pytest.fixture(autouse=True)
def _clean_status():
    from deeplip_amd import _lib
    torch.cuda.synchronize()
    _lib.status_words().zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_words().zero_()


def _configure(mode):
    from deeplip_amd import arith, autograd_video as av
    arith.configure(mode)          # (conftest's _arith_isolated restores the session's baseline after the test)
    assert av.TRAIN_CONV == mode


def _np(t):
    return t.detach().cpu().double().numpy()


def _compare(what, got, ref, floor=None):
    """Every quantity of ``ref`` against ``got``: printed, then asserted.  'y' holds the output bar, everything else the gradient bar."""
    bad = []
    for k, r in ref.items():
        bar = BAR_OUT if k == "y" else BAR_GRAD
        if floor is not None:
            bar = max(bar, 2.0 * floor[k])
        e = rel_err(got[k], r)
        print(f"\n{what}: {k} rel err {e:.3e} (bar {bar:.1e}" + (f", fp32 floor {floor[k]:.1e})" if floor is not None else ")"), end="")
        if not e < bar:
            bad.append((k, e, bar))
    assert not bad, (what, bad)


# ---- Conv2d / Conv1d (H = 1) --------------------------------------------------------------------------------------------------
def _conv_geometry(case):
    N, H, W, C, K, R, S, stride, pad, dil, bias = case
    one = H == 1
    return ((1, stride) if one else (stride, stride)), ((0, pad) if one else (pad, pad)), ((1, dil) if one else (dil, dil))


@functools.lru_cache(maxsize=None)
def _conv_inputs(case, s, gs):
    N, H, W, C, K, R, S, stride, pad, dil, bias = case
    (sh, sw), (ph, pw), (dh, dw) = _conv_geometry(case)
    Ho = (H + 2 * ph - dh * (R - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (S - 1) - 1) // sw + 1
    x = rnd(N, C, H, W, seed=1) * s
    w = rnd(K, C, R, S, seed=2, scale=1.0 / np.sqrt(C * R * S))
    b = rnd(K, seed=3, scale=0.1) if bias else None
    dy = rnd(N, K, Ho, Wo, seed=4) * gs
    return x, w, b, dy


@functools.lru_cache(maxsize=None)
def _conv_reference(case, s, gs, dtype):
    x, w, b, dy = _conv_inputs(case, s, gs)
    geo = _conv_geometry(case)
    xr, wr = x.detach().clone().to(dtype).requires_grad_(), w.detach().clone().to(dtype).requires_grad_()
    br = b.detach().clone().to(dtype).requires_grad_() if b is not None else None
    y = F.conv2d(xr, wr, br, stride=geo[0], padding=geo[1], dilation=geo[2])
    assert y.shape == dy.shape
    y.backward(dy.to(dtype))
    out = {"y": _np(nhwc(y)), "dx": _np(nhwc(xr.grad)), "dW": _np(wr.grad)}
    if b is not None:
        out["db"] = _np(br.grad)
    return out


def _floor(ref32, ref64):
    return {k: rel_err(ref32[k], ref64[k]) for k in ref64}


def _conv_engine(case, s, gs):
    from deeplip_amd import autograd_video as av
    x, w, b, dy = _conv_inputs(case, s, gs)
    geo = _conv_geometry(case)
    xg = nhwc(x).to(DEV).detach().requires_grad_()
    wg_ = w.to(DEV).detach().requires_grad_()
    bg = b.to(DEV).detach().requires_grad_() if b is not None else None
    y = av.conv(xg, wg_, bg, stride=geo[0], pad=geo[1], dil=geo[2])
    y.backward(nhwc(dy).to(DEV))
    torch.cuda.synchronize()
    out = {"y": _np(y), "dx": _np(xg.grad), "dW": _np(wg_.grad)}
    if b is not None:
        out["db"] = _np(bg.grad)
    return out


CONV_CASES = [
    (3, 7, 9, 8, 12, 3, 3, 1, 1, 1, True),         # C = 8: one ragged 32-channel block of the narrow operand kernel, K % 32 != 0, non-square; J = 189: 6 blocks -> odd-pitch bump
    (2, 8, 6, 64, 32, 3, 3, 2, 1, 1, False),       # stride 2 on an even input (spare filter row), wide<64> producer; J = 24 < 32: one block with a zero tail
    (5, 5, 7, 128, 64, 3, 3, 2, 1, 1, False),      # stride 2 on odd sizes, wide<128>; J = 60: 2 blocks -> 3
    (33, 1, 13, 36, 40, 1, 5, 1, 8, 2, True),      # H = 1, dilation 2 with full padding, N > 32, C = 36 (32 + 4)
    (2, 6, 6, 96, 64, 1, 1, 2, 0, 1, False),       # 1x1 stride 2, C = 96 (neither wide kernel)
    (2, 9, 5, 32, 32, 3, 3, 1, 2, 2, False),       # dilation 2 in H and W
]


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_conv_gradients_in_both_modes(case, mode):
    """autograd_video.conv: y, dx, dW, db vs torch-CPU autograd (fp64) at the smallest shapes that reach a branch no other case reaches."""
    from deeplip_amd import _lib
    _configure(mode)
    ref = _conv_reference(case, 1.0, 1.0, torch.float64)
    got = _conv_engine(case, 1.0, 1.0)        # (every case has C % 4 == K % 4 == 0: neither mode may refuse it)
    _lib.check_range(sync=True)
    _compare(f"conv {case} [{mode}]", got, ref)


# ---- the stem's Conv3d ----------------------------------------------------------------------------------------------------------
STEM = (1, 3, 24, 40)


@functools.lru_cache(maxsize=None)
def _stem_inputs(s, gs):
    B, T, H, W = STEM
    x = rnd(B, 1, T, H, W, seed=5) * s
    w = rnd(64, 1, 5, 7, 7, seed=6, scale=1.0 / np.sqrt(245))
    dy = rnd(B, 64, T, H // 2, W // 2, seed=7) * gs
    return x, w, dy


def _stem_rows(t):
    B, T, H, W = STEM
    return t.permute(0, 2, 3, 4, 1).reshape(B * T, H // 2, W // 2, 64).contiguous()


@functools.lru_cache(maxsize=None)
def _stem_reference(s, gs, dtype):
    x, w, dy = _stem_inputs(s, gs)
    wr = w.detach().clone().to(dtype).requires_grad_()
    y = F.conv3d(x.to(dtype), wr, None, stride=(1, 2, 2), padding=(2, 3, 3))
    assert y.shape == dy.shape
    y.backward(dy.to(dtype))
    return {"y": _np(_stem_rows(y)), "dW": _np(wr.grad)}


def _stem_engine(s, gs):
    from deeplip_amd import autograd_video as av
    x, w, dy = _stem_inputs(s, gs)
    wg_ = w.to(DEV).detach().requires_grad_()
    y = av.stem_conv(x.view(*STEM).to(DEV), wg_)
    y.backward(_stem_rows(dy).to(DEV))
    torch.cuda.synchronize()
    return {"y": _np(y), "dW": _np(wg_.grad)}


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
def test_stem_conv_gradients_in_both_modes(mode):
    """autograd_video.stem_conv against F.conv3d (fp64); in f32 the weight gradient takes the GEMM route (dlip_stem_wgrad_operand_f32)."""
    from deeplip_amd import _lib
    _configure(mode)
    got = _stem_engine(1.0, 1.0)
    _lib.check_range(sync=True)
    _compare(f"stem {STEM} [{mode}]", got, _stem_reference(1.0, 1.0, torch.float64))


# ---- TDNN block: Conv1d + batch-statistics BatchNorm + LeakyReLU ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tdnn_inputs(case, s, gs):
    B, T, C, K, S, dil, act_first = case
    x = rnd(B, C, T, seed=11) * s                                           # reference layout [B,C,T]
    w = rnd(K, C, S, seed=12, scale=1.0 / np.sqrt(C * S))
    b = rnd(K, seed=13, scale=0.1)
    gamma = torch.rand(K, generator=torch.Generator().manual_seed(14)) + 0.5
    beta = rnd(K, seed=15, scale=0.2)
    dy = rnd(B, K, T - dil * (S - 1), seed=16) * gs
    return x, w, b, gamma, beta, dy


@functools.lru_cache(maxsize=None)
def _tdnn_reference(case, s, gs, dtype):
    B, T, C, K, S, dil, act_first = case
    x, w, b, gamma, beta, dy = _tdnn_inputs(case, s, gs)
    xr, wr, br, gr, ber = (t.detach().clone().to(dtype).requires_grad_() for t in (x, w, b, gamma, beta))
    z = F.conv1d(xr, wr, br, dilation=dil)
    if act_first:
        y = F.batch_norm(F.leaky_relu(z, 0.2), None, None, gr, ber, training=True, eps=1e-5)
    else:
        y = F.leaky_relu(F.batch_norm(z, None, None, gr, ber, training=True, eps=1e-5), 0.2)
    assert y.shape == dy.shape
    y.backward(dy.to(dtype))
    out = {"y": _np(y), "dx": _np(xr.grad), "dW": _np(wr.grad), "dgamma": _np(gr.grad), "dbeta": _np(ber.grad)}
    if act_first:           # (otherwise the bias sits in front of a batch-statistics BN: its exact gradient is zero -- see _tdnn_check)
        out["db"] = _np(br.grad)
    return out


def _tdnn_engine(case, s, gs):
    from deeplip_amd import autograd as ag
    B, T, C, K, S, dil, act_first = case
    x, w, b, gamma, beta, dy = _tdnn_inputs(case, s, gs)
    xg = x.permute(0, 2, 1).contiguous().to(DEV).detach().requires_grad_()            # [B,T,C]
    wg_, bg, gg, beg = (t.to(DEV).detach().requires_grad_() for t in (w, b, gamma, beta))
    rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    y = ag.TDNNBlockTrainFn.apply(xg, wg_, bg, gg, beg, rm, rv, 0.1, 1e-5, 0.2, dil, act_first)
    y.backward(dy.permute(0, 2, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    return {"y": _np(y.permute(0, 2, 1)), "dx": _np(xg.grad.permute(0, 2, 1)), "dW": _np(wg_.grad), "dgamma": _np(gg.grad), "dbeta": _np(beg.grad),
            "db": _np(bg.grad)}


def _tdnn_check(what, case, s, gs, got, floor=None):
    K, act_first = case[3], case[6]
    _compare(what, got, _tdnn_reference(case, s, gs, torch.float64), floor)
    if not act_first:       # as test_tdnn_block_train_fn_gradients: zero up to rounding on both sides (the absolute term follows dy's scale)
        dy = _tdnn_inputs(case, s, gs)[5]
        assert float(np.abs(got["db"]).max()) < 1e-4 * float(dy.abs().sum() / K) + 1e-5 * gs


TDNN_CASES = [(4, 60, 24, 64, 5, 1, False), (2, 40, 64, 100, 3, 1, True), (3, 45, 64, 64, 1, 1, True), (2, 47, 36, 40, 3, 3, False)]


@pytest.mark.parametrize("mode", ["f16x3", "f32"])
@pytest.mark.parametrize("case", TDNN_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_tdnn_block_gradients_in_both_modes(case, mode):
    """autograd.TDNNBlockTrainFn: output and d/dx, d/dW, d/db, d/dgamma, d/dbeta vs torch-CPU autograd (fp64)."""
    from deeplip_amd import _lib
    _configure(mode)
    got = _tdnn_engine(case, 1.0, 1.0)        # (every case has C % 4 == K % 4 == 0: neither mode may refuse it)
    _lib.check_range(sync=True)
    _tdnn_check(f"tdnn {case} [{mode}]", case, 1.0, 1.0, got)


# ---- the f32 promise across magnitudes -------------------------------------------------------------------------------------------------
SCALES = (2.0 ** -20, 1e-3, 1.0, 1e3, 1e5, 2.0 ** 20)      # 2^-20 .. 2^+20: the range the README claims for `auto` after calibration
GRAD_SCALES = (1.0, 1e-6)
MAG_CONV = (3, 12, 12, 64, 64, 3, 3, 1, 1, 1, False)
MAG_TDNN = (4, 60, 24, 64, 5, 1, False)


@pytest.mark.parametrize("s", SCALES, ids=lambda v: f"{v:.3g}")
def test_f32_conv_is_silent_and_fp32_grade_at_any_input_magnitude(s):
    """Layer input scaled by ``s``, dy at unit scale and at 1e-6: the range check stays silent, and y, dx, dW are within
    max(project bar, 2 x the fp32 floor) of fp64.  The fp32 floors here are below 1e-6, so the project bars decide.  Measured (MI355X):
    y <= 1.1e-6, dx <= 1.0e-6, dW <= 6.0e-7 at every s.  With the layer input split unlifted in the weight gradient (as it was): dW 1.9e-2
    at s = 2^-20, 1.6e-5 at 1e-3, DeepLipRangeError at s = 1e5 and 2^20 (EXPERIMENTS.md R6.21)."""
    from deeplip_amd import _lib
    _configure("f32")
    for gs in GRAD_SCALES:
        ref = _conv_reference(MAG_CONV, s, gs, torch.float64)
        floor = _floor(_conv_reference(MAG_CONV, s, gs, torch.float32), ref)
        got = _conv_engine(MAG_CONV, s, gs)
        _lib.check_range(sync=True)
        _compare(f"f32 conv, input x {s:.3g}, dy x {gs:g}", got, ref, floor)


@pytest.mark.parametrize("s", SCALES, ids=lambda v: f"{v:.3g}")
def test_f32_stem_is_silent_and_fp32_grade_at_any_input_magnitude(s):
    """The same for the stem (its weight gradient: the GEMM route over dlip_stem_wgrad_operand_f32, from a lifted copy of the clip)."""
    from deeplip_amd import _lib
    _configure("f32")
    for gs in GRAD_SCALES:
        ref = _stem_reference(s, gs, torch.float64)
        floor = _floor(_stem_reference(s, gs, torch.float32), ref)
        got = _stem_engine(s, gs)
        _lib.check_range(sync=True)
        _compare(f"f32 stem, clip x {s:.3g}, dy x {gs:g}", got, ref, floor)


@pytest.mark.parametrize("s", SCALES[1:], ids=lambda v: f"{v:.3g}")
def test_f32_tdnn_block_is_silent_and_fp32_grade_at_any_input_magnitude(s):
    """The same for a TDNN block.  (2^-20 is left out: there eps dominates the batch variance and torch's own fp32 dgamma is 5.7e-3
    from fp64 -- nothing a convolution's arithmetic can be held to.)  At 1e-3 the block's bias (0.1) is 100 x the convolution's sum: with
    the bias in the accumulators from the start the output was 2.8e-5 from fp64 (torch fp32: 5.0e-6); the training path adds it last: 2.9e-6, dgamma 4.1e-6."""
    from deeplip_amd import _lib
    _configure("f32")
    for gs in GRAD_SCALES:
        ref = _tdnn_reference(MAG_TDNN, s, gs, torch.float64)
        floor = _floor(_tdnn_reference(MAG_TDNN, s, gs, torch.float32), ref)
        got = _tdnn_engine(MAG_TDNN, s, gs)
        _lib.check_range(sync=True)
        _tdnn_check(f"f32 tdnn, input x {s:.3g}, dy x {gs:g}", MAG_TDNN, s, gs, got, floor)


@pytest.mark.parametrize("which", ["conv", "tdnn"])
def test_f16x3_training_reports_an_input_of_magnitude_1e5(which):
    """The other half of the pair of contracts: the split-fp16 training routes cannot hold |v| >= 65520 and say so."""
    from deeplip_amd import _lib
    _configure("f16x3")
    if which == "conv":
        _conv_engine(MAG_CONV, 1e5, 1.0)
    else:
        _tdnn_engine(MAG_TDNN, 1e5, 1.0)
    with pytest.raises(_lib.DeepLipRangeError):
        _lib.check_range(sync=True)


# ---- whole steps in f32: the golden steps and the recorded step, their assertions unchanged -----------------------------------------
def test_lipreading_train_step_matches_reference_golden_in_f32():
    import test_train_video_gpu as tv
    _configure("f32")
    tv.lipreading_train_step_vs_reference_golden()


def test_recorded_training_step_is_bit_identical_to_eager_in_f32():
    import test_train_video_gpu as tv
    _configure("f32")
    tv.recorded_training_step_vs_eager(4, 9)


def test_speaker_encoder_two_sgd_steps_vs_reference_golden_in_f32(golden):
    import test_train_audio_gpu as ta
    _configure("f32")
    ta.speaker_encoder_two_sgd_steps_vs_reference_golden(golden["audio_train"])


def test_attentive_speaker_encoder_two_sgd_steps_vs_reference_golden_in_f32(golden):
    import test_train_audio_gpu as ta
    _configure("f32")
    ta.attentive_speaker_encoder_two_sgd_steps_vs_reference_golden(golden["audio_attn_train"])
