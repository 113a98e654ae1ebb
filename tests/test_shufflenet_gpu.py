"""Lipreading(backbone_type='shufflenet') on the HIP engine (-m gpu): the reference's goldens (tests/golden/shufflenet_golden.npz)
for every width, an fp64 CPU restatement at B = 8, T = 29, the AvgPool2d(3) window at 112 x 112, kernel-level checks of the new
entry points at odd shapes (NaN-prefilled outputs: padding channels exactly zero, no NaN in a real channel), ragged / uint8 / batch
invariance, arithmetic-mode independence and a recorded StepPlan."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, assert_close_rel
from deeplip_amd import arith, ops
from deeplip_amd import shufflenet as sn
from deeplip_amd import weightgen as wg
from deeplip_amd.video import Lipreading

pytestmark = pytest.mark.gpu

DEV = "cuda"
TCN_OPTS = {"num_layers": 4, "kernel_size": [3, 5, 7], "dropout": 0.2, "dwpw": False, "width_mult": 1}
WIDTHS = (0.5, 1.0, 1.5, 2.0)
D = torch.float64


def tag(w):
    return str(w).replace(".", "p")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "shufflenet_golden.npz"))


def build(width, relu_type="prelu", extract_feats=True, prefix=None):
    m = Lipreading(hidden_dim=256, backbone_type="shufflenet", num_classes=54, relu_type=relu_type, tcn_options=TCN_OPTS,
                   width_mult=width, extract_feats=extract_feats)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()},
                            prefix=prefix if prefix is not None else f"shufflenet_{tag(width)}_{relu_type}.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval().to(DEV), {k: torch.from_numpy(v) for k, v in sd.items()}


def clips(B, T=5, size=88, key="shufflenet.video"):
    return torch.from_numpy(wg.video_input(B, frames=T, size=size, key=key))


def close(got, want, rtol=1e-4, what=""):
    assert_close_rel(torch.as_tensor(got).detach().double().cpu().numpy(), torch.as_tensor(want).double().cpu().numpy(), rtol=rtol,
                     what=what)


# ---- fp64 CPU restatement of the reference (model.py:80-90, shufflenetv2.py) -------------------------------------------------
def _bn(y, sd, pre):
    return F.batch_norm(y, sd[pre + ".running_mean"].double(), sd[pre + ".running_var"].double(), sd[pre + ".weight"].double(),
                        sd[pre + ".bias"].double(), training=False, eps=1e-5)


def _conv(y, sd, pre, stride=1, groups=1):
    w = sd[pre + ".weight"].double()
    return F.conv2d(y, w, stride=stride, padding=w.shape[-1] // 2, groups=groups)


def _banch2(y, sd, pre, stride):
    y = F.relu(_bn(_conv(y, sd, pre + ".0"), sd, pre + ".1"))
    y = _bn(_conv(y, sd, pre + ".3", stride, groups=y.shape[1]), sd, pre + ".4")
    return F.relu(_bn(_conv(y, sd, pre + ".5"), sd, pre + ".6"))


def ref_features(sd, x, relu_type):
    y = F.conv3d(x.double(), sd["frontend3D.0.weight"].double(), stride=(1, 2, 2), padding=(2, 3, 3))
    y = _bn(y, sd, "frontend3D.1")
    y = F.prelu(y, sd["frontend3D.2.weight"].double()) if relu_type == "prelu" else F.relu(y)
    y = F.max_pool3d(y, (1, 3, 3), (1, 2, 2), (0, 1, 1))
    B, C, T, H, W = y.shape
    y = y.transpose(1, 2).reshape(B * T, C, H, W)
    for u in range(16):
        pre = f"trunk.0.{u}"
        if u in (0, 4, 12):
            b1 = _bn(_conv(y, sd, pre + ".banch1.0", 2, groups=y.shape[1]), sd, pre + ".banch1.1")
            b1 = F.relu(_bn(_conv(b1, sd, pre + ".banch1.2"), sd, pre + ".banch1.3"))
            out = torch.cat([b1, _banch2(y, sd, pre + ".banch2", 2)], 1)
        else:
            h = y.shape[1] // 2
            out = torch.cat([y[:, :h], _banch2(y[:, h:], sd, pre + ".banch2", 1)], 1)
        y = sn.channel_shuffle(out, 2)
    y = F.relu(_bn(_conv(y, sd, "trunk.1.0"), sd, "trunk.1.1"))
    y = F.avg_pool2d(y, 3)
    return y.reshape(B, T, -1)


# ---- model level --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,relu_type", [(w, "prelu") for w in WIDTHS] + [(1.0, "relu")])
def test_features_match_reference_golden(gold, width, relu_type):
    m, _ = build(width, relu_type)
    with torch.no_grad():
        got = m(clips(2).to(DEV), [5, 5])
    key = f"feats_w{tag(width)}" + ("_relu" if relu_type == "relu" else "")
    assert got.shape == gold[key].shape
    close(got, gold[key], what=key)


def test_per_stage_taps_match_golden(gold):
    m, _ = build(1.0)
    taps = {}
    with torch.no_grad():
        m(clips(2).to(DEV), [5, 5], taps=taps)
    close(taps["stem"][0].permute(2, 0, 1), gold["tap_stem"], what="stem")
    for k in ("stage2", "stage3", "stage4", "conv_last"):
        close(taps[k][0].permute(2, 0, 1), gold["tap_" + k], what=k)


def test_logits_and_argmax_match_golden(gold):
    m, _ = build(1.0, extract_feats=False)
    x = clips(4, T=8, key="shufflenet.video.logits").to(DEV)
    lengths = gold["logits_lengths"].tolist()
    with torch.no_grad():
        logits = m(x, lengths)
    close(logits, gold["logits_w1p0"], what="logits")
    assert torch.equal(logits.argmax(dim=1).cpu(), torch.from_numpy(gold["logits_argmax"]))
    with torch.no_grad():
        pooled = m.classifier_features(x, lengths)
    ref = pooled @ m.tcn.tcn_output.weight.t() + m.tcn.tcn_output.bias
    close(ref, gold["logits_w1p0"], what="classifier_features @ tcn_output")


@pytest.mark.parametrize("width,relu_type", [(1.0, "prelu"), (2.0, "relu")])
def test_full_clip_batch_against_fp64_restatement(width, relu_type):
    m, sd = build(width, relu_type, prefix=f"sn_fp64_{tag(width)}.")
    x = clips(8, T=29, key="shufflenet.video.b8")
    with torch.no_grad():
        got = m(x.to(DEV), [29] * 8)
    close(got, ref_features(sd, x, relu_type), what=f"B=8 T=29 width {width}")


def test_112_uses_top_left_window_and_bad_sizes_raise(gold):
    m, _ = build(1.0)
    x = clips(1, T=3, size=112, key="shufflenet.video.112").to(DEV)
    with torch.no_grad():
        got = m(x, [3])
    close(got, gold["feats_w1p0_112"], what="112x112")
    for s in (64, 176):
        with pytest.raises(ValueError):
            m(torch.zeros(1, 1, 2, s, s, device=DEV), [2])


def test_ragged_embed_rows_match_single_clips():
    m, _ = build(1.0)
    x = clips(3, T=12, key="shufflenet.video.ragged").to(DEV)
    lengths = [12, 7, 4]
    with torch.no_grad():
        e = m.embed(x, lengths)
        for b, L in enumerate(lengths):
            alone = m.embed(x[b:b + 1, :, :L].contiguous())
            close(e[b:b + 1], alone, rtol=1e-5, what=f"row {b}")
    assert e.shape == (3, 1024)


def test_uint8_frames_match_the_float_clip():
    m, _ = build(0.5)
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, 4, 88, 88), dtype=torch.uint8, generator=g)
    x = ((u8.double() / 255.0 - 0.421) / 0.165).float().view(2, 1, 4, 88, 88)
    with torch.no_grad():
        got = m(u8.to(DEV), [4, 4])
        want = m(x.to(DEV), [4, 4])
        close(got, want, rtol=1e-5, what="uint8 gray")
        rgb = u8.unsqueeze(2).expand(2, 4, 3, 88, 88).contiguous().to(DEV)
        from deeplip_amd.frontend import VideoFrontend
        assert torch.equal(m(rgb, [4, 4]), m(VideoFrontend(88)(rgb), [4, 4]))


def test_batch_invariance():
    m, _ = build(1.5)
    x = clips(4, T=6, key="shufflenet.video.batch").to(DEV)
    with torch.no_grad():
        full = m.embed(x)
        for b in range(4):
            close(full[b:b + 1], m.embed(x[b:b + 1]), rtol=1e-5, what=f"clip {b}")


def test_every_arith_mode_is_exact_fp32():
    m, _ = build(1.0, extract_feats=False)
    x = clips(2, T=6, key="shufflenet.video.arith").to(DEV)
    outs = {}
    for mode in ("f32", "auto", "f16x3"):
        arith.configure(mode)
        with torch.no_grad():
            outs[mode] = (m.embed(x), m(x, [6, 4]), m.classifier_features(x, [6, 4]))
    for mode in ("auto", "f16x3"):
        for a, b in zip(outs[mode], outs["f32"]):
            assert torch.equal(a, b), mode


@pytest.mark.parametrize("mode", ["f32", "auto"])
def test_step_plan_replay_equals_eager(mode):
    from deeplip_amd.plan import StepPlan
    arith.configure(mode)
    m, _ = build(1.0)
    x = clips(4, T=8, key="shufflenet.video.plan").to(DEV)
    with torch.no_grad():
        plan = StepPlan(lambda v: m.embed(v), x.clone())
        x2 = clips(4, T=8, key="shufflenet.video.plan2").to(DEV)
        out = plan(x2)
        got = (out[0] if isinstance(out, (list, tuple)) else out).clone()
        torch.cuda.synchronize()
        want = m.embed(x2)
    assert torch.equal(got, want)
    assert 30 <= plan.launches <= 45
    plan.close()


def test_training_mode_raises():
    m, _ = build(0.5)
    m.train()
    with pytest.raises(NotImplementedError, match="training"):
        m(clips(1, T=2).to(DEV), [2])


# ---- kernel level -------------------------------------------------------------------------------------------------------------
def _ref_dwpw(x, w_kc, b, dw=None, dwb=None, stride=1):
    a = x.double().permute(0, 3, 1, 2)
    if dw is not None:
        C = a.shape[1]
        a = F.conv2d(a, dw.double().t().reshape(C, 1, 3, 3), dwb.double(), stride=stride, padding=1, groups=C)
    return torch.relu(torch.einsum("nchw,kc->nhwk", a, w_kc.double()) + b.double())


# input channel counts are the padded layout's (58 -> 60, 122 -> 124: the kernel reads float4 groups); outputs are the odd widths
@pytest.mark.parametrize("C,K,stride,H", [(24, 24, 2, 22), (60, 58, 1, 11), (60, 58, 2, 11), (124, 122, 1, 7), (124, 122, 2, 11),
                                          (232, 116, 2, 6), (96, 48, 1, 5), (24, 58, 2, 11)])
def test_dwpw_kernel_shuffled_output(C, K, stride, H):
    g = torch.Generator().manual_seed(C * 100 + K + stride)
    N, W = 3, H + 2
    hp = (K + 3) // 4 * 4
    Cx = C + 8                                          # read a channel slice [4, 4 + C) of a wider tensor
    x = torch.randn(N, H, W, Cx, generator=g)
    dw = torch.randn(9, C, generator=g)
    dwb = torch.randn(C, generator=g) * 0.1
    wkc = torch.randn(K, C, generator=g) / C ** 0.5
    b = torch.randn(K, generator=g) * 0.1
    wp = torch.zeros((C + 31) // 32 * 32, (K + 63) // 64 * 64)
    wp[:C, :K] = wkc.t()
    Ho, Wo = (H, W) if stride == 1 else ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
    out = torch.full((N, Ho, Wo, 2 * hp), float("nan"), device=DEV)
    passthrough = torch.randn(N, H, W, hp + 4, generator=g).to(DEV) if stride == 1 else None
    dev = lambda t: t.contiguous().to(DEV)
    ops.shuffle_dwpw(dev(x), dev(wp), dev(b), dw_w=dev(dw), dw_b=dev(dwb), stride=stride, in_channels=C, in_channel_offset=4,
                     out=out, hp=hp, par=1, passthrough=passthrough)
    if stride == 2:                                    # the other branch: a plain 1x1 of the same slice can't be strided; reuse dw
        ops.shuffle_dwpw(dev(x), dev(wp), dev(b), dw_w=dev(dw), dw_b=dev(dwb), stride=2, in_channels=C, in_channel_offset=4,
                         out=out, hp=hp, par=0)
    torch.cuda.synchronize()
    y = out.cpu()
    ref = _ref_dwpw(x[..., 4:4 + C], wkc, b, dw, dwb, stride)
    pos1 = sn.shuffle_positions(K, hp, 1)
    pos0 = sn.shuffle_positions(K, hp, 0)
    close(y[..., pos1], ref, what="banch2 positions")
    if stride == 1:
        assert torch.equal(y[..., pos0], passthrough.cpu()[..., :K])
    else:
        close(y[..., pos0], ref, what="banch1 positions")
    pads = sorted(set(range(2 * hp)) - set(pos0.tolist()) - set(pos1.tolist()))
    assert len(pads) == 2 * (hp - K)
    if pads:
        assert torch.equal(y[..., pads], torch.zeros_like(y[..., pads]))
    assert not torch.isnan(y).any()


def test_dwpw_refuses_unaligned_input_slices():
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    w = torch.zeros(64, 64, device=DEV)
    b = torch.zeros(58, device=DEV)
    with pytest.raises(ValueError):
        ops.shuffle_dwpw(x, w, b, in_channels=58)
    with pytest.raises(ValueError):
        ops.shuffle_dwpw(x, w, b, in_channels=56, in_channel_offset=2)


@pytest.mark.parametrize("C,K", [(60, 58), (24, 24), (124, 122)])
def test_plain_pw_kernel_slice_in_plain_out(C, K):
    g = torch.Generator().manual_seed(7 + C)
    N, H, W = 2, 5, 7
    x = torch.randn(N, H, W, 2 * C, generator=g)
    wkc = torch.randn(K, C, generator=g) / C ** 0.5
    b = torch.randn(K, generator=g) * 0.1
    wp = torch.zeros((C + 31) // 32 * 32, (K + 63) // 64 * 64)
    wp[:C, :K] = wkc.t()
    out = torch.full((N, H, W, K + 6), float("nan"), device=DEV)
    ops.shuffle_dwpw(x.to(DEV), wp.to(DEV), b.to(DEV), in_channels=C, in_channel_offset=C, out=out)
    torch.cuda.synchronize()
    y = out.cpu()
    close(y[..., :K], _ref_dwpw(x[..., C:], wkc, b), what="plain 1x1")
    assert torch.isnan(y[..., K:]).all()                 # nothing written beyond the K channels of a plain output


@pytest.mark.parametrize("B,T,H,W", [(2, 5, 88, 88), (1, 3, 112, 112), (1, 2, 40, 56)])
def test_stem24_kernel(B, T, H, W):
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(B, T, H, W, generator=g)
    w = torch.randn(24, 1, 5, 7, 7, generator=g) / 245 ** 0.5
    b = torch.randn(24, generator=g) * 0.1
    slope = torch.rand(24, generator=g) * 0.3
    wp = torch.zeros(248, 32)
    wp[:245, :24] = w.reshape(24, 245).t()
    y = ops.shuffle_stem24(x.to(DEV), wp.to(DEV), b.to(DEV), slope.to(DEV))
    ref = F.conv3d(x.double().view(B, 1, T, H, W), w.double(), b.double(), stride=(1, 2, 2), padding=(2, 3, 3))
    ref = F.prelu(ref, slope.double()).permute(0, 2, 3, 4, 1).reshape(B * T, H // 2, W // 2, 24)
    close(y, ref, what="stem24")


@pytest.mark.parametrize("H,W", [(3, 3), (4, 4), (5, 3)])
def test_avgpool3_kernel_top_left_window(H, W):
    x = torch.randn(6, H, W, 40)
    y = ops.avgpool3(x.to(DEV))
    close(y, x.double()[:, :3, :3].mean(dim=(1, 2)), what="avgpool3")
    with pytest.raises(ValueError):
        ops.avgpool3(torch.zeros(1, 6, 6, 4, device=DEV))
