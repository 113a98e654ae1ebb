"""`pooling: multi_head_attention` (-m gpu; DESIGN.md 4h, ABI 64): the dlip_mh_attn_* kernels and deeplip_amd.audio.MultiHeadAttention in
both speech encoders against the fp64 restatement of the definition (tests/mh_attn_reference.py, plain torch with autograd).
Bars (the project's own for this family, tests/test_train_audio_gpu.py): outputs 1e-5, gradients 1e-4, max|a - b| / max|b|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mh_attn_reference as R
from conftest import assert_close_rel, rel_err
from deeplip_amd import weightgen as wg
from oracle import deeplip_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_OUT, BAR_GRAD = 1e-5, 1e-4

CASES = {
    "unequal-heads": (3, 41, 64, [8, 12, 20, 24]),             # T no multiple of the wave count
    "few-frames": (2, 5, 8, [4, 4]),                            # fewer frames than waves; C below one channel block
    "single-frame": (2, 1, 8, [4, 8, 4]),
    "long": (4, 300, 40, [6, 10]),                              # T above one 256-frame pass; S no multiple of 64; C % 64 != 0
    "etdnn-width": (2, 37, 1500, [100, 200, 300, 400]),         # the stub's default widths at the E-TDNN's channel count
    "one-head": (3, 41, 64, [16]),
    "eight-heads": (2, 19, 24, [3, 5, 4, 6, 7, 2, 9, 5]),       # the upper limit; S % 4 != 0: the hidden layer runs as the nn.Linear Function
}
_REF = {}


def close(got, want, tol=1e-4, what=""):
    assert rel_err(got, want) < tol, (what, rel_err(got, want))
    assert_close_rel(got, want, rtol=tol, what=what)


def _case(name):
    """The case's fp32 inputs and its fp64 reference (output and gradients), computed once."""
    if name not in _REF:
        B, T, C, widths = CASES[name]
        t = R.case_tensors(B, T, C, widths)
        d = {k: v.double().requires_grad_(k != "dy") for k, v in t.items()}
        y = R.multi_head(d["x"], d["W"], d["b"], d["v"], d["k"], widths)
        y.backward(d["dy"])
        _REF[name] = (t, y.detach(), {k: d[k].grad for k in ("x", "W", "b", "v", "k")})
    return _REF[name]


def _module(t, C, widths):
    from models.audio_models.pooling import MultiHeadAttention
    pool = MultiHeadAttention(C, len(widths), list(widths))
    with torch.no_grad():
        for k in ("W", "b", "v", "k"):
            getattr(pool, k).copy_(t[k])
    return pool.to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_backward_vs_fp64(name):
    from deeplip_amd import autograd as ag
    B, T, C, widths = CASES[name]
    t, ref, gref = _case(name)
    pool = _module(t, C, widths)
    xg = t["x"].to(DEV).requires_grad_()
    y = ag.mh_attentive_stat_pool(xg, pool)
    y.backward(t["dy"].to(DEV))
    torch.cuda.synchronize()
    assert y.shape == (B, len(widths) * 2 * C)
    e_y, e_x = rel_err(y.detach().cpu().numpy(), ref.numpy()), rel_err(xg.grad.cpu().numpy(), gref["x"].numpy())
    print(f"\n{name}: y {e_y:.3e} dx {e_x:.3e}", end="")
    assert e_y < BAR_OUT and e_x < BAR_GRAD
    for k, p in pool.named_parameters():
        got = p.grad.cpu().numpy()
        if k == "k":            # softmax is shift-invariant: d/dk = 0 exactly, rounding noise on both sides (the single-head test's bound)
            print(f" dk {np.abs(got).max():.3e}", end="")
            assert float(np.abs(got).max()) < 1e-5 * float(t["dy"].abs().sum() / B)
        elif T == 1:            # alpha = 1 whatever the scores are: W, b and v have no gradient
            print(f" d{k} {np.abs(got).max():.3e}", end="")
            assert float(gref[k].abs().max()) == 0.0 and float(np.abs(got).max()) <= 1e-5 * float(t["dy"].abs().max())
        else:
            e = rel_err(got, gref[k].numpy())
            print(f" d{k} {e:.3e}", end="")
            assert e < BAR_GRAD, k
    with torch.no_grad():       # the eval-mode path of the same module
        ye = pool.eval().run_ntc(xg.detach())
        yl = pool(xg.detach().permute(0, 2, 1).contiguous())          # the reference layout [B,C,T]
    assert rel_err(ye.cpu().numpy(), ref.numpy()) < BAR_OUT and torch.equal(ye, yl)
    if T == 1:
        assert rel_err(ye[:, C:2 * C].cpu().numpy(), np.full((B, C), np.sqrt(R.EPS))) < 1e-6


def test_one_head_is_the_single_head_kernel():
    """One head against the single-head definition (R.single_head in fp64); AttentiveStatPooling with the same parameters runs the same
    kernels without an offsets array: the same bits."""
    from models.audio_models.pooling import AttentiveStatPooling
    B, T, C, widths = CASES["one-head"]
    t, ref, _ = _case("one-head")
    pool = _module(t, C, widths)
    x = t["x"].to(DEV)
    d = {k: v.double() for k, v in t.items()}
    single = R.single_head(d["x"], d["W"], d["b"], d["v"], d["k"])
    one = AttentiveStatPooling(C, widths[0])
    with torch.no_grad():
        for k in ("W", "b", "v", "k"):
            getattr(one, k).copy_(t[k])
        y = pool.run_ntc(x)
        y1 = one.to(DEV).run_ntc(x, eps=R.EPS)
    assert rel_err(y.cpu().numpy(), single.numpy()) < BAR_OUT
    assert torch.equal(y, y1)


def test_single_head_ragged_rows_without_floor():
    """AttentiveStatPooling.run_ntc(x, lengths) with eps = 0 (the reference's unfloored root) on rows [41, 40, 2, 1] of a [4, 41, 64]
    batch whose padding frames hold NaN and 1e30: every row equals the fp64 restatement of the row alone (a single frame has a zero
    standard deviation on both sides) and is bit-identical to the row run as a batch of one at its own length."""
    from models.audio_models.pooling import AttentiveStatPooling
    B, T, C, H = 4, 41, 64, 16
    lengths = [T, T - 1, 2, 1]
    t = R.case_tensors(B, T, C, [H], seed=9)
    d = {k: v.double() for k, v in t.items()}
    pool = AttentiveStatPooling(C, H)
    with torch.no_grad():
        for k in ("W", "b", "v", "k"):
            getattr(pool, k).copy_(t[k])
    pool = pool.to(DEV).eval()
    x = t["x"].clone()
    for b, L in enumerate(lengths):
        x[b, L:] = float("nan") if b % 2 else 1e30
    with torch.no_grad():
        y = pool.run_ntc(x.to(DEV), torch.tensor(lengths, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all())
        for b, L in enumerate(lengths):
            xr = d["x"][b:b + 1, :L]
            e = torch.relu(xr.matmul(d["W"].t()) + d["b"]).matmul(d["v"]) + d["k"]
            alpha = torch.softmax(e, dim=1)
            m = (alpha * xr).sum(dim=1)
            want = torch.cat([m, torch.sqrt((alpha * xr * xr).sum(dim=1) - m * m)], dim=1)      # pooling.py:103-106
            e_b = rel_err(y[b:b + 1].cpu().numpy(), want.numpy())
            print(f"\nrow {b} (L = {L}): y {e_b:.3e}, smallest std {float(want[0, C:].min()):.3e}", end="")
            assert e_b < BAR_OUT, (b, L)
            alone = pool.run_ntc(t["x"][b:b + 1, :L].contiguous().to(DEV))
            assert torch.equal(alone, y[b:b + 1]), (b, L)


def _launch(x, hidden, t, widths, lens):
    from deeplip_amd import ops
    off = torch.tensor([sum(widths[:i]) for i in range(len(widths) + 1)], dtype=torch.int32, device=DEV)
    alpha = ops.mh_attn_scores(hidden, t["v"].reshape(-1).to(DEV), t["k"].reshape(-1).to(DEV), off, lens)
    return alpha, ops.mh_attn_stat_pool(x, alpha, R.EPS, lens), off


def test_ragged_rows_padding_and_zero_tails():
    """B = 4 with lengths [T, T - 1, 2, 1] at T = 41: every row against the restatement of the row alone at its own length; the same bits
    whatever the padding frames of x and the padding rows of hidden hold; alpha and dx exactly zero behind each row's end."""
    from deeplip_amd import _lib
    from deeplip_amd._lib import check, lib, ptr, stream_handle
    B, T, C, widths = 4, 41, 64, [8, 12, 20, 24]
    n, S = len(widths), sum(widths)
    lengths = [T, T - 1, 2, 1]
    t = R.case_tensors(B, T, C, widths, seed=9)
    d = {k: v.double() for k, v in t.items()}
    lens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    hid = (t["x"].double().matmul(t["W"].double().t()) + t["b"].double()).float()
    outs = []
    for fill in (0.0, 1e30, float("nan")):
        x, h = t["x"].clone(), hid.clone()
        for b, L in enumerate(lengths):
            x[b, L:] = fill
            h[b, L:] = fill
        xg, hg = x.to(DEV), h.to(DEV)
        alpha, y, off = _launch(xg, hg, t, widths, lens)
        dx, dh, rde = torch.empty_like(xg), torch.empty_like(hg), torch.empty_like(hg)
        de, dek = torch.empty((B, n, T), device=DEV), torch.empty((B, n), device=DEV)
        check(lib().dlip_mh_attn_stat_pool_bwd_f32(ptr(xg), ptr(hg), ptr(t["v"].reshape(-1).to(DEV)), ptr(off), ptr(alpha), ptr(y),
                                                   ptr(t["dy"].to(DEV)), ptr(lens), 0, R.EPS, ptr(dx), ptr(dh), ptr(rde), ptr(de), ptr(dek),
                                                   B, T, C, S, n, stream_handle()), "dlip_mh_attn_stat_pool_bwd_f32")
        torch.cuda.synchronize()
        outs.append([o.cpu() for o in (y, alpha, dx, dh, rde, de, dek)])
    for o in outs[1:]:
        for a, b_ in zip(outs[0], o):
            assert torch.equal(a, b_)
    y, alpha, dx, dh, rde, de, dek = outs[2]
    assert all(bool(torch.isfinite(o).all()) for o in outs[2])
    for b, L in enumerate(lengths):
        xr = d["x"][b:b + 1, :L].clone().requires_grad_()
        alone = R.multi_head(xr, d["W"], d["b"], d["v"], d["k"], widths)
        assert rel_err(y[b:b + 1].numpy(), alone.detach().numpy()) < BAR_OUT, (b, L)
        assert float(alpha[b, :, L:].abs().max() if L < T else 0.0) == 0.0 and float(dx[b, L:].abs().max() if L < T else 0.0) == 0.0
        assert float(dh[b, L:].abs().max() if L < T else 0.0) == 0.0 and float(de[b, :, L:].abs().max() if L < T else 0.0) == 0.0
        assert np.allclose(alpha[b, :, :L].double().sum(dim=1).numpy(), 1.0, atol=1e-6)
        # the direct path of dx (hidden held fixed) against autograd of the row alone: dx_total - dhidden W
        alone.backward(d["dy"][b:b + 1])
        total = dx[b, :L].double() + dh[b, :L].double().matmul(d["W"])
        assert rel_err(total.numpy(), xr.grad[0].numpy()) < BAR_GRAD, (b, L)
    # len_add: lengths counted in input frames, as the TDNN encoders pass them
    _, y2, _ = _launch(t["x"].to(DEV), hid.to(DEV), t, widths, lens + 3)
    from deeplip_amd import ops
    off = torch.tensor([0, 8, 20, 40, 64], dtype=torch.int32, device=DEV)
    a3 = ops.mh_attn_scores(hid.to(DEV), t["v"].reshape(-1).to(DEV), t["k"].reshape(-1).to(DEV), off, lens + 3, -3)
    y3 = ops.mh_attn_stat_pool(t["x"].to(DEV), a3, R.EPS, lens + 3, -3)
    torch.cuda.synchronize()
    assert torch.equal(y3.cpu(), outs[0][0]) and not torch.equal(y2.cpu(), outs[0][0])


def test_limits_are_refused_without_a_launch():
    """DLIP_EINVAL (-1) from the entry points themselves; the output buffers keep their bytes."""
    from deeplip_amd._lib import lib, ptr, stream_handle
    B, T, C, S = 2, 6, 8, 16
    x, hid = torch.zeros(B, T, C, device=DEV), torch.zeros(B, T, S, device=DEV)
    v, k = torch.zeros(S, device=DEV), torch.zeros(8, device=DEV)
    off = torch.arange(0, 10, dtype=torch.int32, device=DEV)
    alpha = torch.full((B, 8, T), 7.0, device=DEV)
    y = torch.full((B, 8 * 2 * C), 7.0, device=DEV)
    big_x, big_y = torch.zeros(1, 2, 1708, device=DEV), torch.full((1, 8 * 2 * 1708), 7.0, device=DEV)
    big_alpha = torch.zeros(1, 8, 2, device=DEV)
    L = lib()
    for n in (0, 9, -1):
        assert L.dlip_mh_attn_scores_f32(ptr(hid), ptr(v), ptr(k), ptr(off), None, 0, ptr(alpha), B, T, S, n, stream_handle()) == -1
        assert L.dlip_mh_attn_stat_pool_f32(ptr(x), ptr(alpha), None, 0, 1e-5, ptr(y), B, T, C, n, stream_handle()) == -1
    assert L.dlip_mh_attn_scores_f32(ptr(hid), ptr(v), ptr(k), ptr(off), None, 0, ptr(alpha), B, 16001, S, 2, stream_handle()) == -1
    assert L.dlip_mh_attn_stat_pool_f32(ptr(x), ptr(alpha), None, 0, 1e-5, ptr(y), B, 16001, C, 2, stream_handle()) == -1
    assert L.dlip_mh_attn_stat_pool_f32(ptr(big_x), ptr(big_alpha), None, 0, 1e-5, ptr(big_y), 1, 2, 1708, 8, stream_handle()) == -1   # LDS
    assert L.dlip_mh_attn_stat_pool_f32(ptr(x), ptr(alpha), None, 0, 1e-5, ptr(y), B, T, 6, 2, stream_handle()) == -1                  # C % 4
    for bad in (-1e-5, float("nan")):       # eps < 0 (0 is the unfloored root since ABI 67)
        assert L.dlip_mh_attn_stat_pool_f32(ptr(x), ptr(alpha), None, 0, bad, ptr(y), B, T, C, 2, stream_handle()) == -1
    assert L.dlip_mh_attn_scores_f32(ptr(hid), ptr(v), ptr(k), None, None, 0, ptr(alpha), B, T, S, 2, stream_handle()) == -1            # no head_off, n = 2
    dx, dh, rde = torch.full_like(x, 7.0), torch.full_like(hid, 7.0), torch.full_like(hid, 7.0)
    de, dek = torch.full((B, 8, T), 7.0, device=DEV), torch.full((B, 8), 7.0, device=DEV)
    for n, TT in ((0, T), (9, T), (2, 16001)):
        assert L.dlip_mh_attn_stat_pool_bwd_f32(ptr(x), ptr(hid), ptr(v), ptr(off), ptr(alpha), ptr(y), ptr(y), None, 0, 1e-5, ptr(dx), ptr(dh),
                                                ptr(rde), ptr(de), ptr(dek), B, TT, C, S, n, stream_handle()) == -1
    assert L.dlip_mh_attn_stat_pool_bwd_f32(ptr(big_x), ptr(hid), ptr(v), ptr(off), ptr(big_alpha), ptr(big_y), ptr(big_y), None, 0, 1e-5,
                                            ptr(big_x), ptr(dh), ptr(rde), ptr(de), ptr(dek), 1, 2, 1708, S, 8, stream_handle()) == -1
    assert L.dlip_mh_attn_stat_pool_bwd_f32(ptr(x), ptr(hid), ptr(v), None, ptr(alpha), ptr(y), ptr(y), None, 0, 1e-5, ptr(dx), ptr(dh),
                                            ptr(rde), ptr(de), ptr(dek), B, T, C, S, 2, stream_handle()) == -1                       # no head_off, n = 2
    assert L.dlip_mh_attn_stat_pool_bwd_f32(ptr(x), ptr(hid), ptr(v), ptr(off), ptr(alpha), ptr(y), ptr(y), None, 0, -1e-5, ptr(dx), ptr(dh),
                                            ptr(rde), ptr(de), ptr(dek), B, T, C, S, 2, stream_handle()) == -1                       # eps < 0
    torch.cuda.synchronize()
    for o in (alpha, y, big_y, dx, dh, rde, de, dek):
        assert bool((o == 7.0).all())
    from models.audio_models.pooling import MultiHeadAttention
    with pytest.raises(ValueError):
        MultiHeadAttention(1708, 8, 4).to(DEV).run_ntc(big_x)


# ------------------------------------------------------------------------------------------ the TDNN encoder
HEADS = [8, 12]
TD_CTX = [[-1, 0, 1], [0], [0]]
TD = {"input_dim": 24, "hidden_dim": [32, 32, 64], "context": TD_CTX, "tdnn_layers": 3, "embedding_dim": 32,
      "pooling": "multi_head_attention", "attention_heads": 2, "attention_hidden_size": HEADS, "bn_first": True}


@pytest.fixture(params=["f32", "f16x3"])
def mode(request):
    from deeplip_amd import packing
    packing.set_precision(request.param)
    yield request.param
    packing.set_precision("f32")


def _tdnn(prefix="mh.tdnn."):
    from models.audio_models.tdnn import SpeakerEmbNet
    net = SpeakerEmbNet({"arch": "tdnn", "tdnn": dict(TD)})
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix=prefix)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV), O.to_torch_sd(sd)


def tdnn_ref(p, x, forward=False):
    """The whole net restated: oracle TDNN stack -> the multi-head restatement -> fc1 -> BN / LeakyReLU -> fc2 (-> bn2 / LeakyReLU)."""
    h = O.speaker_tdnn_stack(p, x, TD_CTX)                                        # [B,C,T']
    pooled = R.multi_head(h.permute(0, 2, 1), p["pooling.W"], p["pooling.b"], p["pooling.v"], p["pooling.k"], HEADS)
    x_a = F.linear(pooled, p["fc1.weight"], p["fc1.bias"])
    xv = F.linear(F.leaky_relu(O._bn(x_a, p, "bn1"), 0.2), p["fc2.weight"], p["fc2.bias"])
    return (F.leaky_relu(O._bn(xv, p, "bn2"), 0.2) if forward else xv), x_a


def _f64(sd):
    return {k: (v.double().clone() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}


def test_tdnn_eval_vs_fp64_restatement(mode):
    from deeplip_amd import _lib
    net, sd = _tdnn()
    net.eval()
    x = torch.from_numpy(wg.audio_input(3, 24, 40, key="mh.tdnn.x"))
    taps = {}
    xv, x_a = net.extract_embedding(x.to(DEV))
    xv_t, _ = net.extract_embedding(x.to(DEV), taps=taps)
    _lib.check_range(sync=True)
    with torch.no_grad():
        rv, ra = tdnn_ref(_f64(sd), x.double())
    assert xv.shape == (3, 32) and torch.equal(xv, xv_t) and taps["pooled"].shape == (3, 2 * 2 * 64)
    close(xv.cpu().numpy(), rv.numpy(), what=f"xv {mode}")
    close(x_a.cpu().numpy(), ra.numpy(), what=f"x_a {mode}")


def test_tdnn_ragged_batch_equals_the_utterance_loop(mode):
    net, sd = _tdnn()
    net.eval()
    lengths = [40, 17, 29, 5]                                                   # 5 - 2 consumed frames = 3 pooled frames
    x = torch.from_numpy(wg.audio_input(4, 24, 40, key="mh.tdnn.ragged"))
    items = [x[b:b + 1, :, :L].clone() for b, L in enumerate(lengths)]
    for b, L in enumerate(lengths):
        x[b, :, L:] = 50.0 * (b + 1)
    xv, _ = net.extract_embedding(x.to(DEV), lengths=lengths)
    xv_d, _ = net.extract_embedding(x.to(DEV), lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(xv, xv_d)
    with torch.no_grad():
        for b, it in enumerate(items):
            one, _ = net.extract_embedding(it.to(DEV))
            close(xv[b:b + 1].cpu().numpy(), one.cpu().numpy(), what=f"row {b} against the engine alone")
            close(xv[b:b + 1].cpu().numpy(), tdnn_ref(_f64(sd), it.double())[0].numpy(), what=f"row {b} against fp64")


def _train_step_vs_fp64(net, sd, x, restate, E):
    """loss = (net(x) * g).sum() under model.train(): the loss and every parameter's gradient against fp64 autograd of ``restate``.  A
    gradient that is exactly zero in fp64 (a bias in front of a batch-statistics BatchNorm, pooling.k under the softmax) is held to 1e-6
    absolute with g ~ N(0,1) / (B E), the weight of a mean over the embedding (tests/test_audio_resnet_heads_gpu.py states why)."""
    net.train()
    B = x.shape[0]
    g = torch.randn((B, E), generator=torch.Generator().manual_seed(48)) / (B * E)
    out = net(x.to(DEV))
    loss = (out * g.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    names = [k for k, _ in net.named_parameters()]
    p = _f64(sd)
    for k in names:
        p[k].requires_grad_(True)
    with O.bn_training():
        ref = restate(p, x.double())
    rl = (ref * g.double()).sum()
    rl.backward()
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < BAR_GRAD
    assert abs(float(loss.detach()) - float(rl.detach())) < BAR_GRAD * float((ref.detach() * g.double()).abs().sum())     # (a sum of cancelling terms)
    worst = (0.0, "")
    for k, v in net.named_parameters():
        got, want = v.grad.detach().cpu().double(), p[k].grad
        assert bool(torch.isfinite(got).all()), k
        scale = float(want.abs().max())
        if scale < 1e-9:
            print(f"\nexactly-zero gradient {k}: engine {float(got.abs().max()):.3e}", end="")
            assert float(got.abs().max()) < 1e-6, k
            continue
        e = float((got - want).abs().max()) / scale
        worst = max(worst, (e, k))
        assert e < BAR_GRAD, (k, e)
    print(f"\nworst gradient {worst[1]} {worst[0]:.3e}", end="")


def test_tdnn_training_step_vs_fp64_autograd():
    net, sd = _tdnn("mh.tdnn.train.")
    x = torch.from_numpy(wg.audio_input(4, 24, 40, key="mh.tdnn.train.x"))
    _train_step_vs_fp64(net, sd, x, lambda p, xx: tdnn_ref(p, xx, forward=True)[0], 32)


# ------------------------------------------------------------------------------------------ the ResNet encoder
RN_HIDDEN, RN_LAYERS, RN_E = (16, 32), (1, 1), 16                                # the "k1" geometry of tests/test_audio_resnet_heads_gpu.py
RN_HEADS = [8, 8]


def _resnet(prefix="mh.resnet."):
    from models.resnet import SpeakerEmbNet
    net = SpeakerEmbNet({"arch": "resnet", "resnet": {"input_dim": 1, "hidden_dim": list(RN_HIDDEN), "residual_block_layers": list(RN_LAYERS),
                                                     "fc_layers": 2, "embedding_dim": RN_E, "pooling": "multi_head_attention", "feat_dim": 8,
                                                     "attention_heads": 2, "attention_hidden_size": 8}})
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix=prefix)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV), O.to_torch_sd(sd)


def resnet_ref(p, x):
    y = F.relu(O._bn(F.conv2d(x, p["conv1.weight"], None, padding=1), p, "bn1"))
    for i, n in enumerate(RN_LAYERS):
        for j in range(n):
            y = O.basic_block(p, f"layers.{i}.{j}", y, 2 if (i > 0 and j == 0) else 1, "relu")
    m = y.permute(0, 3, 2, 1)                                                   # [B,W,H,C]: the D-vector of a frame is (h, c) flattened
    pooled = R.multi_head(m.reshape(m.shape[0], m.shape[1], -1), p["pooling.W"], p["pooling.b"], p["pooling.v"], p["pooling.k"], RN_HEADS)
    x_a = F.linear(pooled, p["fc1.weight"], p["fc1.bias"])
    return F.linear(F.relu(O._bn(x_a, p, "fc1_bn")), p["fc2.weight"], p["fc2.bias"]), x_a


def test_resnet_eval_and_ragged(mode):
    from deeplip_amd import _lib
    net, sd = _resnet()
    net.eval()
    T = 12
    x = torch.randn((3, 1, 8, T), generator=torch.Generator().manual_seed(41))
    xv, x_a = net.extract_embedding(x.to(DEV))
    _lib.check_range(sync=True)
    with torch.no_grad():
        rv, ra = resnet_ref(_f64(sd), x.double())
    assert xv.shape == (3, RN_E)
    assert rel_err(xv.cpu().numpy(), rv.numpy()) < BAR_GRAD and rel_err(x_a.cpu().numpy(), ra.numpy()) < BAR_GRAD
    lengths = [T, 1, 7]
    items = [x[b:b + 1, :, :, :L].clone() for b, L in enumerate(lengths)]
    for b, L in enumerate(lengths):
        x[b, :, :, L:] = 1e4 * (b + 1)
    rg, _ = net.extract_embedding(x.to(DEV), lengths=lengths)
    rg_d, _ = net.extract_embedding(x.to(DEV), lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    _lib.check_range(sync=True)
    assert bool(torch.isfinite(rg).all()) and torch.equal(rg, rg_d)
    for b, it in enumerate(items):
        one, _ = net.extract_embedding(it.to(DEV))
        _lib.check_range(sync=True)
        assert rel_err(rg[b:b + 1].cpu().numpy(), one.cpu().numpy()) < 1e-6, (b, lengths[b])


def test_resnet_training_step_vs_fp64_autograd():
    net, sd = _resnet("mh.resnet.train.")
    x = torch.randn((3, 1, 8, 9), generator=torch.Generator().manual_seed(47))
    _train_step_vs_fp64(net, sd, x, lambda p, xx: resnet_ref(p, xx)[0], RN_E)


# ------------------------------------------------------------------------------------------ recorded steps, the trainer
def test_recorded_step_equals_eager():
    """Two steps through a TrainStepGraph (one eager, one recorded and replayed) against two eager steps from the same state: the same
    losses, parameters and BatchNorm buffers, bit for bit."""
    from deeplip_amd.train_plan import TrainStepGraph

    def run(graph):
        net, _ = _tdnn("mh.tdnn.plan.")
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(3e-4, device=DEV), weight_decay=1e-4, capturable=True, fused=True)
        gw = torch.randn((4, 32), generator=torch.Generator().manual_seed(52)).to(DEV)

        def one(xb):
            opt.zero_grad(set_to_none=True)
            l = (net(xb) * gw).sum()
            l.backward()
            opt.step()
            return l

        plan = TrainStepGraph(one, eager_steps=1) if graph else None
        losses = []
        for i in range(3):
            xb = torch.from_numpy(wg.audio_input(4, 24, 40, key=f"mh.tdnn.plan.x{i}")).to(DEV)
            l = plan.step(xb) if graph else one(xb)
            losses.append(float(l.detach()))
        if graph:
            plan.finish()
            assert plan.recorded
        torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}

    le, se = run(False)
    lg, sg = run(True)
    assert le == lg and all(np.isfinite(le))
    for k in se:
        assert torch.equal(se[k], sg[k]), k


def test_train_audio_trains_and_extracts_with_the_option(tmp_path, monkeypatch):
    """train_audio.Trainer with `pooling: multi_head_attention`: one synthetic epoch through the recorded step, then the ragged test list
    through the RaggedExtractor."""
    import train_audio
    monkeypatch.chdir(tmp_path)
    tr = train_audio.Trainer(overrides={"model.arch": "tdnn", "model.tdnn.pooling": "multi_head_attention", "model.tdnn.attention_heads": 2,
                                        "model.tdnn.attention_hidden_size": [8, 12], "model.tdnn.hidden_dim": [32, 32, 32, 32, 64],
                                        "model.tdnn.embedding_dim": 32, "data.test_speakers": 3, "data.test_utt_per_spk": 2, "data.trials": 30,
                                        "data.trial_targets": 6, "data.audio_frames": 60, "data.n_spk": 5, "data.utt_per_spk": 2,
                                        "data.test_audio_frames": [40, 90], "train.bs": 4, "train.epoch": 1})
    try:
        assert tr.model.fc1.weight.shape == (32, 2 * 2 * 64)
        before = {k: v.detach().clone() for k, v in tr.model.named_parameters()}
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        assert np.isfinite(loss) and tr.last_epoch_stats["steps"] == 2 and tr.last_epoch_stats["step_mode"] == "graph"
        assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
        for k in ("pooling.W", "pooling.b", "pooling.v", "tdnn.0.context_layer.weight", "fc1.weight"):
            assert not torch.equal(before[k], dict(tr.model.named_parameters())[k].detach()), k
        table = tr.extract_test_xv(batch=4)
        assert table.emb.shape == (6, 32) and bool(torch.isfinite(table.emb).all())
    finally:
        tr.close()


def test_train_fusion_av_test_from_waveforms_with_the_option(tmp_path, monkeypatch):
    """train_fusion's av_test from waveforms (front-end + speech encoder in one recorded plan per padded shape) with the option on the
    shipped E-TDNN: every x-vector of the ragged extraction equals front-end -> encoder of the utterance alone (1e-6, the bar of
    tests/test_frontend_ragged_gpu.py's entry-point tests)."""
    import train_fusion
    monkeypatch.chdir(tmp_path)
    small = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.test_speakers": 3, "data.test_utt_per_spk": 2, "data.trials": 30,
             "data.trial_targets": 6, "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120],
             "data.test_video_frames": [5, 12], "data.test_clips_per_utt": 1, "test.batch": 4, "test.write_store": False,
             "data.python_data_config.test_from_waves": True, "model.audio_config.etdnn.pooling": "multi_head_attention",
             "model.audio_config.etdnn.attention_heads": 2, "model.audio_config.etdnn.attention_hidden_size": [8, 12]}
    tr = train_fusion.Trainer("av_test", overrides=small)
    try:
        assert tr.model_audio.fc1.weight.shape == (512, 2 * 2 * 1500)
        ds = tr.lomgridtestset
        tr.extract_test_xv_lomgrid()
        fe = tr._test_frontend("etdnn")
        xa = tr.lomgrid_tables[1].emb
        assert bool(torch.isfinite(xa).all())
        for i in range(len(ds)):
            want = tr.model_audio.extract_embedding(fe(torch.from_numpy(ds.wave_item(i)[None]).to(tr.device)))[0]
            assert rel_err(xa[i:i + 1].cpu().numpy(), want.cpu().numpy()) < 1e-6, i
    finally:
        tr.close()
