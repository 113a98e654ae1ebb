"""Statistics and attentive pooling + the two-layer head of the ResNet speech encoder (`arch: resnet`; -m gpu).  DESIGN.md 4b defines
them; the fp64 restatement below composes oracle.basic_block / _bn / bn_training with those formulas.

Bars (the project's own: tests/test_train_f32_gpu.py): kernel outputs element by element, assert_close_rel at 2e-5; gradients that pass
a linear op and model embeddings rel_err < 1e-4; whole-network gradients the fp32 noise floor of the restatement itself (the network is
piecewise linear: tests/test_train_video_gpu.py::test_full_size_training_step_loss_and_gradients_vs_fp64_oracle); copies, a ragged row
against the utterance alone in exact arithmetic's own bar 1e-6 (tests/test_audio_resnet_ragged_gpu.py), recorded steps bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_rel, rel_err
from deeplip_amd import weightgen as wg
from oracle import deeplip_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5
BAR_OUT, BAR_GRAD = 2e-5, 1e-4
MAPS = [(1, 2, 4), (3, 5, 32), (2, 9, 12)]            # (H, W, C); N = 3


@pytest.fixture(params=["f32", "f16x3"])
def mode(request):
    from deeplip_amd import packing
    packing.set_precision(request.param)
    yield request.param
    packing.set_precision("f32")


def _valid(L, shift, W):
    return ((min(max(L, 1), W << shift) - 1) >> shift) + 1


# ------------------------------------------------------------------------------------------ the fp64 restatement
def ref_statpool(m, wb=None):
    """m [N,H,W,C] -> [N, 2 H C]: per feature j = h C + c the mean and sqrt(unbiased variance + eps) over the first wb[n] frames."""
    N, H, W, C = m.shape
    rows = []
    for n in range(N):
        v = m[n, :, :(W if wb is None else wb[n])]                  # [H,Wb,C]
        mean = v.mean(dim=1)
        var = ((v - mean[:, None]) ** 2).sum(dim=1) / (v.shape[1] - 1)
        rows.append(torch.cat([mean.reshape(-1), torch.sqrt(var + EPS).reshape(-1)]))
    return torch.stack(rows)


def ref_attentive(m, W_, b, v, k, wb=None):
    """m [N,H,W,C]; W_ [Hd,D], b [1,Hd], v [Hd,1], k [1,1] -> [N, 2 D] over each row's first wb[n] frames (oracle.attentive_stat_pooling with
    the floored standard deviation)."""
    N, H, W, C = m.shape
    rows = []
    for n in range(N):
        x = m[n, :, :(W if wb is None else wb[n])].permute(1, 0, 2).reshape(-1, H * C)      # [Wb, D]
        e = F.relu(x.matmul(W_.t()) + b).matmul(v) + k                                     # [Wb, 1]
        alpha = F.softmax(e, dim=0)
        mean = (alpha * x).sum(dim=0)
        std = torch.sqrt(torch.clamp((alpha * x * x).sum(dim=0) - mean * mean, min=0.0) + EPS)
        rows.append(torch.cat([mean, std]))
    return torch.stack(rows)


def ref_map(sd, x, layers):
    """[B,1,F,T] -> the trunk's last tensor, channels-last [B,H,W,C] (oracle.audio_resnet_embedding's trunk; honours bn_training())."""
    y = F.relu(O._bn(F.conv2d(x, sd["conv1.weight"], None, padding=1), sd, "bn1"))
    for i, n in enumerate(layers):
        for j in range(n):
            y = O.basic_block(sd, f"layers.{i}.{j}", y, 2 if (i > 0 and j == 0) else 1, "relu")
    return y.permute(0, 2, 3, 1)


def ref_embedding(sd, x, layers, pooling, fc_layers, taps=None):
    m = ref_map(sd, x, layers)
    if taps is not None:
        taps["map"] = m
    if pooling == "statistic":
        p = ref_statpool(m)
    else:
        p = ref_attentive(m, sd["pooling.W"], sd["pooling.b"], sd["pooling.v"], sd["pooling.k"])
    if fc_layers == 1:
        e = F.linear(p, sd["fc.weight"], sd["fc.bias"])
        return e, e
    x_a = F.linear(p, sd["fc1.weight"], sd["fc1.bias"])
    return F.linear(F.relu(O._bn(x_a, sd, "fc1_bn")), sd["fc2.weight"], sd["fc2.bias"]), x_a


# ------------------------------------------------------------------------------------------ kernels: statistics pooling
def _planted_map(shape, seed):
    """randn with one all-zero feature (h 0, c 1) and one constant feature (last h, c 2)."""
    H, W, C = shape
    x = torch.randn((3, H, W, C), generator=torch.Generator().manual_seed(seed))
    x[:, 0, :, 1] = 0.0
    x[:, H - 1, :, 2] = 0.75
    return x


def _length_cases(W):
    """(shift, input lengths of the three rows): no stage in front with Wb = 2, W and one in between; behind 1 and 2 stride-2 stages the
    lengths that give Wb = 2 and Wb = W, and one past the end (clamped)."""
    cases = [(0, [2, W, (W + 2) // 2])]
    for s in (1, 2):
        cases.append((s, [(1 << s) + 1, W << s, (W << s) + 3]))
    return cases


@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_statpool_forward_vs_fp64(shape):
    from deeplip_amd import ops
    H, W, C = shape
    x = _planted_map(shape, 11)
    got = ops.statpool_nhwc(x.to(DEV), None, 0, EPS).cpu()
    ref = ref_statpool(x.double())
    assert got.shape == (3, 2 * H * C)
    assert_close_rel(got.numpy(), ref.numpy(), rtol=BAR_OUT, what=f"statpool {shape}")
    D = H * C
    assert float(got[:, 1].abs().max()) == 0.0                                               # the all-zero feature: mean 0 ...
    assert_close_rel(got[:, D + 1].numpy(), np.full(3, np.sqrt(EPS)), rtol=BAR_OUT)          # ... std sqrt(eps)
    j = (H - 1) * C + 2
    assert_close_rel(got[:, j].numpy(), np.full(3, 0.75), rtol=BAR_OUT)
    assert_close_rel(got[:, D + j].numpy(), np.full(3, np.sqrt(EPS)), rtol=BAR_OUT)
    for shift, lens in _length_cases(W):
        wb = [_valid(L, shift, W) for L in lens]
        assert 2 in wb and W in wb
        xg = x.clone()
        for n in range(3):
            xg[n, :, wb[n]:] = 1e30                                                          # the padding must not reach the output
        got = ops.statpool_nhwc(xg.to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), shift, EPS).cpu()
        assert_close_rel(got.numpy(), ref_statpool(x.double(), wb).numpy(), rtol=BAR_OUT, what=f"statpool {shape} shift {shift} lens {lens}")


def test_statpool_refuses_a_single_frame():
    from deeplip_amd import ops
    with pytest.raises(ValueError):
        ops.statpool_nhwc(torch.zeros(3, 2, 1, 4, device=DEV))
    with pytest.raises(ValueError):
        ops.statpool_nhwc(torch.zeros(3, 2, 5, 6, device=DEV))                               # C % 4


@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_statpool_backward_vs_fp64_autograd(shape):
    from deeplip_amd import autograd as ag
    H, W, C = shape
    x = _planted_map(shape, 13)
    dy = torch.randn((3, 2 * H * C), generator=torch.Generator().manual_seed(14))
    xr = x.double().requires_grad_()
    ref_statpool(xr).backward(dy.double())
    xg = x.to(DEV).requires_grad_()
    y = ag.statpool_nhwc(xg, EPS)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    dx = xg.grad.cpu()
    assert bool(torch.isfinite(dx).all())                                                    # the constant features included
    assert_close_rel(dx.numpy(), xr.grad.numpy(), rtol=BAR_OUT, what=f"statpool dx {shape}")


@pytest.mark.parametrize("shape", [(3, 5, 4), (2, 7, 32)], ids=lambda s: "x".join(map(str, s)))
def test_swap_axes_is_permute_bit_for_bit(shape):
    from deeplip_amd import autograd as ag, ops
    H, W, C = shape
    x = torch.randn((3, H, W, C), generator=torch.Generator().manual_seed(21)).to(DEV)
    y = ops.swap_axes_nhwc(x)
    assert y.shape == (3, W, H, C) and torch.equal(y, x.permute(0, 2, 1, 3).contiguous())
    assert torch.equal(ops.swap_axes_nhwc(y), x)                                             # the other direction: the same kernel
    xg = x.clone().requires_grad_()
    dy = torch.randn((3, W, H, C), generator=torch.Generator().manual_seed(22)).to(DEV)
    ag.swap_axes_nhwc(xg).backward(dy)
    assert torch.equal(xg.grad, dy.permute(0, 2, 1, 3).contiguous())


def test_time_valid_lengths_on_the_device():
    from deeplip_amd import ops
    for shift in (0, 1, 2):
        lens = [0, 1, 2, 3, 5, 8, 9, 23, 24, 25, 1000]
        got = ops.time_valid_lengths(torch.tensor(lens, dtype=torch.int32, device=DEV), shift, 6).cpu().tolist()
        assert got == [_valid(L, shift, 6) for L in lens]


# ------------------------------------------------------------------------------------------ kernels: the attentive route
def _attentive_case():
    from models.audio_models.pooling import AttentiveStatPooling
    N, H, W, C, Hd = 3, 2, 6, 8, 5
    g = torch.Generator().manual_seed(31)
    pool = AttentiveStatPooling(H * C, Hd)
    with torch.no_grad():
        pool.W.copy_(torch.randn(Hd, H * C, generator=g) / np.sqrt(H * C)); pool.b.copy_(torch.randn(1, Hd, generator=g) * 0.1)
        pool.v.copy_(torch.randn(Hd, 1, generator=g) * 0.5); pool.k.copy_(torch.randn(1, 1, generator=g) * 0.1)
    x = torch.relu(torch.randn((N, H, W, C), generator=g) + 0.5)                             # post-ReLU, as the trunk's map
    x[:, 1, :, 3] = 0.0                                                                      # one all-zero feature
    return pool, x, torch.randn((N, 2 * H * C), generator=g)


def test_attentive_route_forward_and_gradients_vs_fp64_autograd():
    from deeplip_amd.audio_resnet import attentive_pool_nhwc, attentive_pool_nhwc_train
    pool, x, dy = _attentive_case()
    sd = {k: v.detach().double().clone().requires_grad_() for k, v in pool.named_parameters()}
    xr = x.double().requires_grad_()
    ref = ref_attentive(xr, sd["W"], sd["b"], sd["v"], sd["k"])
    ref.backward(dy.double())
    pool = pool.to(DEV)
    xg = x.to(DEV).requires_grad_()
    y = attentive_pool_nhwc_train(xg, pool)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert_close_rel(y.detach().cpu().numpy(), ref.detach().numpy(), rtol=BAR_OUT, what="attentive forward (train)")
    with torch.no_grad():
        assert_close_rel(attentive_pool_nhwc(xg.detach(), pool).cpu().numpy(), ref.detach().numpy(), rtol=BAR_OUT, what="attentive forward (eval)")
    assert bool(torch.isfinite(xg.grad).all()) and all(bool(torch.isfinite(p.grad).all()) for p in pool.parameters())
    e = rel_err(xg.grad.cpu().numpy(), xr.grad.numpy())
    print(f"\nattentive dx rel err {e:.3e}", end="")
    assert e < BAR_GRAD
    for k, p in pool.named_parameters():
        if k == "k":            # softmax is shift-invariant: d/dk = 0 exactly, rounding noise on both sides (test_train_audio_gpu.py's bound)
            assert float(p.grad.abs().max()) < 1e-5 * float(dy.abs().sum() / dy.shape[0])
            continue
        e = rel_err(p.grad.cpu().numpy(), sd[k].grad.numpy())
        print(f"\nattentive d{k} rel err {e:.3e}", end="")
        assert e < BAR_GRAD, k


def test_attentive_route_ragged_forward():
    from deeplip_amd.audio_resnet import attentive_pool_nhwc
    pool, x, _ = _attentive_case()
    sd = {k: v.detach().double() for k, v in pool.named_parameters()}
    pool = pool.to(DEV)
    for shift, lens in ((0, [1, 3, 6]), (1, [1, 5, 12]), (2, [12, 24, 4])):
        wb = [_valid(L, shift, 6) for L in lens]
        assert sorted(wb) == [1, 3, 6]
        xg = x.clone()
        for n in range(3):
            xg[n, :, wb[n]:] = 1e30
        with torch.no_grad():
            got = attentive_pool_nhwc(xg.to(DEV), pool, torch.tensor(lens, dtype=torch.int32, device=DEV), shift).cpu()
        ref = ref_attentive(x.double(), sd["W"], sd["b"], sd["v"], sd["k"], wb)
        assert_close_rel(got.numpy(), ref.numpy(), rtol=BAR_OUT, what=f"attentive ragged shift {shift}")


# ------------------------------------------------------------------------------------------ the model
NETS = {"k1": ((16, 32), (1, 1)), "k2": ((8, 16, 32), (1, 1, 1))}
E = 16


def _net(which, pooling, fc_layers, feat_dim):
    from models.resnet import SpeakerEmbNet
    hidden, layers = NETS[which]
    net = SpeakerEmbNet({"arch": "resnet", "resnet": {"input_dim": 1, "hidden_dim": list(hidden), "residual_block_layers": list(layers),
                                                     "fc_layers": fc_layers, "embedding_dim": E, "pooling": pooling, "feat_dim": feat_dim,
                                                     "attention_hidden_size": 8}})
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix=f"aresnet.heads.{which}.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV), O.to_torch_sd(sd), layers


def _features(B, Fd, T, seed):
    return torch.randn((B, 1, Fd, T), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("fc_layers", [1, 2])
@pytest.mark.parametrize("pooling", ["statistic", "attentive_statistic"])
@pytest.mark.parametrize("which,Fd,T", [("k1", 8, 9), ("k1", 9, 12), ("k2", 9, 9), ("k2", 8, 12)])
def test_embedding_vs_fp64_restatement(which, Fd, T, pooling, fc_layers, mode):
    from deeplip_amd import _lib
    net, sd, layers = _net(which, pooling, fc_layers, Fd)
    net.eval()
    x = _features(3, Fd, T, 41)
    xv, x_a = net.extract_embedding(x.to(DEV))
    _lib.check_range(sync=True)
    with torch.no_grad():
        rv, ra = ref_embedding({k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}, x.double(), layers, pooling, fc_layers)
    assert xv.shape == (3, E) and x_a.shape == (3, E) and ((xv is x_a) == (fc_layers == 1))
    ev, ea = rel_err(xv.cpu().numpy(), rv.numpy()), rel_err(x_a.cpu().numpy(), ra.numpy())
    print(f"\n{which} F={Fd} T={T} {pooling} fc{fc_layers} {mode}: xv {ev:.3e} x_a {ea:.3e}", end="")
    assert ev < BAR_GRAD and ea < BAR_GRAD
    net2 = net.forward(x.to(DEV))
    assert torch.equal(net2, xv)


@pytest.mark.parametrize("pooling", ["statistic", "attentive_statistic"])
@pytest.mark.parametrize("which,Fd", [("k1", 8), ("k2", 9)])
def test_ragged_rows_equal_the_utterance_alone(which, Fd, pooling, mode):
    """Row b of a padded batch with lengths == that utterance run alone (1e-6, the ragged-rows bar of the average pooling), the shortest
    legal length included, a device length vector the same bits as the host list, garbage in the padding."""
    from deeplip_amd import _lib
    net, _, _ = _net(which, pooling, 2, Fd)
    net.eval()
    T = 12
    lengths = [T, net.min_frames(), 7]
    x = _features(3, Fd, T, 43)
    items = [x[b:b + 1, :, :, :L].clone() for b, L in enumerate(lengths)]
    for b, L in enumerate(lengths):
        x[b, :, :, L:] = 1e4 * (b + 1)
    xv, x_a = net.extract_embedding(x.to(DEV), lengths=lengths)
    xv_d, x_a_d = net.extract_embedding(x.to(DEV), lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV))
    _lib.check_range(sync=True)
    assert bool(torch.isfinite(xv).all()) and torch.equal(xv, xv_d) and torch.equal(x_a, x_a_d)
    for b, it in enumerate(items):
        one_v, one_a = net.extract_embedding(it.to(DEV))
        _lib.check_range(sync=True)
        ev, ea = rel_err(xv[b:b + 1].cpu().numpy(), one_v.cpu().numpy()), rel_err(x_a[b:b + 1].cpu().numpy(), one_a.cpu().numpy())
        print(f"\nrow {b} (L={lengths[b]}): xv {ev:.3e} x_a {ea:.3e}", end="")
        assert ev < 1e-6 and ea < 1e-6, (b, lengths[b], ev, ea)


def test_lengths_are_validated_against_min_frames():
    net, _, _ = _net("k2", "statistic", 1, 8)
    net.eval()
    assert net.min_frames() == 5
    x = torch.zeros(2, 1, 8, 12, device=DEV)
    with pytest.raises(ValueError):
        net.extract_embedding(x, lengths=[12, 4])                  # 4 frames leave one on the last map
    net.extract_embedding(x, lengths=[12, 5])
    with pytest.raises(ValueError):
        net.extract_embedding(torch.zeros(2, 1, 8, 4, device=DEV))  # a rectangular batch with one frame on the last map
    att, _, _ = _net("k2", "attentive_statistic", 1, 8)
    att.eval()
    assert att.min_frames() == 1
    att.extract_embedding(x, lengths=[12, 1])
    net.train()
    with pytest.raises(NotImplementedError):
        net.extract_embedding(x, lengths=[12, 5])


# ------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("pooling", ["statistic", "attentive_statistic"])
def test_training_step_gradients_and_running_buffers_vs_fp64_restatement(pooling):
    """loss = (xv * g).sum() at hidden (16,32), F = 8, T = 9, fc_layers 2: every parameter gradient and the BatchNorm running buffers after
    the step against the restatement under oracle.bn_training().  The gradients get the fp32 noise floor measured from the restatement
    itself (fp32 run against fp64 run); tensors whose fp64 gradient is exactly zero (fc1.bias and the like, in front of a BatchNorm) are
    held to 1e-6 absolute.  Precondition: at least one pooled feature of the fp64 map has zero variance over time -- where a standard
    deviation without a floor has a 0/0 gradient -- and every engine gradient is finite.

    The scale of g.  The relative bars do not depend on it; the absolute one for the exactly-zero gradients does.  fc1.bias' gradient is
    the column sum of the BatchNorm's input gradient over B = 3 rows, whose entries are O(|g| gamma invstd): in fp32 that sum is off zero
    by a few ulps of its addends whoever computes it.  With g ~ N(0,1) the addends reach 6 and the restatement's own fp32 run leaves
    3.3e-6 (statistic) / 1.2e-6 (attentive) there -- above the bar before the engine is looked at (the engine: 1.07e-6).  So g carries the
    weight of a mean over the batch's B E embedding elements, N(0,1) / (B E), the scale of the mean cross-entropy the cited test takes its
    gradients from; that the bar can be held at this scale is asserted on the fp32 restatement as well."""
    net, sd, layers = _net("k1", pooling, 2, 8)
    net.train()
    x = _features(3, 8, 9, 47)
    g = torch.randn((3, E), generator=torch.Generator().manual_seed(48)) / (3 * E)
    xv = net(x.to(DEV))
    (xv * g.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    names = [k for k, _ in net.named_parameters()]
    grads = {k: v.grad.detach().cpu().double() for k, v in net.named_parameters()}
    assert all(bool(torch.isfinite(v).all()) for v in grads.values())

    def restate(dtype):
        p = {k: (v.to(dtype).clone() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
        for k in names:
            p[k].requires_grad_(True)
        taps = {}
        with O.bn_training():
            rv, _ = ref_embedding(p, x.to(dtype), layers, pooling, 2, taps)
        (rv * g.to(dtype)).sum().backward()
        return rv.detach(), {k: p[k].grad.double() for k in names}, p, taps["map"].detach()

    rv64, g64, p64, m64 = restate(torch.float64)
    _, g32, _, _ = restate(torch.float32)
    flat = int((m64.var(dim=2, unbiased=True) == 0).sum())
    print(f"\n{pooling}: {flat} of {m64.shape[0] * m64.shape[1] * m64.shape[3]} pooled features constant over time", end="")
    assert flat >= 1
    assert rel_err(xv.detach().cpu().numpy(), rv64.numpy()) < BAR_GRAD
    ours, floor = [], []
    for k in names:
        scale = float(g64[k].abs().max())
        if scale < 1e-9:           # fc1.bias in front of fc1_bn, pooling.k under the softmax: the exact gradient is zero (fp64 leaves 1e-14)
            z32, zg = float(g32[k].abs().max()), float(grads[k].abs().max())
            print(f"\n{pooling}: exactly-zero gradient {k}: engine {zg:.3e}, fp32 restatement {z32:.3e}", end="")
            assert z32 < 1e-6, k           # (the bar is one fp32 can hold at this scale)
            assert zg < 1e-6, k
            continue
        ours.append((float((grads[k] - g64[k]).abs().max()) / scale, k))
        floor.append(float((g32[k] - g64[k]).abs().max()) / scale)
    worst, who = max(ours)
    print(f"\n{pooling}: worst gradient {who} {worst:.3e} (fp32 restatement's worst {max(floor):.3e}); mean {np.mean([e for e, _ in ours]):.3e} "
          f"(fp32 {np.mean(floor):.3e})", end="")
    assert worst < max(1e-4, 2.0 * max(floor)), (who, worst, max(floor))
    assert np.mean([e for e, _ in ours]) < max(1e-4, 2.0 * np.mean(floor))
    for k, v in net.state_dict().items():
        if "running" in k:
            assert rel_err(v.cpu().numpy(), p64[k].numpy()) < BAR_GRAD, k
        elif "num_batches_tracked" in k:
            assert int(v) == 1, k


def test_recorded_step_is_bit_identical_to_eager():
    """A TrainStepGraph of `statistic` + fc_layers 2 (one eager step, then the recorded one replayed) against the eager loop over three
    batches: the same losses, parameters and BatchNorm buffers, bit for bit (after tests/test_train_video_gpu.py's
    recorded_training_step_vs_eager; no dropout anywhere)."""
    from deeplip_amd.train_plan import TrainStepGraph

    def run(graph):
        net, _, _ = _net("k1", "statistic", 2, 8)
        net.train()
        opt = torch.optim.Adam(net.parameters(), lr=torch.tensor(3e-4, device=DEV), weight_decay=1e-4, capturable=True, fused=True)
        gw = torch.randn((3, E), generator=torch.Generator().manual_seed(52)).to(DEV)

        def one(xb):
            opt.zero_grad(set_to_none=True)
            l = (net(xb) * gw).sum()
            l.backward()
            opt.step()
            return l

        plan = TrainStepGraph(one, eager_steps=1) if graph else None
        losses = []
        for i in range(3):
            xb = _features(3, 8, 9, 60 + i).to(DEV)
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


def test_train_audio_trains_and_extracts_with_the_statistics_head(tmp_path, monkeypatch):
    """train_audio.Trainer with the resnet section switched to `pooling: statistic, fc_layers: 2` (feat_dim filled in from the data
    section): one synthetic epoch of two steps, then the ragged test list through the RaggedExtractor."""
    import train_audio
    monkeypatch.chdir(tmp_path)
    tr = train_audio.Trainer(overrides={"model.arch": "resnet", "model.resnet.pooling": "statistic", "model.resnet.fc_layers": 2,
                                        "model.resnet.hidden_dim": [32, 64], "model.resnet.residual_block_layers": [1, 1],
                                        "model.resnet.embedding_dim": 32, "data.feat_dim": 24, "data.test_speakers": 3,
                                        "data.test_utt_per_spk": 2, "data.trials": 30, "data.trial_targets": 6, "data.audio_frames": 60,
                                        "data.n_spk": 5, "data.utt_per_spk": 2, "data.test_audio_frames": [40, 90], "train.bs": 4,
                                        "train.epoch": 1})
    try:
        assert tr.model.feat_dim == 24 and tr.model.min_frames() == 3 and tr._min_frames() == 3
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        assert np.isfinite(loss) and tr.last_epoch_stats["steps"] == 2
        assert all(bool(torch.isfinite(p).all()) for p in tr.model.parameters())
        assert int(tr.model.fc1_bn.num_batches_tracked) == 2
        table = tr.extract_test_xv(batch=4)
        assert table.emb.shape == (6, 32) and bool(torch.isfinite(table.emb).all())
        assert tr.extract_stats["audio_batches"] >= 1
    finally:
        tr.close()
