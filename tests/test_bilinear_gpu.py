"""BNBilinear on the GPU (-m gpu): parity of the kernels and of the module with an fp64 restatement, the arithmetic modes,
determinism and graph replay, and train_fusion's trainer with ``model.fusion: bilinear``.

The yardstick.  The class is absent upstream (the reference's train_fusion.py:84 names it, LBP.py does not define it), so there is
nothing to capture from: the expected values are the five lines below in fp64 on the CPU, with torch.nn.BatchNorm1d and torch
autograd supplying the BatchNorm and every gradient.  Inputs are seeded: randn embeddings, uniform(-1, 1) factors.

The bar is the project's own, conftest.assert_close_rel (|a - b| <= 1e-4 |b| + 1e-6 max|b| for every element); torch's own fp32 on
the CPU stays within 0.43 of it against fp64 on these inputs for z, y and the four gradients, so it is attainable with no
element and no case left out."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, assert_close_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, d1, d2, o, k): the shipped sizes at four batch sizes, then the edges -- d1 != d2, k o no multiple of 240, B above 256, o = 1,
# k = 1, k o no multiple of 4 (the element-wise loads), k above one 64-column pass
SHAPES = [(60, 512, 512, 512, 30), (16, 512, 512, 512, 30), (256, 512, 512, 512, 30), (1, 512, 512, 512, 30), (7, 64, 96, 40, 30),
          (33, 128, 128, 64, 5), (257, 64, 32, 24, 7), (5, 32, 32, 1, 30), (9, 64, 64, 48, 1), (2, 32, 64, 9, 7), (6, 32, 32, 3, 70)]


def _inputs(B, d1, d2, o, k, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + d1 + o + k)
    e1 = torch.randn(B, d1, generator=g, dtype=torch.float64)
    e2 = torch.randn(B, d2, generator=g, dtype=torch.float64)
    U = torch.rand(d1, k * o, generator=g, dtype=torch.float64) * 2 - 1
    V = torch.rand(d2, k * o, generator=g, dtype=torch.float64) * 2 - 1
    # the engine sees the fp32 roundings; the restatement starts from the SAME numbers
    return [t.float().double() for t in (e1, e2, U, V)]


def _pool64(e1, e2, U, V, o, k):
    P = e1 @ U
    Q = e2 @ V
    return (P * Q).view(-1, o, k).mean(-1)


def _head64(e1, e2, U, V, o, k, bn):
    z = _pool64(e1, e2, U, V, o, k)
    y = F.normalize(z, p=2, dim=-1)
    return z, y, bn(y)


def _dev(*ts):
    return [t.float().to(DEV).contiguous() for t in ts]


def _bn64(o, seed=5):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(o).double()
    with torch.no_grad():
        bn.weight.copy_((torch.rand(o, generator=g) + 0.5).float().double())
        bn.bias.copy_((torch.randn(o, generator=g) * 0.1).float().double())
        bn.running_mean.copy_((torch.randn(o, generator=g) * 0.01).float().double())
        bn.running_var.copy_((torch.rand(o, generator=g) * 0.01 + 0.001).float().double())
    return bn


def _module(o, k, d1, d2, U, V, bn):
    from deeplip_amd.fusion import BNBilinear
    m = BNBilinear(d1, d2, o, k=k)
    with torch.no_grad():
        m.U.copy_(U.float()); m.V.copy_(V.float())
        m.bn1.weight.copy_(bn.weight.float()); m.bn1.bias.copy_(bn.bias.float())
        m.bn1.running_mean.copy_(bn.running_mean.float()); m.bn1.running_var.copy_(bn.running_var.float())
    return m.to(DEV)


@pytest.mark.parametrize("shape", SHAPES)
def test_pool_kernels_by_hand_match_fp64(shape):
    """z, the kept P and Q, and the four gradients of the pooling launches for a random dz."""
    from deeplip_amd import ops
    B, d1, d2, o, k = shape
    e1, e2, U, V = _inputs(*shape)
    e1.requires_grad_(); e2.requires_grad_(); U.requires_grad_(); V.requires_grad_()
    z64 = _pool64(e1, e2, U, V, o, k)
    dz64 = torch.randn(B, o, generator=torch.Generator().manual_seed(9), dtype=torch.float64).float().double()
    z64.backward(dz64)
    de1, de2, dU, dV = _dev(e1.detach(), e2.detach(), U.detach(), V.detach())
    z_eval = ops.bilinear_pool(de1, de2, dU, dV, k)
    z, P, Q = ops.bilinear_pool(de1, de2, dU, dV, k, save=True)
    assert torch.equal(z, z_eval)                                           # keeping P and Q does not change a bit of z
    assert_close_rel(z.cpu().numpy(), z64.detach().numpy(), what=f"z {shape}")
    assert_close_rel(P.cpu().numpy(), (e1 @ U).detach().numpy(), what=f"P {shape}")
    assert_close_rel(Q.cpu().numpy(), (e2 @ V).detach().numpy(), what=f"Q {shape}")
    (dz,) = _dev(dz64)
    gU, gV = ops.bilinear_pool_bwd_w(de1, de2, P, Q, dz, k)
    g1, g2 = ops.bilinear_pool_bwd_x(P, Q, dz, dU, dV, k)
    for got, want, name in ((gU, U.grad, "dU"), (gV, V.grad, "dV"), (g1, e1.grad, "de1"), (g2, e2.grad, "de2")):
        assert_close_rel(got.cpu().numpy(), want.numpy(), what=f"{name} {shape}")
    only1, none2 = ops.bilinear_pool_bwd_x(P, Q, dz, dU, dV, k, True, False)
    assert none2 is None and torch.equal(only1, g1)


@pytest.mark.parametrize("shape", SHAPES)
def test_eval_forward_matches_fp64(shape):
    B, d1, d2, o, k = shape
    e1, e2, U, V = _inputs(*shape, seed=1)
    bn = _bn64(o).eval()
    with torch.no_grad():
        _, _, out64 = _head64(e1, e2, U, V, o, k, bn)
    m = _module(o, k, d1, d2, U, V, bn).eval()
    with torch.no_grad():
        out = m(*_dev(e1, e2))
    assert tuple(out.shape) == (B, o)
    assert_close_rel(out.cpu().numpy(), out64.numpy(), what=f"eval out {shape}")


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2])
def test_train_forward_matches_fp64(shape):
    """z, y, out and the updated running statistics; o = 1 included (y = +-1)."""
    from deeplip_amd import autograd as ag
    B, d1, d2, o, k = shape
    e1, e2, U, V = _inputs(*shape, seed=2)
    bn = _bn64(o).train()
    with torch.no_grad():
        z64, y64, out64 = _head64(e1, e2, U, V, o, k, bn)
    m = _module(o, k, d1, d2, U, V, _bn64(o)).train()
    a, b = _dev(e1, e2)
    with torch.no_grad():
        z = ag.bilinear_pool(a, b, m.U, m.V, k)
        y = ag.l2_normalize(z, 1e-12)
        out = m(a, b)
    assert_close_rel(z.cpu().numpy(), z64.numpy(), what=f"z {shape}")
    assert_close_rel(y.cpu().numpy(), y64.numpy(), what=f"y {shape}")
    assert_close_rel(out.cpu().numpy(), out64.numpy(), what=f"out {shape}")
    assert_close_rel(m.bn1.running_mean.cpu().numpy(), bn.running_mean.numpy(), what=f"running_mean {shape}")
    assert_close_rel(m.bn1.running_var.cpu().numpy(), bn.running_var.numpy(), what=f"running_var {shape}")
    assert int(m.bn1.num_batches_tracked) == 1


def _loss(out, w1, w2):
    return (out * w1).sum() + 0.5 * (out * out * w2).sum()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2 and s[3] >= 2])
def test_loss_backward_matches_fp64_autograd(shape):
    """Through loss.backward(): dU, dV, de1, de2, dgamma, dbeta of the whole head (o = 1 is left to the by-hand test: there
    y = +-1 has a zero derivative and every gradient but dbeta is rounding noise around an exact 0)."""
    B, d1, d2, o, k = shape
    e1, e2, U, V = _inputs(*shape, seed=3)
    g = torch.Generator().manual_seed(11)
    w1 = torch.randn(B, o, generator=g, dtype=torch.float64).float().double()
    w2 = torch.randn(B, o, generator=g, dtype=torch.float64).float().double()
    bn = _bn64(o).train()
    for t in (e1, e2, U, V):
        t.requires_grad_()
    _loss(_head64(e1, e2, U, V, o, k, bn)[2], w1, w2).backward()
    m = _module(o, k, d1, d2, U.detach(), V.detach(), _bn64(o)).train()
    a, b = _dev(e1.detach(), e2.detach())
    a.requires_grad_(); b.requires_grad_()
    d1w, d2w = _dev(w1, w2)
    _loss(m(a, b), d1w, d2w).backward()
    for got, want, name in ((m.U.grad, U.grad, "dU"), (m.V.grad, V.grad, "dV"), (a.grad, e1.grad, "de1"), (b.grad, e2.grad, "de2"),
                            (m.bn1.weight.grad, bn.weight.grad, "dgamma"), (m.bn1.bias.grad, bn.bias.grad, "dbeta")):
        assert_close_rel(got.cpu().numpy(), want.numpy(), what=f"{name} {shape}")


def test_frozen_embeddings_get_no_input_gradient_launch():
    """train_fusion freezes the encoders: the Function then returns None for both embeddings (the launch is not made), and an
    embedding that asks alone gets its gradient alone."""
    from deeplip_amd import autograd as ag, ops
    shape = (7, 64, 96, 40, 30)
    e1, e2, U, V = _dev(*_inputs(*shape))
    z, P, Q = ops.bilinear_pool(e1, e2, U, V, 30, save=True)
    dz = torch.randn_like(z)

    class Ctx:
        saved_tensors = (e1, e2, U, V, P, Q)
        k = 30
    Ctx.needs_input_grad = (False, False, True, True, False)
    de1, de2, dU, dV, dk = ag.BilinearPoolFn.backward(Ctx, dz)
    assert de1 is None and de2 is None and dk is None and tuple(dU.shape) == (64, 1200) and tuple(dV.shape) == (96, 1200)
    Ctx.needs_input_grad = (False, True, False, False, False)
    de1, de2, dU, dV, dk = ag.BilinearPoolFn.backward(Ctx, dz)
    assert de1 is None and dU is None and dV is None and tuple(de2.shape) == (7, 96)
    U.requires_grad_(); V.requires_grad_()
    ag.bilinear_pool(e1, e2, U, V, 30).sum().backward()
    assert U.grad is not None and V.grad is not None and e1.grad is None and e2.grad is None


def test_host_checks_raise_before_any_launch():
    from deeplip_amd.fusion import BNBilinear
    from deeplip_amd import ops
    m = BNBilinear(32, 32, 8, k=3).to(DEV)
    e = torch.zeros(4, 32, device=DEV)
    with pytest.raises(ValueError):
        m(e, torch.zeros(5, 32, device=DEV))                               # batch sizes differ
    with pytest.raises(ValueError):
        m.train()(e[:1], e[:1])                                            # BatchNorm1d needs two rows in train mode
    m.eval()(e[:1], e[:1])                                                 # ... one is fine in eval mode
    with pytest.raises(ValueError):
        m(e.double(), e)                                                   # fp32 only
    with pytest.raises(ValueError):
        m(torch.zeros(4, 30, device=DEV), e)                               # d1 % 4, and not the module's width
    with pytest.raises(ValueError):
        ops.bilinear_pool(torch.zeros(4, 64, device=DEV)[:, ::2], e, m.U.detach(), m.V.detach(), 3)      # not contiguous


def test_outputs_are_bit_identical_under_every_arith_mode_and_across_calls():
    from deeplip_amd import arith
    shape = (33, 128, 128, 64, 5)
    B, d1, d2, o, k = shape
    e1, e2, U, V = _inputs(*shape, seed=4)
    a, b = _dev(e1, e2)
    results = []
    for mode in ("auto", "f16x3", "f32", "f32"):
        arith.configure(mode)
        m = _module(o, k, d1, d2, U, V, _bn64(o))
        with torch.no_grad():
            ev = m.eval()(a, b)
        out = m.train()(a, b)
        out.sum().backward()
        results.append([t.detach().clone() for t in (ev, out, m.U.grad, m.V.grad, m.bn1.running_mean, m.bn1.running_var)])
    for r in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0], r))


def _small_net():
    from deeplip_amd.fusion import BNBilinear
    from models.audio_models.loss import CrossEntropy
    rs = np.random.get_state()
    np.random.seed(5)
    net = BNBilinear(64, 64, 32, k=5).to(DEV).train()
    np.random.set_state(rs)
    return net, CrossEntropy(32, 6).to(DEV)


def _batch(seed, B=24):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 64, generator=g).to(DEV), torch.randn(B, 64, generator=g).to(DEV), torch.randint(0, 6, (B,), generator=g).to(DEV))


def test_recorded_step_replayed_on_a_second_batch_is_bit_identical_to_eager():
    from deeplip_amd.train_plan import TrainStepGraph

    def run(recorded):
        torch.manual_seed(3)
        torch.cuda.manual_seed(3)
        net, crit = _small_net()
        params = list(net.parameters()) + list(crit.parameters())
        opt = torch.optim.SGD(params, lr=torch.tensor(0.05, device=DEV), momentum=0.9, fused=True)

        def one(e1, e2, lab):
            opt.zero_grad(set_to_none=True)
            loss, logits = crit(net(e1, e2), lab)
            loss.backward()
            opt.step()
            return loss, logits
        plan = TrainStepGraph(one, eager_steps=1 if recorded else 10 ** 6, device=torch.device(DEV), branch_streams=False, verify=False)
        losses = []
        for seed in (1, 2, 3, 4):
            loss, _ = plan.step(*_batch(seed))
            plan.finish()
            losses.append(float(loss.detach()))
        assert plan.recorded == recorded
        state = torch.cat([t.detach().reshape(-1).float() for t in params + [net.bn1.running_mean, net.bn1.running_var]]).cpu()
        return losses, state

    l_g, s_g = run(True)
    l_e, s_e = run(False)
    assert len(set(l_g)) == 4 and l_g == l_e and torch.equal(s_g, s_e)


SMALL = {"train.bs": 16, "train.epoch": 2, "train.steps_per_epoch": 3, "data.n_spk": 6, "data.utt_per_spk": 4,
         "data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 300, "data.trial_targets": 60,
         "data.video_frames": 9, "data.audio_frames": 120, "data.test_audio_frames": [60, 120], "data.test_video_frames": [5, 12],
         "data.test_clips_per_utt": 2, "test.batch": 16}


@pytest.mark.parametrize("loss", ["CrossEntropy", "LMCL"])
def test_trainer_with_the_bilinear_head(loss, arith_mode, tmp_path, monkeypatch):
    import train_fusion
    from deeplip_amd.fusion import BNBilinear
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("train", overrides=dict(SMALL, **{"train.loss": loss, "model.fusion": "bilinear", "train.sgd.init_lr": 0.05}))
    assert isinstance(tr.model_fusion, BNBilinear) and tr.model_fusion.o == 512 and tr.model_fusion.k == 30
    u0 = tr.model_fusion.U.detach().clone()
    tr.current_epoch = 1
    l0, _ = tr._train_epoch()
    tr.save()
    tr.current_epoch = 2
    l1, _ = tr._train_epoch()
    assert np.isfinite(l0) and np.isfinite(l1)
    assert tr.last_epoch_stats["step_mode"] == "graph"
    assert not torch.equal(u0, tr.model_fusion.U.detach())                 # the factors train
    if loss == "CrossEntropy":
        assert l1 < l0
    p = tr.save()
    want = {k: v.detach().clone() for k, v in tr.model_fusion.state_dict().items()}
    with torch.no_grad():
        for t in tr.model_fusion.state_dict().values():
            t.zero_()
    tr.load(p)
    got = tr.model_fusion.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    tr.epoch = 2
    avg = tr.model_average(2)
    assert set(avg) == set(want) and all(torch.isfinite(v.double()).all() for v in avg.values())
    tr.close()


def test_trainer_eager_step_with_the_bilinear_head(tmp_path, monkeypatch):
    import train_fusion
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("train", overrides=dict(SMALL, **{"model.fusion": "bilinear", "model.bilinear.out_dim": 64, "model.bilinear.rank": 7,
                                                                   "train.graph_step": False, "train.sgd.init_lr": 0.05}), arith_mode="f32")
    assert tr.model_fusion.o == 64 and tr.model_fusion.k == 7
    tr.current_epoch = 1
    l0, _ = tr._train_epoch()
    assert np.isfinite(l0) and tr.last_epoch_stats["step_mode"] == "eager"
    tr.close()


def test_train_fusion_bilinear_dp_on_rccl_one_rank(tmp_path):
    """`train_fusion.py --mode train` with the bilinear head as a one-rank job on the real backend: the 63 MB of factor gradients go
    through GradBuckets inside the recorded step (the pattern of tests/test_rccl_gpu.py)."""
    from deeplip_amd import launch
    over = ["train.bs=16", "train.epoch=1", "train.steps_per_epoch=3", "data.n_spk=6", "data.utt_per_spk=4", "data.test_speakers=4",
            "data.test_utt_per_spk=3", "data.trials=300", "data.trial_targets=60", "data.video_frames=9", "data.audio_frames=120",
            "model.fusion=bilinear"]
    lines = []
    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        rc = launch.self_launch(os.path.join(ROOT, "train_fusion.py"), ["--mode", "train", "--config", os.path.join(ROOT, "conf/fusion_config.yaml"),
                                                                       "--set", *over], 1, relay=lines.append)
    finally:
        os.chdir(cwd)
    text = "".join(lines)
    assert rc == 0, text[-2000:]
    assert "[graph]" in text and "EER" in text
