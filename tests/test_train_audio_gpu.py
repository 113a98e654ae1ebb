"""SURVEY §8(f) rank 2 (-m gpu): the speech encoder under model.train() -- every layer differentiable
through dlip_* forward AND backward launches.  Kernel-level gradient checks against torch-CPU autograd
of the same op, then two SGD steps of SpeakerEmbNet + LMCL against values captured from the reference
classes (tests/golden/capture_golden.py: audio_train).  Tolerance 1e-4 relative; argmax bit-exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from deeplip_amd import weightgen as wg

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


@pytest.mark.parametrize("act_first", [False, True])
@pytest.mark.parametrize("M,C", [(8, 512), (1531, 128), (19000, 36)])
def test_bn_rows_act_fwd_bwd(M, C, act_first):
    from deeplip_amd import autograd as ag
    x = (rnd(M, C, seed=1) * 1.5 + 0.3).requires_grad_()
    gamma = (torch.rand(C, generator=torch.Generator().manual_seed(2)) + 0.5).requires_grad_()
    beta = rnd(C, seed=3, scale=0.2).requires_grad_()
    dy = rnd(M, C, seed=4)
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    a = F.leaky_relu(x.double(), 0.2) if act_first else x.double()
    yb = F.batch_norm(a, rm, rv, gamma.double(), beta.double(), training=True, momentum=0.1, eps=1e-5)
    ref = yb if act_first else F.leaky_relu(yb, 0.2)
    ref.backward(dy.double())
    xg = x.detach().to(DEV).requires_grad_(); gg = gamma.detach().to(DEV).requires_grad_(); bg = beta.detach().to(DEV).requires_grad_()
    rmg, rvg = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = ag.BNRowsActFn.apply(xg, gg, bg, rmg, rvg, 0.1, 1e-5, 0.2, act_first)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    assert rel_err(xg.grad.cpu().numpy(), x.grad.numpy()) < 1e-4
    assert rel_err(gg.grad.cpu().numpy(), gamma.grad.numpy()) < 1e-4
    assert rel_err(bg.grad.cpu().numpy(), beta.grad.numpy()) < 1e-4
    assert rel_err(rvg.cpu().numpy(), rv.numpy()) < 1e-5 and rel_err(rmg.cpu().numpy(), rm.numpy()) < 1e-5


def test_meanstd_pool_bwd():
    from deeplip_amd import autograd as ag
    x = (rnd(3, 57, 128, seed=5) * 0.7 + 1.0).requires_grad_()          # [B,T,C]
    dy = rnd(3, 256, seed=6)
    xt = x.double().permute(0, 2, 1)
    ref = torch.cat([xt.mean(2), xt.std(2)], 1)
    ref.backward(dy.double())
    xg = x.detach().to(DEV).requires_grad_()
    y = ag.meanstd_pool(xg)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    assert rel_err(y.detach().cpu().numpy(), ref.detach().numpy()) < 1e-6
    assert rel_err(xg.grad.cpu().numpy(), x.grad.numpy()) < 1e-5


def test_permute3():
    from deeplip_amd import autograd as ag
    x = rnd(5, 7, 12, seed=7)
    assert torch.equal(ag._permute3(x.to(DEV), (0, 2, 1)).cpu(), x.permute(0, 2, 1).contiguous())
    assert torch.equal(ag._permute3(x.to(DEV), (1, 2, 0), flip_axis=2).cpu(), x.flip(2).permute(1, 2, 0).contiguous())
    assert torch.equal(ag._permute3(x.to(DEV), (2, 1, 0)).cpu(), x.permute(2, 1, 0).contiguous())


@pytest.mark.parametrize("B,T,C,K,S,dil,act_first", [(4, 60, 24, 64, 5, 1, False), (3, 50, 128, 256, 3, 2, False),
                                                     (2, 47, 64, 128, 3, 3, True), (5, 33, 256, 512, 1, 1, False),
                                                     # (round 4: the fused operand flow's fall-backs -- an output width that is no multiple of
                                                     # 64 / 32 (tdnn.9's 1 500) on a k = 1 and on a k = 3 layer, 64 input channels)
                                                     (2, 40, 64, 100, 1, 1, False), (2, 40, 64, 100, 3, 1, True), (3, 45, 64, 64, 1, 1, True)])
def test_tdnn_block_train_fn_gradients(B, T, C, K, S, dil, act_first):
    """Conv1d + train-mode BN + LeakyReLU: output and d/dx, d/dW, d/db, d/dgamma, d/dbeta vs torch autograd (fp64)."""
    from deeplip_amd import autograd as ag
    x = rnd(B, C, T, seed=11).requires_grad_()                            # reference layout [B,C,T]
    w = rnd(K, C, S, seed=12, scale=1.0 / np.sqrt(C * S)).requires_grad_()
    b = rnd(K, seed=13, scale=0.1).requires_grad_()
    gamma = (torch.rand(K, generator=torch.Generator().manual_seed(14)) + 0.5).requires_grad_()
    beta = rnd(K, seed=15, scale=0.2).requires_grad_()
    z = F.conv1d(x.double(), w.double(), b.double(), dilation=dil)
    if act_first:
        ref = F.batch_norm(F.leaky_relu(z, 0.2), None, None, gamma.double(), beta.double(), training=True, eps=1e-5)
    else:
        ref = F.leaky_relu(F.batch_norm(z, None, None, gamma.double(), beta.double(), training=True, eps=1e-5), 0.2)
    dy = rnd(*ref.shape, seed=16)
    ref.backward(dy.double())
    xg = x.detach().permute(0, 2, 1).contiguous().to(DEV).requires_grad_()   # [B,T,C]
    wg_, bg, gg, beg = (t.detach().to(DEV).requires_grad_() for t in (w, b, gamma, beta))
    rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    y = ag.TDNNBlockTrainFn.apply(xg, wg_, bg, gg, beg, rm, rv, 0.1, 1e-5, 0.2, dil, act_first)
    y.backward(dy.permute(0, 2, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    assert rel_err(y.detach().cpu().permute(0, 2, 1).numpy(), ref.detach().numpy()) < 2e-5
    assert rel_err(xg.grad.cpu().permute(0, 2, 1).numpy(), x.grad.numpy()) < 1e-4
    assert rel_err(wg_.grad.cpu().numpy(), w.grad.numpy()) < 1e-4
    assert rel_err(gg.grad.cpu().numpy(), gamma.grad.numpy()) < 1e-4
    assert rel_err(beg.grad.cpu().numpy(), beta.grad.numpy()) < 1e-4
    if act_first:
        assert rel_err(bg.grad.cpu().numpy(), b.grad.numpy()) < 1e-4
    else:   # the conv bias sits right in front of a batch-statistics BN: its gradient is zero up to rounding on both sides
        assert float(bg.grad.abs().max()) < 1e-4 * float(dy.abs().sum() / K) + 1e-5


@pytest.mark.parametrize("B,T,C,K1,K2,S2,dil2", [(9, 60, 64, 128, 64, 1, 1), (7, 70, 64, 512, 128, 3, 2), (5, 44, 32, 64, 96, 3, 1), (6, 50, 64, 100, 64, 1, 1),
                                                 (6, 50, 64, 64, 64, 1, 1)])      # (k = 1 behind 64 channels: the producer's 64-channel tile)
def test_tdnn_blocks_with_the_activation_applied_on_load(B, T, C, K1, K2, S2, dil2):
    """Round 5: a TDNN block's activated output is not stored when the next block can take it on load -- the next block's operand
    producers read the raw convolution output and apply BatchNorm + LeakyReLU per loaded value (dlip_wgrad_*_bn_f32).  Two blocks in a
    row, deferred against stored: outputs, every gradient and the running statistics bit for bit; a second block that cannot take the
    values on load (K1 = 100: no multiple of 64) has them written first."""
    from deeplip_amd import autograd as ag
    x = rnd(B, T, C, seed=61)
    w1 = rnd(K1, C, 3, seed=62, scale=1.0 / np.sqrt(C * 3)); b1 = rnd(K1, seed=63, scale=0.1)
    w2 = rnd(K2, K1, S2, seed=64, scale=1.0 / np.sqrt(K1 * S2)); b2 = rnd(K2, seed=65, scale=0.1)
    g1 = torch.rand(K1, generator=torch.Generator().manual_seed(66)) + 0.5; be1 = rnd(K1, seed=67, scale=0.2)
    g2 = torch.rand(K2, generator=torch.Generator().manual_seed(68)) + 0.5; be2 = rnd(K2, seed=69, scale=0.2)
    dy = rnd(B, T - 2 - dil2 * (S2 - 1), K2, seed=70)

    def run(defer):
        ts = [t.clone().to(DEV).requires_grad_() for t in (x, w1, b1, g1, be1, w2, b2, g2, be2)]
        xg, a1, c1, d1, e1, a2, c2, d2, e2 = ts
        rm1, rv1, rm2, rv2 = torch.zeros(K1, device=DEV), torch.ones(K1, device=DEV), torch.zeros(K2, device=DEV), torch.ones(K2, device=DEV)
        n1 = torch.zeros((), dtype=torch.long, device=DEV)
        out = ag.TDNNBlockTrainFn.apply(xg, a1, c1, d1, e1, rm1, rv1, 0.1, 1e-5, 0.2, 1, False, n1, defer, None)
        pend = None
        if defer:
            h, z, mean, invstd = out
            pend = (z, mean, invstd, d1.detach(), e1.detach(), 0.2)
        else:
            h = out
        y = ag.TDNNBlockTrainFn.apply(h, a2, c2, d2, e2, rm2, rv2, 0.1, 1e-5, 0.2, dil2, False, None, False, pend)
        y.backward(dy.to(DEV))
        torch.cuda.synchronize()
        return [y.detach().clone()] + [t.grad.clone() for t in ts] + [rm1, rv1, rm2, rv2, n1.float()]

    a, b = run(True), run(False)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), i
    assert float(a[-1]) == 1.0


def load(module, prefix):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    sd = wg.fill_state_dict(shapes, prefix=prefix)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return module.to(DEV)


def test_speaker_encoder_two_sgd_steps_vs_reference_golden(golden):
    speaker_encoder_two_sgd_steps_vs_reference_golden(golden["audio_train"])


def speaker_encoder_two_sgd_steps_vs_reference_golden(g):
    """(the body of the test above, in whichever arithmetic is configured: test_train_f32_gpu.py runs it again under arith "f32")"""
    from models.audio_models.loss import LMCL
    from models.audio_models.tdnn import SpeakerEmbNet
    opts = {"arch": "tdnn", "tdnn": {"input_dim": 24, "hidden_dim": [512] * 4 + [1500],
                                     "context": [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0], [0]], "tdnn_layers": 5,
                                     "embedding_dim": 512, "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}}
    net = load(SpeakerEmbNet(opts), "atrain.audio.").train()
    crit = load(LMCL(512, 57, 30, 0.2), "atrain.lmcl.").train()
    x = torch.from_numpy(wg.audio_input(8, 24, 120, key="atrain.x")).to(DEV)
    lab = torch.from_numpy(wg.labels(8, 57)).to(DEV)
    opt = torch.optim.SGD([{"params": net.parameters()}, {"params": crit.parameters()}], 0.01, momentum=0.9, weight_decay=1e-5)
    for step in range(2):
        opt.zero_grad()
        output = net(x)
        loss, logits = crit(output, lab)
        loss.backward()
        if step == 0:
            assert abs(float(loss) - float(g["loss0"])) < 1e-4 * float(g["loss0"])
            assert rel_err(output.detach().cpu().numpy(), g["output0"]) < 1e-4
            assert rel_err(logits.detach().cpu().numpy(), g["logits0"]) < 1e-4
            assert np.array_equal(torch.max(logits, 1)[1].cpu().numpy(), g["argmax0"])
            gr = {k: v.grad for k, v in net.named_parameters()}
            # Layers behind the last LeakyReLU: 1e-4 element-wise.  Below it the element-wise bar is 2e-2: LeakyReLU'
            # is a step function, and the handful of BN outputs within ~1e-5 of zero (of 1.2 M) take the other
            # slope when the forward differs from the reference's in the 6th digit -- each moves one column of a
            # bias / weight gradient by 0.8 |dy|.  Measured against an fp64 autograd run the incoming gradient of
            # every layer is right to 4e-6 and each block's own backward to 1e-7 (kernel tests above); the norms of
            # all 28 gradients agree with the reference's to 1e-4 (below).
            assert rel_err(gr["bn2.weight"].cpu().numpy(), g["grad_bn2_w"]) < 1e-4
            assert rel_err(gr["fc1.weight"][:4].cpu().numpy(), g["grad_fc1_w_rows4"]) < 1e-4
            assert rel_err(gr["tdnn.0.context_layer.weight"].cpu().numpy(), g["grad_tdnn0_w"]) < 2e-2
            assert rel_err(gr["tdnn.0.bn.weight"].cpu().numpy(), g["grad_tdnn0_bn_w"]) < 2e-2
            assert rel_err(gr["tdnn.2.context_layer.weight"][:4].cpu().numpy(), g["grad_tdnn2_w_rows4"]) < 2e-2
            assert rel_err(gr["tdnn.4.bn.bias"].cpu().numpy(), g["grad_tdnn4_bn_b"]) < 2e-2
            for k, v in gr.items():
                ref = g[f"gradnorm_{k}"]
                if ref[0] > 1e-6:          # (biases in front of a batch-statistics BN have ~0 gradient: skip the ratio)
                    assert abs(float(v.double().norm()) - ref[0]) < 1e-4 * ref[0], k
        opt.step()
    assert abs(float(loss) - float(g["loss1"])) < 1e-3 * max(1.0, float(g["loss1"]))
    assert rel_err(net.tdnn[0].context_layer.weight.detach().cpu().numpy(), g["after2_tdnn0_w"]) < 1e-4
    assert rel_err(net.tdnn[1].bn.running_var.cpu().numpy(), g["after2_tdnn1_running_var"]) < 1e-4
    assert rel_err(net.fc2.weight.detach()[:4].cpu().numpy(), g["after2_fc2_w_rows4"]) < 1e-4
    assert int(net.tdnn[3].bn.num_batches_tracked) == 2
    for k, v in net.state_dict().items():
        ref = g[f"after2_{k}_sum"]
        assert abs(float(v.detach().double().abs().sum()) - ref[1]) < 1e-4 * max(ref[1], 1e-6), k


@pytest.mark.parametrize("B,T,C,H", [(32, 278, 1500, 64), (3, 41, 64, 16),
                                     (2, 257, 8, 4),        # a second 256-frame alpha chunk; a channel block with 2 of 16 float4 lanes active
                                     (2, 5, 68, 5),         # a second, one-float4 channel block; H % 4 != 0: the nn.Linear hidden layer
                                     (2, 2, 4, 1)])         # one float4, one hidden unit, two frames
def test_attentive_stat_pooling_forward_backward_vs_oracle_autograd(B, T, C, H):
    """AttentiveStatPooling under model.train() (models/audio_models/pooling.py:87-107; `pooling: attentive_statistic`, tdnn.py:66-75)
    at the size the E-TDNN feeds it ([32,1500,278]) and at the edge shapes of the kernels it shares with MultiHeadAttention (one head,
    eps = 0: the unfloored root): output and the gradients of x, W, b, v, k against torch autograd of the oracle's restatement in fp64.
    (x is kept positive-ish with a real spread over frames so that no channel's weighted variance sits at the fp32 cancellation floor,
    where the reference itself returns NaN: the smallest fp64 standard deviation of the five cases is 0.118.)"""
    from deeplip_amd import autograd as ag
    from models.audio_models.pooling import AttentiveStatPooling
    from oracle import deeplip_oracle as O
    pool = AttentiveStatPooling(C, H)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        pool.W.copy_(torch.randn(H, C, generator=g) / np.sqrt(C)); pool.b.copy_(torch.randn(1, H, generator=g) * 0.1)
        pool.v.copy_(torch.randn(H, 1, generator=g) * 0.5); pool.k.copy_(torch.randn(1, 1, generator=g) * 0.1)
    x = torch.randn(B, C, T, generator=g) * 0.8 + 0.3                      # reference layout [B,C,T]
    dy = torch.randn(B, 2 * C, generator=g)
    sd = {"pooling." + k: v.detach().double().clone().requires_grad_() for k, v in pool.named_parameters()}
    xr = x.double().requires_grad_()
    ref = O.attentive_stat_pooling(sd, "pooling", xr)
    ref.backward(dy.double())
    pool = pool.to(DEV)
    xg = x.permute(0, 2, 1).contiguous().to(DEV).requires_grad_()          # engine layout [B,T,C]
    y = ag.attentive_stat_pool(xg, pool)
    y.backward(dy.to(DEV))
    torch.cuda.synchronize()
    e_y, e_x = rel_err(y.detach().cpu().numpy(), ref.detach().numpy()), rel_err(xg.grad.cpu().permute(0, 2, 1).numpy(), xr.grad.numpy())
    print(f"\n({B}, {T}, {C}, {H}): smallest fp64 std {float(ref.detach()[:, C:].min()):.3f} y {e_y:.3e} dx {e_x:.3e}", end="")
    assert e_y < 1e-5
    assert e_x < 1e-4
    for k, p in pool.named_parameters():
        if k == "k":            # softmax is shift-invariant: d/dk = 0 exactly, rounding noise on both sides
            print(f" dk {float(p.grad.abs().max()):.3e}", end="")
            assert float(p.grad.abs().max()) < 1e-5 * float(dy.abs().sum() / B)
            continue
        e = rel_err(p.grad.cpu().numpy(), sd["pooling." + k].grad.numpy())
        print(f" d{k} {e:.3e}", end="")
        assert e < 1e-4, k
    # eval-mode forward of the same module (the golden-pinned kernel): same values
    with torch.no_grad():
        assert rel_err(pool.eval().run_ntc(xg.detach()).cpu().numpy(), ref.detach().numpy()) < 1e-5


def test_attentive_speaker_encoder_two_sgd_steps_vs_reference_golden(golden):
    """`pooling: attentive_statistic` trains: two SGD steps of SpeakerEmbNet + LMCL against values captured from the reference's own
    classes (tests/golden/capture_golden.py: audio_attn_train; lr 1e-4 -- at the config's 0.01 the reference's second forward is NaN
    on these inputs, see the capture script)."""
    attentive_speaker_encoder_two_sgd_steps_vs_reference_golden(golden["audio_attn_train"])


def attentive_speaker_encoder_two_sgd_steps_vs_reference_golden(g):
    """(the body of the test above, in whichever arithmetic is configured: test_train_f32_gpu.py runs it again under arith "f32")"""
    from models.audio_models.loss import LMCL
    from models.audio_models.tdnn import SpeakerEmbNet
    opts = {"arch": "tdnn", "tdnn": {"input_dim": 24, "hidden_dim": [512] * 4 + [1500],
                                     "context": [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0], [0]], "tdnn_layers": 5,
                                     "embedding_dim": 512, "pooling": "attentive_statistic", "attention_hidden_size": 64, "bn_first": True}}
    net = load(SpeakerEmbNet(opts), "attrain.audio.").train()
    crit = load(LMCL(512, 57, 30, 0.2), "attrain.lmcl.").train()
    x = torch.from_numpy(wg.audio_input(8, 24, 120, key="attrain.x")).to(DEV)
    lab = torch.from_numpy(wg.labels(8, 57)).to(DEV)
    opt = torch.optim.SGD([{"params": net.parameters()}, {"params": crit.parameters()}], 0.0001, momentum=0.9, weight_decay=1e-5)
    for step in range(2):
        opt.zero_grad()
        output = net(x)
        loss, logits = crit(output, lab)
        loss.backward()
        if step == 0:
            assert abs(float(loss) - float(g["loss0"])) < 1e-4 * float(g["loss0"])
            assert rel_err(output.detach().cpu().numpy(), g["output0"]) < 1e-4
            assert rel_err(logits.detach().cpu().numpy(), g["logits0"]) < 1e-4
            assert np.array_equal(torch.max(logits, 1)[1].cpu().numpy(), g["argmax0"])
            gr = {k: v.grad for k, v in net.named_parameters()}
            for k in ("pooling.W", "pooling.b", "pooling.v"):
                got = gr[k][:6] if k == "pooling.W" else gr[k]                        # (the fixture keeps six rows of W's gradient)
                assert rel_err(got.cpu().numpy(), g["grad_" + k]) < 1e-3, k           # (through sqrt(q - m^2): fp32 cancellation on both sides)
            assert abs(float(gr["pooling.k"])) < 1e-5                                  # softmax is shift-invariant: d/dk = 0 up to rounding
            assert rel_err(gr["fc1.weight"][:4].cpu().numpy(), g["grad_fc1_w_rows4"]) < 1e-4
            for k, v in gr.items():
                ref = g[f"gradnorm_{k}"]
                if ref[0] > 1e-5:
                    assert abs(float(v.double().norm()) - ref[0]) < 2e-3 * ref[0], k
        opt.step()
    assert abs(float(loss) - float(g["loss1"])) < 1e-3 * max(1.0, float(g["loss1"]))
    for k in ("pooling.W", "pooling.v"):
        got = dict(net.named_parameters())[k].detach()
        assert rel_err((got[:6] if k == "pooling.W" else got).cpu().numpy(), g["after2_" + k]) < 1e-4, k
    for k, v in net.state_dict().items():
        ref = g[f"after2_{k}_sum"]
        assert abs(float(v.detach().double().abs().sum()) - ref[1]) < 1e-4 * max(ref[1], 1e-6), k


def test_full_size_training_step_vs_fp64_oracle():
    """The speech encoder's optimisation step at the size bench.py times it (configs.F2_train_audio_step: B = 256 utterances x 300
    frames x 24 features, E-TDNN, LMCL): loss and EVERY parameter's gradient against the oracle's train-mode restatement
    (oracle.speaker_forward_train + oracle.lmcl) in fp64 with torch autograd on the host cores.  The LeakyReLU kinks make any
    fp32 evaluation sit 1e-3 .. 6e-3 (per tensor: largest element error over largest element) from the fp64 gradient -- measured
    with the same oracle in fp32 -- so the gradients are held to that floor (worst tensor and average within twice the fp32
    oracle's), the loss to 1e-5."""
    import os
    import torch.nn.functional as F  # noqa: F401
    from deeplip_amd import weightgen as wg
    from models.audio_models.loss import LMCL
    from models.audio_models.tdnn import SpeakerEmbNet
    from oracle import deeplip_oracle as O
    B = 256
    et = {"input_dim": 24, "hidden_dim": [512] * 9 + [1500], "context": O.ETDNN_CONTEXT, "tdnn_layers": 10, "embedding_dim": 512,
          "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}
    net = SpeakerEmbNet({"arch": "etdnn", "etdnn": et})
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="audio.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net.cuda().train()
    crit = LMCL(512, 57, 30, 0.2).cuda()
    x = torch.from_numpy(wg.audio_input(B, 24, 300, key="full.atrain"))
    lab = torch.from_numpy(wg.labels(B, 57))
    sd0 = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    cw = crit.weights.detach().cpu().clone()
    loss, _ = crit(net(x.cuda()), lab.cuda())
    loss.backward()
    torch.cuda.synchronize()
    names = [k for k, _ in net.named_parameters()]
    grads = {k: v.grad.detach().cpu().double() for k, v in net.named_parameters()}
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))

    def oracle(dt):
        p = {k: (v.to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd0.items()}
        for k in names:
            p[k].requires_grad_(True)
        l, _ = O.lmcl(O.speaker_forward_train(p, x.to(dt), O.ETDNN_CONTEXT), lab, cw.to(dt), 30, 0.2)
        l.backward()
        return float(l.detach()), {k: p[k].grad.double() for k in names}

    l64, g64 = oracle(torch.float64)
    _, g32 = oracle(torch.float32)
    assert abs(float(loss.detach()) - l64) < 1e-5 * abs(l64)
    ours, floor = [], []
    for k in names:
        sc = float(g64[k].abs().max())
        if sc < 1e-12:
            continue
        ours.append((float((grads[k] - g64[k]).abs().max()) / sc, k))
        floor.append(float((g32[k] - g64[k]).abs().max()) / sc)
    worst, who = max(ours)
    assert worst < max(1e-4, 2.0 * max(floor)), (who, worst, max(floor))
    assert np.mean([e for e, _ in ours]) < max(1e-4, 2.0 * np.mean(floor))


@pytest.mark.parametrize("B,T,C,K,S,dil,act_first", [(40, 120, 64, 128, 1, 1, False), (40, 120, 64, 128, 3, 2, False), (24, 200, 128, 64, 5, 1, False),
                                                     (40, 120, 64, 128, 1, 1, True), (36, 130, 64, 192, 3, 1, False),
                                                     # (ABI 49) a k = 1 layer whose width is no multiple of 64 / of 32: the ragged last channel block
                                                     (40, 120, 64, 100, 1, 1, False), (20, 250, 128, 1500, 1, 1, False),
                                                     (35, 118, 64, 64, 1, 1, False)])       # (the k = 1 producer's 64-channel tile, not ragged)
def test_tdnn_block_backward_with_the_batchnorm_gradient_formed_on_load(B, T, C, K, S, dil, act_first, monkeypatch):
    """ABI 47: conv -> BatchNorm -> LeakyReLU under backward() at more than 4 096 rows -- the BatchNorm's input gradient dz is formed per loaded
    value by the operand producers of the convolution in front (dlip_wgrad_*_bnbwd_f32) behind a sums pass that also bounds its lift
    (dlip_bn_rows_train_bwd_sums_f32), and never stored.  Against fp64 autograd (1e-4), and against the path that stores dz (the same
    expression per value; the lift's exponent differs, which moves nothing but the last bit of a split: 2e-6)."""
    from deeplip_amd import autograd as ag
    x = rnd(B, C, T, seed=21).requires_grad_()
    w = rnd(K, C, S, seed=22, scale=1.0 / np.sqrt(C * S)).requires_grad_()
    b = rnd(K, seed=23, scale=0.1).requires_grad_()
    gamma = (torch.rand(K, generator=torch.Generator().manual_seed(24)) + 0.5).requires_grad_()
    beta = rnd(K, seed=25, scale=0.2).requires_grad_()
    z = F.conv1d(x.double(), w.double(), b.double(), dilation=dil)
    if act_first:
        ref = F.batch_norm(F.leaky_relu(z, 0.2), None, None, gamma.double(), beta.double(), training=True, eps=1e-5)
    else:
        ref = F.leaky_relu(F.batch_norm(z, None, None, gamma.double(), beta.double(), training=True, eps=1e-5), 0.2)
    dy = rnd(*ref.shape, seed=26) * 1e-4                     # (gradient-sized values: the lift matters)
    ref.backward(dy.double())
    assert B * (T - dil * (S - 1)) > ag.BN_SMALL_ROWS
    out = {}
    for fused in (True, False):
        monkeypatch.setattr(ag, "BN_BWD_ON_LOAD", fused)
        xg = x.detach().permute(0, 2, 1).contiguous().to(DEV).requires_grad_()
        wg_, bg, gg, beg = (t.detach().to(DEV).requires_grad_() for t in (w, b, gamma, beta))
        rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
        y = ag.TDNNBlockTrainFn.apply(xg, wg_, bg, gg, beg, rm, rv, 0.1, 1e-5, 0.2, dil, act_first)
        y.backward(dy.permute(0, 2, 1).contiguous().to(DEV))
        torch.cuda.synchronize()
        out[fused] = (xg.grad.cpu().permute(0, 2, 1).numpy(), wg_.grad.cpu().numpy(), gg.grad.cpu().numpy(), beg.grad.cpu().numpy(), bg.grad.cpu().numpy())
    for got in out.values():
        assert rel_err(got[0], x.grad.numpy()) < 1e-4
        assert rel_err(got[1], w.grad.numpy()) < 1e-4
        assert rel_err(got[2], gamma.grad.numpy()) < 1e-4
        assert rel_err(got[3], beta.grad.numpy()) < 1e-4
    for a, c in zip(out[True][:4], out[False][:4]):
        assert rel_err(a, c) < 2e-6
    from deeplip_amd import _lib
    _lib.check_range(sync=True)


@pytest.mark.parametrize("B,switch", [(12, "POOL_BN_ON_LOAD"), (64, "POOL_BN_ON_LOAD"), (64, "POOL_BWD_ON_LOAD")])
def test_meanstd_pooling_with_the_batchnorm_in_front_applied_on_load(B, switch, monkeypatch):
    """ABI 48: the last TDNN block's BatchNorm + LeakyReLU output is not stored when the statistics pooling behind it reads the raw
    convolution output and applies them per loaded value (forward AND backward; POOL_BN_ON_LOAD) -- and with more than 4 096 rows (B = 64)
    the pooling's backward writes nothing either: the block's BatchNorm backward forms that gradient per loaded value from the pooled
    statistics and their gradient (POOL_BWD_ON_LOAD, dlip_bn_rows_train_bwd_ms_f32).  The whole encoder's forward + backward with the switch
    on and off: same loss, same running statistics, gradients to 1e-6 (the same expressions per value)."""
    from deeplip_amd import autograd as ag, weightgen as wg
    from models.audio_models.loss import LMCL
    from models.audio_models.tdnn import SpeakerEmbNet
    from oracle import deeplip_oracle as O
    opts = {"arch": "tdnn", "tdnn": {"input_dim": 24, "hidden_dim": [512] * 4 + [1500], "context": O.TDNN_CONTEXT, "tdnn_layers": 5,
                                      "embedding_dim": 512, "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}}
    x = torch.from_numpy(wg.audio_input(B, 24, 90, key="pool.onload")).to(DEV)
    lab = torch.from_numpy(wg.labels(B, 19)).to(DEV)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(ag, switch, on)
        net = SpeakerEmbNet(opts)
        sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="audio_tdnn.")
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.to(DEV).train()
        crit = LMCL(512, 19, 30, 0.2).to(DEV)
        with torch.no_grad():
            crit.weights.copy_(torch.from_numpy(wg.fill_state_dict({"w": tuple(crit.weights.shape)}, prefix="pool.onload.crit.")["w"]))
        loss, _ = crit(net(x), lab)
        loss.backward()
        torch.cuda.synchronize()
        res[on] = (float(loss.detach()), {k: v.grad.detach().cpu().numpy() for k, v in net.named_parameters()},
                   {k: v.detach().cpu().numpy() for k, v in net.named_buffers()})
    assert res[True][0] == res[False][0]
    for k in res[True][1]:
        assert rel_err(res[True][1][k], res[False][1][k]) < 1e-6, k
    for k in res[True][2]:
        assert np.array_equal(res[True][2][k], res[False][2][k]), k            # running statistics: the same sums
