"""CompactBilinearPooling on the GPU (-m gpu): parity of the kernels, the layer and the trainer's head with an fp64 restatement, the
arithmetic modes, determinism and graph replay, and train_fusion's trainer with ``model.fusion: compact_bilinear``.

The yardstick.  Upstream ships no runnable source for the layer (only a stale bytecode file that calls the removed torch.rfft), so
there is nothing to capture a golden from: the expected values are upstream's FFT form restated in fp64 on the CPU, computed from
the fp32 inputs, with torch autograd supplying every gradient and torch.nn.BatchNorm1d the head's BatchNorm.
tests/test_compact_bilinear_cpu.py checks that form against the direct circular convolution.

The bar is the project's own, conftest.assert_close_rel (|a - b| <= 1e-4 |b| + 1e-6 max|b| for every element), on out, psi1, psi2,
dx1, dx2, the head's out, its running statistics, dgamma and dbeta.  An in-order fp32 accumulation emulated on the CPU stays within
0.19 of that bound for the outputs and for both gradients at (16,1,512,512,512), (8,9,512,512,512), (8,1,40,24,16),
(8,1,512,512,1024), (8,1,512,512,4) and (4,1,7,5,30), so fp32 accumulators hold it with no element and no case left out."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, assert_close_rel

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, P, d1, d2, D): the shipped sizes, a single row, unequal widths, widths no multiple of 4 with D no power of two (one k per
# thread), mostly empty bins, heavy collisions, D = 1, a batch past 256, a 3 x 3 map; then two of this file's own: the largest D (the
# backward's four LDS rows are exactly 64 KB) and several positions on the one-k-per-thread path
SHAPES = [(60, 1, 512, 512, 512), (256, 1, 512, 512, 512), (1, 1, 512, 512, 512), (2, 1, 40, 24, 16), (3, 1, 7, 5, 30),
          (2, 1, 24, 24, 1024), (2, 1, 512, 512, 4), (2, 1, 8, 8, 1), (257, 1, 16, 16, 100), (4, 9, 32, 32, 64),
          (2, 1, 8, 12, 4096), (3, 4, 6, 10, 30)]
HW = {1: (1, 1), 4: (2, 2), 9: (3, 3)}
CASES = [(s, True) for s in SHAPES] + [(s, False) for s in SHAPES if s[1] > 1]


def _layer(d1, d2, D, sum_pool=True, seed=0):
    from deeplip_amd.fusion import CompactBilinearPooling
    rs = torch.random.get_rng_state()
    torch.manual_seed(100 + seed + d1 + d2 + D)
    m = CompactBilinearPooling(d1, d2, D, sum_pool=sum_pool)
    torch.random.set_rng_state(rs)
    return m


def _inputs(shape, seed=0):
    B, P, d1, d2, D = shape
    g = torch.Generator().manual_seed(1000 * seed + B + P + d1 + D)
    return torch.randn(B, d1, *HW[P], generator=g), torch.randn(B, d2, *HW[P], generator=g)


def _cbp64(x1, x2, S1, S2, sum_pool):
    """Upstream's forward in fp64 (x [B,C,H,W] fp64, S [C,D])."""
    D = S1.shape[1]
    psi1 = x1.permute(0, 2, 3, 1) @ S1.double()
    psi2 = x2.permute(0, 2, 3, 1) @ S2.double()
    cbp = torch.fft.irfft(torch.fft.rfft(psi1, dim=-1) * torch.fft.rfft(psi2, dim=-1), n=D, dim=-1) * D
    return (cbp.sum(dim=[1, 2]) if sum_pool else cbp), psi1, psi2


_REF = {}


def _reference(shape, sum_pool):
    """out, psi1, psi2, g, dx1, dx2 in fp64 for the case's seeded inputs; computed once and shared."""
    key = (shape, sum_pool)
    if key not in _REF:
        B, P, d1, d2, D = shape
        m = _layer(d1, d2, D, sum_pool)
        x1, x2 = _inputs(shape)
        a, b = x1.double().requires_grad_(), x2.double().requires_grad_()
        out, psi1, psi2 = _cbp64(a, b, m.tensor_sketch1, m.tensor_sketch2, sum_pool)
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).double()
        out.backward(g)
        _REF[key] = tuple(t.detach().numpy() for t in (out, psi1.reshape(B, P, D), psi2.reshape(B, P, D), g, a.grad, b.grad))
    return _REF[key]


def _packs(m):
    from deeplip_amd import ops
    return ops.compact_bilinear_pack(m.tensor_sketch1.to(DEV), "tensor_sketch1"), ops.compact_bilinear_pack(m.tensor_sketch2.to(DEV), "tensor_sketch2")


@pytest.mark.parametrize("shape,sum_pool", CASES)
def test_kernels_by_hand_match_fp64(shape, sum_pool):
    """out, the kept psi1 and psi2, and both input gradients for a random g: every element."""
    from deeplip_amd import ops
    B, P, d1, d2, D = shape
    out64, psi1_64, psi2_64, g64, dx1_64, dx2_64 = _reference(shape, sum_pool)
    m = _layer(d1, d2, D, sum_pool)
    p1, p2 = _packs(m)
    x1, x2 = (t.to(DEV) for t in _inputs(shape))
    out_only = ops.compact_bilinear(x1, x2, p1, p2, sum_pool)
    out, psi1, psi2 = ops.compact_bilinear(x1, x2, p1, p2, sum_pool, save=True)
    assert torch.equal(out, out_only)                                       # keeping the sketches does not change a bit
    assert tuple(out.shape) == out64.shape and tuple(psi1.shape) == (B, P, D)
    for got, want, name in ((out, out64, "out"), (psi1, psi1_64, "psi1"), (psi2, psi2_64, "psi2")):
        assert_close_rel(got.cpu().numpy(), want, what=f"{name} {shape} pool={sum_pool}")
    g = torch.from_numpy(g64).float().to(DEV)
    dx1, dx2 = ops.compact_bilinear_bwd(g, psi1, psi2, p1, p2, x1.shape, x2.shape, sum_pool)
    assert dx1.shape == x1.shape and dx2.shape == x2.shape
    assert_close_rel(dx1.cpu().numpy(), dx1_64, what=f"dx1 {shape} pool={sum_pool}")
    assert_close_rel(dx2.cpu().numpy(), dx2_64, what=f"dx2 {shape} pool={sum_pool}")
    only1, none2 = ops.compact_bilinear_bwd(g, psi1, psi2, p1, p2, x1.shape, x2.shape, sum_pool, True, False)
    none1, only2 = ops.compact_bilinear_bwd(g, psi1, psi2, p1, p2, x1.shape, x2.shape, sum_pool, False, True)
    assert none1 is None and none2 is None and torch.equal(only1, dx1) and torch.equal(only2, dx2)
    if P == 1:                                                               # [B,C] is [B,C,1,1]
        flat = ops.compact_bilinear(x1.reshape(B, d1), x2.reshape(B, d2), p1, p2, sum_pool)
        assert torch.equal(flat, out)


@pytest.mark.parametrize("shape,sum_pool", CASES)
def test_layer_autograd_matches_fp64(shape, sum_pool):
    """The module through loss.backward(): the same numbers by way of autograd.CompactBilinearFn."""
    B, P, d1, d2, D = shape
    out64, _, _, g64, dx1_64, dx2_64 = _reference(shape, sum_pool)
    m = _layer(d1, d2, D, sum_pool).to(DEV)
    x1, x2 = (t.to(DEV).requires_grad_() for t in _inputs(shape))
    out = m(x1, x2)
    (out * torch.from_numpy(g64).float().to(DEV)).sum().backward()
    assert_close_rel(out.detach().cpu().numpy(), out64, what=f"out {shape}")
    assert_close_rel(x1.grad.cpu().numpy(), dx1_64, what=f"dx1 {shape}")
    assert_close_rel(x2.grad.cpu().numpy(), dx2_64, what=f"dx2 {shape}")


@pytest.mark.parametrize("shape,sum_pool", CASES)
def test_nan_prefilled_outputs_are_fully_written(shape, sum_pool):
    """The entry points called on buffers full of NaN: every element of out, psi1, psi2, dx1, dx2 is written, with the bits the
    wrappers return."""
    from deeplip_amd import ops
    from deeplip_amd._lib import check, lib, ptr, stream_handle
    B, P, d1, d2, D = shape
    m = _layer(d1, d2, D, sum_pool)
    p1, p2 = _packs(m)
    x1, x2 = (t.to(DEV) for t in _inputs(shape))
    want_out, want_psi1, want_psi2 = ops.compact_bilinear(x1, x2, p1, p2, sum_pool, save=True)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    out, psi1, psi2 = nan(*want_out.shape), nan(B, P, D), nan(B, P, D)
    check(lib().dlip_compact_bilinear_f32(ptr(x1), ptr(x2), ptr(p1["rowptr"]), ptr(p1["idx"]), ptr(p1["sgn"]), ptr(p2["rowptr"]), ptr(p2["idx"]),
                                          ptr(p2["sgn"]), ptr(out), ptr(psi1), ptr(psi2), B, d1, d2, P, D, int(sum_pool), stream_handle()), "fwd")
    assert torch.equal(out, want_out) and torch.equal(psi1, want_psi1) and torch.equal(psi2, want_psi2)
    g = torch.randn_like(out)
    want1, want2 = ops.compact_bilinear_bwd(g, psi1, psi2, p1, p2, x1.shape, x2.shape, sum_pool)
    dx1, dx2 = nan(*x1.shape), nan(*x2.shape)
    check(lib().dlip_compact_bilinear_bwd_f32(ptr(g), ptr(psi1), ptr(psi2), ptr(p1["h"]), ptr(p1["s"]), ptr(p2["h"]), ptr(p2["s"]), ptr(dx1),
                                              ptr(dx2), B, d1, d2, P, D, int(sum_pool), stream_handle()), "bwd")
    assert torch.equal(dx1, want1) and torch.equal(dx2, want2) and not torch.isnan(dx1).any() and not torch.isnan(dx2).any()


# ---- the trainer's head: bn1(F.normalize(cbp(e1, e2))) ----
def _bn64(o, seed=5):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm1d(o).double()
    with torch.no_grad():
        bn.weight.copy_((torch.rand(o, generator=g) + 0.5).float().double())
        bn.bias.copy_((torch.randn(o, generator=g) * 0.1).float().double())
        bn.running_mean.copy_((torch.randn(o, generator=g) * 0.01).float().double())
        bn.running_var.copy_((torch.rand(o, generator=g) * 0.01 + 0.001).float().double())
    return bn


def _head(shape, bn, seed=0):
    from deeplip_amd.fusion import BNCompactBilinear
    B, P, d1, d2, D = shape
    rs = torch.random.get_rng_state()
    torch.manual_seed(200 + seed + d1 + d2 + D)
    m = BNCompactBilinear(d1, d2, D)
    torch.random.set_rng_state(rs)
    with torch.no_grad():
        m.bn1.weight.copy_(bn.weight.float()); m.bn1.bias.copy_(bn.bias.float())
        m.bn1.running_mean.copy_(bn.running_mean.float()); m.bn1.running_var.copy_(bn.running_var.float())
    return m


def _head64(m, x1, x2, bn):
    z, _, _ = _cbp64(x1, x2, m.cbp.tensor_sketch1.cpu(), m.cbp.tensor_sketch2.cpu(), True)
    return bn(F.normalize(z, p=2, dim=-1))


def _head_inputs(shape, seed):
    B, P, d1, d2, D = shape
    x1, x2 = _inputs(shape, seed)
    return (x1.reshape(B, d1), x2.reshape(B, d2)) if P == 1 else (x1, x2)      # the trainer hands [B,C] embeddings


def _as4d(t):
    return t if t.dim() == 4 else t[:, :, None, None]


@pytest.mark.parametrize("shape", SHAPES)
def test_head_eval_forward_matches_fp64(shape):
    bn = _bn64(shape[4]).eval()
    m = _head(shape, bn)
    x1, x2 = _head_inputs(shape, 1)
    with torch.no_grad():
        out64 = _head64(m, _as4d(x1).double(), _as4d(x2).double(), bn)
        out = m.to(DEV).eval()(x1.to(DEV), x2.to(DEV))
    assert tuple(out.shape) == (shape[0], shape[4])
    assert_close_rel(out.cpu().numpy(), out64.numpy(), what=f"eval out {shape}")


def _loss(out, w1, w2):
    return (out * w1).sum() + 0.5 * (out * out * w2).sum()


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2])
def test_head_train_step_matches_fp64_autograd(shape):
    """Train mode: out, the updated running statistics, dgamma and dbeta on every shape with the two rows BatchNorm1d needs.  The
    gradients that reach the embeddings are compared where they are more than rounding noise around an exact zero: D >= 2 (at D = 1
    the normalised value is +-1 and its derivative 0) and B >= 3 (two rows leave BatchNorm's backward a difference of equal numbers)."""
    B, P, d1, d2, D = shape
    bn = _bn64(D).train()
    m = _head(shape, _bn64(D))
    x1, x2 = _head_inputs(shape, 2)
    g = torch.Generator().manual_seed(11)
    w1 = torch.randn(B, D, generator=g).double()
    w2 = torch.randn(B, D, generator=g).double()
    a, b = _as4d(x1).double().requires_grad_(), _as4d(x2).double().requires_grad_()
    out64 = _head64(m, a, b, bn)
    _loss(out64, w1, w2).backward()
    m = m.to(DEV).train()
    c, d = x1.to(DEV).requires_grad_(), x2.to(DEV).requires_grad_()
    out = m(c, d)
    _loss(out, w1.float().to(DEV), w2.float().to(DEV)).backward()
    assert_close_rel(out.detach().cpu().numpy(), out64.detach().numpy(), what=f"out {shape}")
    assert_close_rel(m.bn1.running_mean.cpu().numpy(), bn.running_mean.numpy(), what=f"running_mean {shape}")
    assert_close_rel(m.bn1.running_var.cpu().numpy(), bn.running_var.numpy(), what=f"running_var {shape}")
    assert int(m.bn1.num_batches_tracked) == 1
    assert_close_rel(m.bn1.weight.grad.cpu().numpy(), bn.weight.grad.numpy(), what=f"dgamma {shape}")
    assert_close_rel(m.bn1.bias.grad.cpu().numpy(), bn.bias.grad.numpy(), what=f"dbeta {shape}")
    assert m.cbp.tensor_sketch1.grad is None and m.cbp.tensor_sketch2.grad is None
    if D >= 2 and B >= 3:
        assert_close_rel(c.grad.cpu().numpy(), a.grad.reshape(c.shape).numpy(), what=f"de1 {shape}")
        assert_close_rel(d.grad.cpu().numpy(), b.grad.reshape(d.shape).numpy(), what=f"de2 {shape}")


def test_outputs_are_bit_identical_under_every_arith_mode_and_across_calls():
    from deeplip_amd import arith
    shape = (5, 4, 24, 40, 64)
    x1, x2 = (t.to(DEV) for t in _inputs(shape))
    results = []
    for mode in ("auto", "f16x3", "f32", "f32"):
        arith.configure(mode)
        m = _head(shape, _bn64(64)).to(DEV)
        with torch.no_grad():
            ev = m.eval()(x1, x2)
            raw = m.cbp(x1, x2)
        a, b = x1.clone().requires_grad_(), x2.clone().requires_grad_()
        out = m.train()(a, b)
        out.sum().backward()
        results.append([t.detach().clone() for t in (ev, raw, out, a.grad, b.grad, m.bn1.weight.grad, m.bn1.running_mean, m.bn1.running_var)])
    arith.configure("f32")
    for r in results[1:]:
        assert all(torch.equal(x, y) for x, y in zip(results[0], r))


def test_frozen_inputs_make_no_backward_launch(monkeypatch):
    """train_fusion freezes the encoders: nothing is kept by the forward, the output needs no gradient and the backward entry
    point is never reached; an input that asks alone gets its gradient alone."""
    from deeplip_amd import _lib, autograd as ag, ops
    shape = (3, 4, 6, 10, 30)
    m = _layer(6, 10, 30).to(DEV)
    x1, x2 = (t.to(DEV) for t in _inputs(shape))
    calls = []
    real = ops.compact_bilinear
    monkeypatch.setattr(ops, "compact_bilinear", lambda *a, **k: calls.append(k.get("save", False)) or real(*a, **k))
    bwd = []
    real_bwd = ops.compact_bilinear_bwd
    monkeypatch.setattr(ops, "compact_bilinear_bwd", lambda *a, **k: bwd.append(a[-2:]) or real_bwd(*a, **k))
    out = m(x1, x2)
    assert calls == [False] and not out.requires_grad and out.grad_fn is None
    x2.requires_grad_()
    out = m(x1, x2)
    assert calls == [False, True]
    out.sum().backward()
    assert x1.grad is None and x2.grad is not None and bwd == [(False, True)]
    assert ops.compact_bilinear_bwd(out.detach(), None, None, None, None, None, None, True, False, False) == (None, None)
    p1, p2 = _packs(m.cpu())
    _, psi1, psi2 = real(x1, x2.detach(), p1, p2, True, save=True)
    rc = _lib.lib().dlip_compact_bilinear_bwd_f32(_lib.ptr(out.detach()), _lib.ptr(psi1), _lib.ptr(psi2), _lib.ptr(p1["h"]), _lib.ptr(p1["s"]),
                                                  _lib.ptr(p2["h"]), _lib.ptr(p2["s"]), None, None, 3, 6, 10, 4, 30, 1, _lib.stream_handle())
    assert rc == 0                                                           # both outputs absent: accepted, nothing launched
    assert ag.CompactBilinearFn.apply(x1, x2.detach(), p1, p2, True).grad_fn is None


def test_host_checks_raise_before_any_launch():
    from deeplip_amd import ops
    from deeplip_amd._lib import DeepLipHipError
    from deeplip_amd.fusion import BNCompactBilinear
    m = _layer(8, 12, 16).to(DEV)
    x1, x2 = torch.zeros(4, 8, 3, 3, device=DEV), torch.zeros(4, 12, 3, 3, device=DEV)
    m(x1, x2)
    with pytest.raises(ValueError):
        m(x1, x2[:3])                                                        # B differs
    with pytest.raises(ValueError):
        m(x1, torch.zeros(4, 12, 3, 2, device=DEV))                          # W differs
    with pytest.raises(ValueError):
        m(x1, torch.zeros(4, 12, device=DEV))                                # 4-D with 2-D
    with pytest.raises(ValueError):
        m(x1.double(), x2)                                                   # fp32 only
    with pytest.raises(ValueError):
        m(x1, torch.zeros(4, 8, 3, 3, device=DEV))                           # not the sketch's channel count
    with pytest.raises(ValueError):
        m(torch.zeros(4, 3, 3, 8, device=DEV).permute(0, 3, 1, 2), x2)       # not contiguous
    with pytest.raises(ValueError):
        m(torch.zeros(4, 8, 3, device=DEV), torch.zeros(4, 12, 3, device=DEV))      # neither [B,C] nor [B,C,H,W]
    with pytest.raises(DeepLipHipError):
        m(x1.cpu(), x2)
    with torch.no_grad():
        m.tensor_sketch1[3] = 0.0                                            # an empty row: refused at the re-pack, row named
    with pytest.raises(ValueError, match=r"tensor_sketch1: row 3\b"):
        m(x1, x2)
    p1, p2 = _packs(_layer(8, 12, 16))
    p3 = ops.compact_bilinear_pack(_layer(8, 12, 32).tensor_sketch2.to(DEV))
    with pytest.raises(ValueError):
        ops.compact_bilinear(x1, x2, p1, p3)                                 # two different D
    head = BNCompactBilinear(8, 8, 16).to(DEV)
    e = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        head.train()(e[:1], e[:1])                                           # BatchNorm1d needs two rows in train mode
    head.eval()(e[:1], e[:1])                                                # ... one is fine in eval mode


def test_load_state_dict_with_other_sketches_repacks():
    shape = (4, 1, 16, 16, 32)
    a, b = _layer(16, 16, 32, seed=1).to(DEV), _layer(16, 16, 32, seed=2).to(DEV)
    x1, x2 = (t.to(DEV) for t in _inputs(shape))
    out_a, out_b = a(x1, x2), b(x1, x2)
    assert not torch.equal(out_a, out_b)
    a.load_state_dict(b.state_dict(), strict=True)
    assert torch.equal(a(x1, x2), out_b)                                     # the pack was rebuilt from the loaded sketches
    assert not a.tensor_sketch1.requires_grad


def _small_net():
    from models.audio_models.loss import CrossEntropy
    return _head((24, 1, 64, 48, 32), _bn64(32)).to(DEV).train(), CrossEntropy(32, 6).to(DEV)


def _batch(seed, B=24):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, 64, generator=g).to(DEV), torch.randn(B, 48, generator=g).to(DEV), torch.randint(0, 6, (B,), generator=g).to(DEV))


def test_recorded_step_replayed_on_a_second_batch_is_bit_identical_to_eager():
    from deeplip_amd.train_plan import TrainStepGraph

    def run(recorded):
        torch.manual_seed(3)
        torch.cuda.manual_seed(3)
        net, crit = _small_net()
        params = [p for p in net.parameters() if p.requires_grad] + list(crit.parameters())
        opt = torch.optim.SGD(params, lr=torch.tensor(0.05, device=DEV), momentum=0.9, weight_decay=1e-3, fused=True)

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
def test_trainer_with_the_compact_bilinear_head(loss, arith_mode, tmp_path, monkeypatch):
    import train_fusion
    from deeplip_amd.fusion import BNCompactBilinear
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("train", overrides=dict(SMALL, **{"train.loss": loss, "model.fusion": "compact_bilinear", "train.sgd.init_lr": 0.05}))
    head = tr.model_fusion
    assert isinstance(head, BNCompactBilinear) and head.o == 512 and tuple(head.cbp.tensor_sketch1.shape) == (512, 512)
    opt_params = {id(p) for g in tr.optim.param_groups for p in g["params"]}
    assert id(head.bn1.weight) in opt_params and id(head.cbp.tensor_sketch1) not in opt_params and id(head.cbp.tensor_sketch2) not in opt_params
    s0 = [head.cbp.tensor_sketch1.detach().clone(), head.cbp.tensor_sketch2.detach().clone()]
    w0 = head.bn1.weight.detach().clone()
    tr.current_epoch = 1
    l0, _ = tr._train_epoch()
    tr.save()
    tr.current_epoch = 2
    l1, _ = tr._train_epoch()
    assert np.isfinite(l0) and np.isfinite(l1)
    assert tr.last_epoch_stats["step_mode"] == "graph"
    assert not torch.equal(w0, head.bn1.weight.detach())                    # the BatchNorm trains ...
    assert torch.equal(s0[0], head.cbp.tensor_sketch1) and torch.equal(s0[1], head.cbp.tensor_sketch2)      # ... the sketches do not (no weight decay)
    p = tr.save()
    want = {k: v.detach().clone() for k, v in head.state_dict().items()}
    with torch.no_grad():
        for k, t in head.state_dict().items():
            if "sketch" not in k:
                t.zero_()
        head.cbp.tensor_sketch1.copy_(head.cbp.tensor_sketch1.roll(1, 1))   # other hashes: the checkpoint must bring its own back
    tr.load(p)
    got = head.state_dict()
    assert set(got) == set(want) and all(torch.equal(got[k], want[k]) for k in want)
    tr.epoch = 2
    avg = tr.model_average(2)
    assert set(avg) == set(want) and all(torch.isfinite(v.double()).all() for v in avg.values())
    assert torch.equal(avg["cbp.tensor_sketch1"].to(s0[0].device).float(), s0[0])
    tr.close()


def test_trainer_eager_step_with_the_compact_bilinear_head(tmp_path, monkeypatch):
    import train_fusion
    monkeypatch.chdir(tmp_path)
    tr = train_fusion.Trainer("train", overrides=dict(SMALL, **{"model.fusion": "compact_bilinear", "model.compact_bilinear.out_dim": 100,
                                                                   "train.graph_step": False, "train.sgd.init_lr": 0.05}), arith_mode="f32")
    assert tr.model_fusion.o == 100
    tr.current_epoch = 1
    l0, _ = tr._train_epoch()
    assert np.isfinite(l0) and tr.last_epoch_stats["step_mode"] == "eager"
    tr.close()


def test_train_fusion_compact_bilinear_dp_on_rccl_one_rank(tmp_path):
    """`train_fusion.py --mode train` with the compact bilinear head as a one-rank job on the real backend: the sketches take part
    in the start-of-run broadcast and stay out of GradBuckets (the pattern of tests/test_rccl_gpu.py)."""
    from deeplip_amd import launch
    over = ["train.bs=16", "train.epoch=1", "train.steps_per_epoch=3", "data.n_spk=6", "data.utt_per_spk=4", "data.test_speakers=4",
            "data.test_utt_per_spk=3", "data.trials=300", "data.trial_targets=60", "data.video_frames=9", "data.audio_frames=120",
            "model.fusion=compact_bilinear"]
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
