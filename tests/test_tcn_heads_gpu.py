"""The single-branch TCN head and the depthwise-separable (dwpw) heads on the MI355X: the depthwise temporal-convolution kernels
(deeplip_amd/csrc/tcn_dw_ops.hip) against an fp64 restatement, eval logits and per-block outputs against the reference's
(tests/golden/capture_tcn_heads_golden.py) under every arithmetic mode, whole models on both trunks, one train-mode step of each
new head against the reference's loss / gradients / running statistics, recorded steps against eager ones, and train_video.py with a
dwpw config."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, assert_close_rel, rel_err
from deeplip_amd import arith, ops
from deeplip_amd import weightgen as wg
from test_tcn_heads_cpu import VARIANTS, fill, make_head, opts

pytestmark = pytest.mark.gpu
DEV = "cuda"

TRAIN = {
    "k3": ([3], False, 64, [32] * 3),
    "k3_dwpw": ([3], True, 64, [32] * 3),
    "k357_dwpw": ([3, 5, 7], True, 64, [48] * 2),
}
TRAIN_B, TRAIN_T, TRAIN_CLASSES = 4, 10, 10


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "tcn_heads_golden.npz"))


# ---------------------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def ref_fwd(x, w, d, P, T_out):
    """fp64 z[b,t,c] = sum_j w[j,c] x[b, t - P + j d, c], zeros outside [0, T)."""
    B, T, C = x.shape
    z = np.zeros((B, T_out, C))
    for j in range(w.shape[0]):
        lo, hi = max(0, P - j * d), min(T_out, T + P - j * d)
        if lo < hi:
            z[:, lo:hi] += w[j] * x[:, lo - P + j * d:hi - P + j * d]
    return z


def ref_dgrad(dz, w, d, P, T):
    B, T_out, C = dz.shape
    dx = np.zeros((B, T, C))
    for j in range(w.shape[0]):
        lo, hi = max(0, j * d - P), min(T, T_out + j * d - P)
        if lo < hi:
            dx[:, lo:hi] += w[j] * dz[:, lo + P - j * d:hi + P - j * d]
    return dx


def ref_wgrad(x, dz, k, d, P):
    B, T, C = x.shape
    T_out = dz.shape[1]
    dw = np.zeros((k, C))
    for j in range(k):
        lo, hi = max(0, P - j * d), min(T_out, T + P - j * d)
        if lo < hi:
            dw[j] = (dz[:, lo:hi] * x[:, lo - P + j * d:hi - P + j * d]).sum(axis=(0, 1))
    return dw


def poison(*shapes):
    """Leave NaN-filled blocks of these sizes in torch's caching allocator: outputs the kernels allocate next start as NaN, so a
    position a kernel fails to write shows."""
    bufs = [torch.full(s, float("nan"), device=DEV) for s in shapes]
    torch.cuda.synchronize()
    del bufs


def g64(key, shape):
    return wg.gen(key, shape).astype(np.float64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


CASES = [(B, T, C, k, d) for (B, T, C) in [(2, 11, 36), (3, 29, 260)] for k in (3, 5, 7) for d in (1, 2, 4, 8)] + [(2, 3, 36, 7, 8), (1, 1, 4, 3, 1)]


@pytest.mark.parametrize("B,T,C,k,d", CASES)
def test_dw_kernels_vs_fp64(B, T, C, k, d):
    tag = f"dwk.{B}.{T}.{C}.{k}.{d}"
    x, w = g64(tag + ".x", (B, T, C)), g64(tag + ".w", (k, C))
    bias, slope = g64(tag + ".b", (C,)), g64(tag + ".s", (C,)) * 0.25
    xd, wd = dev(x), dev(w)
    # eval: "same" padding, folded bias, PReLU
    P = (k - 1) * d // 2
    poison((B, T, C))
    (y,) = ops.tcn_dw(xd, [wd], d, pads=[P], t_outs=[T], biases=[dev(bias)], slopes=[dev(slope)])
    z = ref_fwd(x, w, d, P, T) + bias
    assert_close_rel(y.cpu().numpy(), np.where(z < 0, z * slope, z), rtol=2e-6, afloor=1e-6, what="eval forward")
    # train: full padded length, raw
    P, To = (k - 1) * d, T + (k - 1) * d
    poison((B, To, C))
    (z_,) = ops.tcn_dw(xd, [wd], d, pads=[P], t_outs=[To])
    assert_close_rel(z_.cpu().numpy(), ref_fwd(x, w, d, P, To), rtol=2e-6, afloor=1e-6, what="train forward")
    dz = g64(tag + ".dz", (B, To, C))
    poison((B, T, C))
    dx = ops.tcn_dw_dgrad([dev(dz)], [wd], d, pads=[P], T=T)
    assert_close_rel(dx.cpu().numpy(), ref_dgrad(dz, w, d, P, T), rtol=2e-6, afloor=1e-6, what="data gradient")
    poison((k, C))
    (dw,) = ops.tcn_dw_wgrad(xd, [dev(dz)], [k], d, pads=[P])
    assert_close_rel(dw.cpu().numpy(), ref_wgrad(x, dz, k, d, P), rtol=1e-6, afloor=1e-6, what="weight gradient")
    (dw2,) = ops.tcn_dw_wgrad(xd, [dev(dz)], [k], d, pads=[P])
    assert torch.equal(dw, dw2)                                   # fixed-order reduction: the same bits every time


@pytest.mark.parametrize("d", [1, 4])
def test_dw_kernels_three_branches_in_one_launch(d):
    B, T, C = 2, 13, 100
    ks = [3, 5, 7]
    x = g64(f"dwb.{d}.x", (B, T, C))
    ws = [g64(f"dwb.{d}.w{k}", (k, C)) for k in ks]
    pads = [(k - 1) * d for k in ks]
    tos = [T + p for p in pads]
    zs = ops.tcn_dw(dev(x), [dev(w) for w in ws], d, pads=pads, t_outs=tos)
    for z, w, P, To in zip(zs, ws, pads, tos):
        assert_close_rel(z.cpu().numpy(), ref_fwd(x, w, d, P, To), rtol=2e-6, afloor=1e-6)
    dzs = [g64(f"dwb.{d}.dz{k}", (B, To, C)) for k, To in zip(ks, tos)]
    dx = ops.tcn_dw_dgrad([dev(g) for g in dzs], [dev(w) for w in ws], d, pads=pads, T=T)
    want = sum(ref_dgrad(g, w, d, P, T) for g, w, P in zip(dzs, ws, pads))
    assert_close_rel(dx.cpu().numpy(), want, rtol=2e-6, afloor=1e-6)
    dws = ops.tcn_dw_wgrad(dev(x), [dev(g) for g in dzs], ks, d, pads=pads)
    for dw, g, k, P in zip(dws, dzs, ks, pads):
        assert_close_rel(dw.cpu().numpy(), ref_wgrad(x, g, k, d, P), rtol=1e-6, afloor=1e-6)


def test_dw_kernels_refuse_bad_shapes():
    x = torch.zeros(2, 5, 6, device=DEV)
    with pytest.raises(ValueError):
        ops.tcn_dw(x, [torch.zeros(3, 6, device=DEV)], 1, pads=[1], t_outs=[5])
    x = torch.zeros(2, 5, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.tcn_dw(x, [torch.zeros(8, 3, device=DEV)], 1, pads=[1], t_outs=[5])          # weights must be tap-major [k, C]
    with pytest.raises(ValueError):
        ops.tcn_dw_wgrad(torch.zeros(2, 5, 6, device=DEV), [torch.zeros(2, 7, 6, device=DEV)], [3], 1, pads=[2])
    with pytest.raises(ValueError):
        ops.tcn_dw_dgrad([torch.zeros(2, 7, 6, device=DEV)], [torch.zeros(3, 6, device=DEV)], 1, pads=[2], T=5)


# ---------------------------------------------------------------------------------------------------------------------------------
# eval heads and models against the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def loaded_head(v):
    h = make_head(v)
    sd = fill({k: tuple(t.shape) for k, t in h.state_dict().items()}, f"tcn_heads.{v}.")
    h.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, strict=True)
    return h.to(DEV).eval()


@pytest.mark.parametrize("v", list(VARIANTS))
def test_head_logits_and_blocks_match_reference(gold, v):
    from deeplip_amd.video import _cached_pack
    cin = VARIANTS[v][4]
    h = loaded_head(v)
    x = torch.from_numpy(wg.gen(f"tcn_heads.x.{cin}", (2, 8, cin))).to(DEV)
    lengths = [int(l) for l in gold["lengths"]]
    want = gold[f"logits_{v}"]
    for mode in ("f32", "f16x3", "auto"):
        arith.configure(mode)
        with torch.no_grad():
            got = h(x, lengths, 2).cpu().numpy()
        assert_close_rel(got, want, what=f"{v} {mode}")
        assert (got.argmax(1) == want.argmax(1)).all()
    arith.configure("f32")
    blocks = h.tcn_trunk.network if hasattr(h, "tcn_trunk") else h.mb_ms_tcn.network
    p = _cached_pack(h, DEV, h.pack)
    y = x
    with torch.no_grad():
        for i, (b, bp) in enumerate(zip(blocks, p["blocks"])):
            y = b.run(y, bp)
            assert_close_rel(y.cpu().numpy(), gold[f"block{i}_{v}"], what=f"{v} block {i}")


def make_model(name):
    from deeplip_amd.video import Lipreading
    bb, w, dwpw = {"resnet_k3": ("resnet", 1.0, False), "shufflenet0p5_k3_dwpw": ("shufflenet", 0.5, True)}[name]
    net = Lipreading(hidden_dim=256, backbone_type=bb, num_classes=54, relu_type="prelu", tcn_options=opts([3], dwpw), width_mult=w)
    sd = fill({k: tuple(t.shape) for k, t in net.state_dict().items()}, f"tcn_heads.model.{name}.")
    net.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, strict=True)
    return net.to(DEV).eval()


@pytest.mark.parametrize("name", ["resnet_k3", "shufflenet0p5_k3_dwpw"])
def test_whole_model_logits_match_reference(gold, name):
    net = make_model(name)
    x = torch.from_numpy(wg.video_input(2, frames=5, key="tcn_heads.video")).to(DEV)
    lengths = [int(l) for l in gold["model_lengths"]]
    want = gold[f"model_logits_{name}"]
    for mode in ("f32", "auto"):
        arith.configure(mode)
        with torch.no_grad():
            got = net(x, lengths).cpu().numpy()
        assert_close_rel(got, want, what=f"{name} {mode}")
        assert (got.argmax(1) == want.argmax(1)).all()


@pytest.mark.parametrize("name", ["resnet_k3", "shufflenet0p5_k3_dwpw"])
def test_eval_step_plan_replays_the_eager_forward(name):
    from deeplip_amd.plan import StepPlan
    arith.configure("f32")
    net = make_model(name)
    ln = torch.tensor([6, 4], dtype=torch.int32, device=DEV)
    x = torch.from_numpy(wg.video_input(2, frames=6, key="tcn_heads.plan")).to(DEV)
    with torch.no_grad():
        plan = StepPlan(lambda v: net(v, ln), x.clone())
        x2 = torch.from_numpy(wg.video_input(2, frames=6, key="tcn_heads.plan2")).to(DEV)
        out = plan(x2)
        got = (out[0] if isinstance(out, (list, tuple)) else out).clone()
        torch.cuda.synchronize()
        want = net(x2, ln)
    assert torch.equal(got, want)
    plan.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------------------
def train_head(name):
    from deeplip_amd.video import TCN, MultiscaleMultibranchTCN
    ks, dwpw, cin, chans = TRAIN[name]
    cls = TCN if len(ks) == 1 else MultiscaleMultibranchTCN
    h = cls(input_size=cin, num_channels=chans, num_classes=TRAIN_CLASSES, tcn_options=opts(ks, dwpw, layers=len(chans), dropout=0.0),
            dropout=0.0, relu_type="prelu", dwpw=dwpw)
    sd = fill({k: tuple(t.shape) for k, t in h.state_dict().items()}, f"tcn_heads.train.{name}.")
    h.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, strict=True)
    return h.to(DEV).train()


def head_loss(h, x, ln, G):
    from deeplip_amd import autograd_video as av
    av.prepare_weights(h)
    return (h.forward_train(x, ln, 0.0) * G).sum()


@pytest.mark.parametrize("name", list(TRAIN))
def test_train_step_matches_reference(gold, name):
    h = train_head(name)
    cin = TRAIN[name][2]
    x = torch.from_numpy(wg.gen(f"tcn_heads.train.x.{name}", (TRAIN_B, TRAIN_T, cin))).to(DEV)
    ln = torch.from_numpy(gold["train_lengths"]).to(DEV)
    G = torch.from_numpy(gold["train_G"]).to(DEV)
    before = {k: v.clone() for k, v in h.state_dict().items() if k.endswith("running_var")}
    loss = head_loss(h, x, ln, G)
    loss.backward()
    assert abs(float(loss.detach()) - float(gold[f"train_{name}_loss"])) <= 1e-4 * max(1.0, abs(float(gold[f"train_{name}_loss"])))
    n = 0
    for pn, p in h.named_parameters():
        want = gold[f"train_{name}.grad.{pn}"]
        got = p.grad.detach().cpu().numpy()
        if np.abs(want).max() < 1e-5:            # a bias in front of a BatchNorm: its true gradient is zero, both sides hold rounding noise
            assert np.abs(got).max() < 1e-4, pn
        else:
            assert rel_err(got, want) < 1e-4, pn
        n += 1
    assert n == len([k for k in gold.files if k.startswith(f"train_{name}.grad.")])
    for bn, b in h.named_buffers():
        if bn.endswith("running_mean") or bn.endswith("running_var"):
            assert rel_err(b.cpu().numpy(), gold[f"train_{name}.buf.{bn}"]) < 1e-4, bn
    assert all(not torch.equal(before[k], h.state_dict()[k]) for k in before)


@pytest.mark.parametrize("name", ["k3", "k357_dwpw"])
def test_recorded_train_step_is_bit_identical_to_eager(name):
    from deeplip_amd.train_plan import TrainStepGraph
    cin = TRAIN[name][2]

    def run(graph):
        h = train_head(name)
        opt = torch.optim.Adam(h.parameters(), lr=torch.tensor(3e-4, device=DEV), capturable=True, fused=True)
        G = torch.from_numpy(wg.gen("tcn_heads.train.G", (TRAIN_B, TRAIN_CLASSES))).to(DEV)

        def one(xb, ln):
            opt.zero_grad(set_to_none=True)
            l = head_loss(h, xb, ln, G)
            l.backward()
            opt.step()
            return l

        plan = TrainStepGraph(one, eager_steps=1) if graph else None
        losses = []
        for i in range(4):
            x = torch.from_numpy(wg.gen(f"tcn_heads.tsg.{i}", (TRAIN_B, TRAIN_T, cin))).to(DEV)
            ln = torch.tensor([TRAIN_T - (j + i) % 3 for j in range(TRAIN_B)], dtype=torch.int32, device=DEV)
            l = plan.step(x, ln) if graph else one(x, ln)
            losses.append(float(l.detach()))
        if graph:
            plan.finish()
            assert plan.recorded
        torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in h.state_dict().items()}

    le, se = run(False)
    lg, sg = run(True)
    assert le == lg
    for k in se:
        assert torch.equal(se[k], sg[k]), k


@pytest.mark.parametrize("ks,dwpw", [([3], True), ([3], False), ([3, 5, 7], True)])
def test_lipreading_trains_with_the_new_heads(ks, dwpw):
    from deeplip_amd import autograd as ag
    from deeplip_amd.video import Lipreading
    net = Lipreading(num_classes=54, relu_type="prelu", tcn_options=opts(ks, dwpw, dropout=0.2))
    sd = fill({k: tuple(v.shape) for k, v in net.state_dict().items()}, "tcn_heads.lip.")
    net.load_state_dict({k: torch.from_numpy(a) for k, a in sd.items()}, strict=True)
    net.to(DEV).train()
    x = torch.from_numpy(wg.video_input(2, frames=7, key="tcn_heads.lip")).to(DEV)
    loss = ag.margin_ce_loss(net(x, lengths=[7, 5]), torch.tensor([1, 2], device=DEV))
    loss.backward()
    assert np.isfinite(float(loss.detach()))
    grads = [p.grad for p in net.tcn.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert all(int(v) == 1 for k, v in net.state_dict().items() if k.startswith("tcn.") and k.endswith("num_batches_tracked"))


def test_train_video_entry_point_with_dwpw_config(tmp_path):
    import train_video
    cfg = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conf", "video_config.json")))
    cfg.update({"tcn_kernel_size": [3], "tcn_dwpw": True})
    path = tmp_path / "k3_dwpw.json"
    path.write_text(json.dumps(cfg))
    for extra in ([], ["--eager-step"]):
        loss, shape = train_video.main(["--config-path", str(path), "--save-path", str(tmp_path / ("ck" + "".join(extra))),
                                        "--steps", "3", "--frames", "9"] + extra)
        assert np.isfinite(loss) and shape == (4, 54)
