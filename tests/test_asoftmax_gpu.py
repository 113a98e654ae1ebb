"""ASoftmax on the device (-m gpu): dlip_asoftmax_logits_f32 / dlip_row_norm_f32 and the criterion built on them against a restatement
of the definition (SphereFace, Liu et al. 2017) written here with torch on the CPU -- upstream has no implementation.

Bars.  The restatement runs in fp64 (the reference) and once more in fp32; the engine's distance from fp64 may be at most
max(project bar, 2 x the fp32 run's own distance), project bars 2e-5 for values and 1e-4 for gradients, each relative to the tensor's
largest magnitude.  Both distances are printed."""
import math

import numpy as np
import pytest
import torch

from deeplip_amd import weightgen as wg

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_VALUE, BAR_GRAD = 2e-5, 1e-4
LAMBDAS = (0.0, 5.0, 1000.0)
EPS = 1e-12                                                         # the clamp of dlip_l2_normalize_f32 as the criteria call it


def cuts(m):
    return [math.cos(j * math.pi / m) for j in range(1, m)]


def psi(c, m):
    """psi(c) = (-1)^k T_m(c) - 2k on c clamped to [-1, 1], k = #{ j in 1 .. m-1 : c <= cos(j pi / m) }."""
    c = c.clamp(-1, 1)
    k = torch.zeros_like(c)
    for t in cuts(m):
        k = k + (c.detach() <= t).to(c.dtype)
    T = {1: c, 2: 2 * c ** 2 - 1, 3: 4 * c ** 3 - 3 * c, 4: 8 * c ** 4 - 8 * c ** 2 + 1}[m]
    return c, (1 - 2 * (k % 2)) * T - 2 * k


def z_of(c, r, labels, m, lam):
    """The logits the cross-entropy sees, from cosines c [B,K] and norms r [B]."""
    cy, p = psi(c.gather(1, labels[:, None])[:, 0], m)
    zy = r * (lam * cy + p) / (1 + lam)
    return (r[:, None] * c).scatter(1, labels[:, None], zy[:, None])


def restate(x, W, labels, m, lam, dtype):
    """(loss, dX, dW) of the criterion in ``dtype`` on the CPU."""
    x = x.to(dtype).clone().requires_grad_()
    W = W.to(dtype).clone().requires_grad_()
    r = x.norm(dim=1).clamp_min(EPS)
    c = (x / r[:, None]) @ (W / W.norm(dim=1, keepdim=True).clamp_min(EPS)).T
    loss = torch.nn.functional.cross_entropy(z_of(c, r, labels, m, lam), labels)
    loss.backward()
    return float(loss.detach()), x.grad.double().numpy(), W.grad.double().numpy()


def rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(scale if scale is not None else np.abs(b).max(), 1e-30))


def crit_on(W, m, lam):
    from models.audio_models.loss import ASoftmax
    crit = ASoftmax(W.shape[1], W.shape[0], m=m).to(DEV)
    with torch.no_grad():
        crit.weights.copy_(W.to(DEV))
    crit.set_lambda(lam)
    return crit


def engine(x, W, labels, m, lam):
    crit = crit_on(W, m, lam)
    xg = x.to(DEV).requires_grad_()
    loss, logits = crit(xg, labels.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), xg.grad.cpu().numpy(), crit.weights.grad.cpu().numpy(), logits.detach().cpu()


def inputs(B, K, E, tag=""):
    x = torch.from_numpy(wg.gen(f"asoftmax.{tag}x.{B}.{K}.{E}", (B, E)))
    W = torch.from_numpy(wg.gen(f"asoftmax.{tag}w.{B}.{K}.{E}", (K, E)))
    labels = torch.from_numpy(np.minimum((wg.gen(f"asoftmax.{tag}labels.{B}.{K}.{E}", (B,), kind="uniform") * K).astype(np.int64), K - 1))
    return x, W, labels


def check_against_fp64(x, W, labels, m, lam, what):
    l64, dx64, dw64 = restate(x, W, labels, m, lam, torch.float64)
    l32, dx32, dw32 = restate(x, W, labels, m, lam, torch.float32)
    loss, dx, dw, _ = engine(x, W, labels, m, lam)
    assert np.isfinite(loss) and np.isfinite(dx).all() and np.isfinite(dw).all()
    own = (abs(l32 - l64) / abs(l64), rel(dx32, dx64), rel(dw32, dw64))
    got = (abs(loss - l64) / abs(l64), rel(dx, dx64), rel(dw, dw64))
    bars = (max(BAR_VALUE, 2 * own[0]), max(BAR_GRAD, 2 * own[1]), max(BAR_GRAD, 2 * own[2]))
    print(f"{what} m {m} lambda {lam:g}: loss {got[0]:.2e} (fp32 {own[0]:.2e}), dX {got[1]:.2e} (fp32 {own[1]:.2e}), dW {got[2]:.2e} (fp32 {own[2]:.2e})")
    assert got[0] <= bars[0] and got[1] <= bars[1] and got[2] <= bars[2], (got, bars)


# (5, 300, 16): more columns than one 256-wide step of the workgroup, and no multiple of it
@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("B,K,E", [(32, 57, 64), (7, 3, 4), (1, 2, 8), (5, 300, 16)])
def test_value_and_gradients_match_fp64(B, K, E, m):
    x, W, labels = inputs(B, K, E)
    for lam in LAMBDAS:
        check_against_fp64(x, W, labels, m, lam, f"({B},{K},{E})")


@pytest.mark.parametrize("lam", LAMBDAS)
def test_m1_is_cross_entropy_on_r_times_cosine(lam):
    """m = 1: psi(c) = c, so the loss is CE(r c) -- built here from the ops that existed before."""
    from deeplip_amd import autograd as ag
    x, W, labels = inputs(32, 57, 64)
    loss, dx, dw, _ = engine(x, W, labels, 1, lam)
    xg, wg_ = x.to(DEV).requires_grad_(), W.to(DEV).requires_grad_()
    c = ag.linear(ag.l2_normalize(xg), ag.l2_normalize(wg_))
    r = torch.sqrt((xg * xg).sum(dim=1)).clamp_min(EPS)
    ref = ag.margin_ce_loss(r[:, None] * c, labels.to(DEV), 1.0, 0.0)
    ref.backward()
    ref = float(ref.detach())
    e = (abs(loss - ref) / abs(ref), rel(dx, xg.grad.cpu().numpy()), rel(dw, wg_.grad.cpu().numpy()))
    print(f"m 1 lambda {lam:g} vs CE(r c) from the existing ops: loss {e[0]:.2e}, dX {e[1]:.2e}, dW {e[2]:.2e}")
    assert e[0] <= BAR_VALUE and e[1] <= BAR_GRAD and e[2] <= BAR_GRAD


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_target_cosine_at_plus_and_minus_one_and_a_row_at_the_clamp(m):
    x, W, labels = inputs(8, 5, 16, tag="rows.")
    x = x.clone()
    x[0] = W[labels[0]]                      # cos = +1
    x[1] = -W[labels[1]]                     # cos = -1
    x[2] = 2.5 * W[labels[2]]
    x[3] = 0.0                               # the norm sits at the clamp
    for lam in LAMBDAS:
        check_against_fp64(x, W, labels, m, lam, "constructed rows")
    _, _, _, logits = engine(x, W, labels, m, 5.0)
    assert abs(float(logits[0, labels[0]]) - 1) <= 1e-6 and abs(float(logits[1, labels[1]]) + 1) <= 1e-6 and bool((logits[3] == 0).all())


@pytest.mark.parametrize("m", [2, 3, 4])
def test_branch_points_to_one_ulp_either_side(m):
    """The launches themselves on constructed cosines: the target at every cos(j pi / m), one fp32 ulp below and above, at +-1 and one
    ulp outside [-1, 1]; a row whose norm is the clamp gets dr = 0.  z, dc and dr against the fp64 restatement of the same function."""
    from deeplip_amd import autograd as ag
    pts = []
    for t in cuts(m) + [1.0, -1.0]:
        f = np.float32(t)
        pts += [f, np.nextafter(f, np.float32(-2)), np.nextafter(f, np.float32(2))]
    B, K = len(pts), 7
    g = torch.Generator().manual_seed(m)
    c = torch.rand(B, K, generator=g) * 1.6 - 0.8
    labels = torch.arange(B) % K
    c[torch.arange(B), labels] = torch.from_numpy(np.asarray(pts, dtype=np.float32))
    r = torch.rand(B, generator=g) * 3 + 0.5
    r[-1] = EPS
    dz = torch.randn(B, K, generator=g)
    for lam in LAMBDAS:
        lam_t = torch.full((1,), lam, device=DEV)
        cg, rg = c.to(DEV).requires_grad_(), r.to(DEV).requires_grad_()
        z = ag.asoftmax_logits(cg, rg, labels.to(DEV), lam_t, m)
        z.backward(dz.to(DEV))
        outs = {}
        for dt in (torch.float64, torch.float32):
            cc, rr = c.clone().to(dt).requires_grad_(), r.clone().to(dt).requires_grad_()
            zz = z_of(cc, rr, labels, m, lam)
            zz.backward(dz.to(dt))
            dr = rr.grad.clone()
            dr[-1] = 0                      # the clamp's derivative: r is the OUTPUT of a clamp there
            outs[dt] = (zz.detach().double().numpy(), cc.grad.double().numpy(), dr.double().numpy())
        got = (z.detach().cpu().numpy(), cg.grad.cpu().numpy(), rg.grad.cpu().numpy())
        assert all(np.isfinite(t).all() for t in got) and got[2][-1] == 0.0
        for name, a, w64, w32, bar in zip(("z", "dc", "dr"), got, outs[torch.float64], outs[torch.float32], (BAR_VALUE, BAR_GRAD, BAR_GRAD)):
            e, own = rel(a, w64), rel(w32, w64)
            print(f"m {m} lambda {lam:g} {name}: {e:.2e} (fp32 {own:.2e})")
            assert e <= max(bar, 2 * own), (name, e, own)


def test_int32_and_int64_labels_agree():
    x, W, labels = inputs(32, 57, 64)
    outs = []
    for dt in (torch.int64, torch.int32):
        crit = crit_on(W, 4, 5.0)
        xg = x.to(DEV).requires_grad_()
        loss, _ = crit(xg, labels.to(DEV).to(dt))
        loss.backward()
        with torch.no_grad():
            l2, _ = crit(x.to(DEV), labels.to(DEV).to(dt))
        outs.append((float(loss.detach()), float(l2), xg.grad.clone(), crit.weights.grad.clone()))
    assert outs[0][:2] == outs[1][:2] and torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][3], outs[1][3])
    assert abs(outs[0][0] - outs[0][1]) <= BAR_VALUE * abs(outs[0][0])          # the no-grad path: the same loss to rounding


def test_predict_returns_loss_cosine_logits_and_argmax():
    x, W, labels = inputs(32, 57, 64)
    crit = crit_on(W, 3, 5.0)
    loss, logits, amax = crit.predict(x.to(DEV), labels.to(DEV))
    l64, _, _ = restate(x, W, labels, 3, 5.0, torch.float64)
    assert abs(float(loss) - l64) <= BAR_VALUE * abs(l64) and torch.equal(amax, logits.argmax(dim=1)) and float(logits.abs().max()) <= 1 + 1e-6
    assert crit.predict(x.to(DEV))[0] is None


def test_recorded_step_follows_lambda_written_between_replays():
    """A recorded step replayed at two further lambda values written by set_lambda: every replay is bit-identical to the eager call at
    that lambda -- the kernels read lambda from the device, the step is not recorded again."""
    from deeplip_amd.train_plan import TrainStepGraph
    x, W, labels = inputs(32, 57, 64)
    lams = (1000.0, 1000.0, 5.0, 0.25)

    def run(recorded):
        crit = crit_on(W, 4, lams[0])
        opt = torch.optim.SGD(crit.parameters(), lr=torch.tensor(0.05, device=DEV), momentum=0.9, fused=True)

        def one(xb, lab):
            opt.zero_grad(set_to_none=True)
            xg = xb.detach().requires_grad_()
            loss, _ = crit(xg, lab)
            loss.backward()
            opt.step()
            return loss, xg.grad
        plan = TrainStepGraph(one, eager_steps=1 if recorded else 10 ** 6, device=torch.device(DEV), branch_streams=False, verify=False)
        outs = []
        for i, lam in enumerate(lams):
            crit.set_lambda(lam)
            loss, dx = plan.step(x.to(DEV) * (1 + 0.1 * i), labels.to(DEV))
            plan.finish()
            outs.append((float(loss.detach()), dx.clone().cpu()))
        assert plan.recorded == recorded
        return outs, crit.weights.detach().cpu().clone()

    o_g, w_g = run(True)
    o_e, w_e = run(False)
    for (lg, dg), (le, de) in zip(o_g, o_e):
        assert lg == le and torch.equal(dg, de)
    assert torch.equal(w_g, w_e)
    # ... and lambda matters: the same batch at the last two lambdas gives different losses
    l5 = engine(x * 1.3, W, labels, 4, 5.0)[0]
    l025 = engine(x * 1.3, W, labels, 4, 0.25)[0]
    assert l5 != l025


OV = {"data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 200, "data.trial_targets": 40, "data.audio_frames": 120,
      "data.n_spk": 6, "data.utt_per_spk": 3, "train.bs": 16, "train.epoch": 2, "train.steps_per_epoch": 3}       # test_triplet_gpu.py's


def _train(tmp_path, monkeypatch, loss, probe=lambda tr: None):
    """(epoch statistics, probe(trainer)) of a two-epoch run.  A trainer and its recorded steps point at each other, so a dead one waits
    for Python's cyclic collector, and a recorded graph destroyed by the collector INSIDE a later capture aborts the process: the dead
    ones go here, outside any capture, before the next trainer is built and after this one is done."""
    import gc
    import train_audio
    gc.collect()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tr = train_audio.Trainer(overrides={**OV, "train.loss": loss}, arith_mode="f32")
    tr._train()
    out = (tr.last_epoch_stats, probe(tr))
    del tr
    gc.collect()
    return out


def test_train_audio_with_asoftmax(tmp_path, monkeypatch):
    from models.audio_models.loss import ASoftmax

    def probe(tr):
        crit = tr.criterion
        return {"class": type(crit), "it": crit.it, "lam": float(crit.lam), "want": crit.schedule(crit.it), "groups": len(tr.optim.param_groups),
                "crit_params": [tuple(p.shape) for p in tr.optim.param_groups[1]["params"]], "weights": tuple(crit.weights.shape)}
    st, got = _train(tmp_path, monkeypatch, "ASoftmax", probe)
    st_l, _ = _train(tmp_path, monkeypatch, "LMCL")
    assert got["class"] is ASoftmax and np.isfinite(st["loss"]) and "acc" in st
    assert st["step_mode"] == st_l["step_mode"] == "graph"
    assert got["it"] == 6                                               # two epochs of three steps: one anneal() per step
    assert got["lam"] == float(np.float32(got["want"])) and got["want"] == pytest.approx(1000.0 / 1.72, rel=1e-12)
    assert got["groups"] == 2 and got["crit_params"] == [got["weights"]]
