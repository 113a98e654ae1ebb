"""``arch: ftdnn`` on the GPU (-m gpu) against tests/ftdnn_ref.py, the fp64 restatement of its definition: the
semi-orthogonal step kernel and its device-side schedule, the factorized block and the encoder in eval mode under the three
arithmetic modes (ragged rows bit-identical to rows run alone), the training path's outputs and gradients under both TRAIN_CONV
modes, an SGD trajectory with the constraint applied, the recorded step of train_audio.Trainer and the entry point itself.

Bars are the project's: 2e-5 of the tensor's largest magnitude on outputs (and on the matrices the step rewrites), 1e-4 on gradients
(tests/test_train_f32_gpu.py), 1e-6 between a recorded and an eager trajectory (tests/test_train_plan_gpu.py)."""
import functools
import gc
import os
import re

import numpy as np
import pytest
import torch

import ftdnn_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR_OUT, BAR_GRAD, BAR_REPLAY = 2e-5, 1e-4, 1e-6


@pytest.fixture(autouse=True)
def _clean_status():
    from deeplip_amd import _lib
    torch.cuda.synchronize()
    _lib.status_words().zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_words().zero_()


def _f32(a):
    return np.asarray(a, dtype=np.float32)


# ---- the semi-orthogonal step kernel -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _step_inputs():
    """The table of the issue: 8 x 24, 12 x 36 (rows no tile multiple, cols no multiple of 32), 24 x 24 (the square edge: Bn = 24, Cin = 8,
    k = 3), 128 x 1536 (several K-splits) and a converged matrix -- as fp32 values, which both sides start from."""
    mats = [ref.uniform_matrix(8, 24, 1), ref.uniform_matrix(12, 36, 3), ref.uniform_matrix(24, 24, 4), ref.uniform_matrix(128, 1536, 2),
            ref.converged_matrix(8, 24, 1)]
    return tuple(_f32(m) for m in mats)


@functools.lru_cache(maxsize=None)
def _step_reference(steps):
    """[step][matrix] fp64 trajectories; asserts -- a condition on the INPUTS -- that no ratio met on the way lies within 1e-3 of a nu
    branch point, so that fp32 cannot take another branch than fp64."""
    cur = [m.astype(np.float64) for m in _step_inputs()]
    out = []
    for s in range(steps):
        for i, m in enumerate(cur):
            ratio = ref.semi_orth_quantities(m)[4]
            assert abs(ratio - 1.02) >= 1e-3 and abs(ratio - 1.1) >= 1e-3, (s, i, ratio)
        cur = [ref.semi_orth_step(m) for m in cur]
        out.append(cur)
    return out


def _launch(mats_np, every, calls, counter0=0):
    from deeplip_amd import ops
    mats = [torch.from_numpy(m.copy()).to(DEV) for m in mats_np]
    tab, max_rows, max_cols = ops.semi_orth_table(mats)
    ws = ops.semi_orth_workspace(len(mats), DEV)
    counter = torch.tensor([counter0, 0], dtype=torch.int32, device=DEV)
    snaps = []
    for _ in range(calls):
        ops.semi_orth_step(tab, len(mats), max_rows, max_cols, counter, every, ws)
        snaps.append([m.clone() for m in mats])
    torch.cuda.synchronize()
    return [[m.cpu().numpy() for m in s] for s in snaps], counter.cpu().tolist()


def test_semi_orth_step_kernel_against_the_reference():
    """ONE launch pair over the whole table, then the twelve-step trajectory; every matrix within 2e-5 of max|M| of fp64."""
    want = _step_reference(12)
    nus = sorted({ref.semi_orth_quantities(m.astype(np.float64))[5] for m in _step_inputs()})
    assert nus == [0.03125, 0.0625, 0.125]                               # the table takes all three nu branches in its first launch
    got, counter = _launch(_step_inputs(), 1, 12)
    assert counter[0] == 12
    worst = {1: 0.0, 12: 0.0}
    for s in (1, 12):
        for g, w in zip(got[s - 1], want[s - 1]):
            e = rel_err(g, w)
            worst[s] = max(worst[s], e)
            print(f"\nsemi-orth step {s}: {g.shape[0]} x {g.shape[1]} rel err {e:.3e}, defect {ref.semi_orth_defect(g):.3e}", end="")
    print(f"\nsemi-orth worst: one step {worst[1]:.3e}, twelve steps {worst[12]:.3e} (bar {BAR_OUT:.0e})")
    assert worst[1] < BAR_OUT and worst[12] < BAR_OUT


def test_semi_orth_step_is_reproducible():
    a, _ = _launch(_step_inputs(), 1, 2)
    b, _ = _launch(_step_inputs(), 1, 2)
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_semi_orth_schedule_lives_on_the_device():
    """every = 4, nine calls from counter 0: the matrices change on calls 4 and 8 alone -- bit-exactly nothing on the others -- and the
    counter ends at 9; every = 0 never changes them (and still counts)."""
    mats = _step_inputs()[:3]
    got, counter = _launch(mats, 4, 9)
    assert counter[0] == 9
    prev = list(mats)
    for call, snap in enumerate(got, start=1):
        changed = [not np.array_equal(a, b) for a, b in zip(snap, prev)]
        assert all(changed) if call in (4, 8) else not any(changed), (call, changed)
        prev = snap
    want = [ref.semi_orth_step(ref.semi_orth_step(m.astype(np.float64))) for m in mats]
    assert max(rel_err(g, w) for g, w in zip(got[8], want)) < BAR_OUT
    got, counter = _launch(mats, 0, 5)
    assert counter[0] == 5 and all(np.array_equal(a, b) for a, b in zip(got[4], mats))
    # a counter that starts elsewhere (a resumed run): due when counter + 1 is a multiple
    got, counter = _launch(mats, 4, 2, counter0=2)
    assert counter[0] == 4 and all(np.array_equal(a, b) for a, b in zip(got[0], mats)) and not any(np.array_equal(a, b) for a, b in zip(got[1], mats))


def test_semi_orth_refusals():
    from deeplip_amd import _lib, ops
    with pytest.raises(ValueError):
        ops.semi_orth_table([torch.zeros(132, 512, device=DEV)])         # more rows than P's LDS plan carries
    with pytest.raises(ValueError):
        ops.semi_orth_table([torch.zeros(8, 4, device=DEV)])             # rows > cols
    m = torch.zeros(8, 24, device=DEV)
    tab, mr, mc = ops.semi_orth_table([m])
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.DeepLipHipError):                            # a workspace that is too small
        ops.semi_orth_step(tab, 1, mr, mc, counter, 4, torch.zeros(256, dtype=torch.uint8, device=DEV))
    with pytest.raises(_lib.DeepLipHipError):
        ops.semi_orth_step(tab, 1, mr, mc, counter, -1, ops.semi_orth_workspace(1, DEV))
    torch.cuda.synchronize()
    assert counter.cpu().tolist() == [0, 0]


# ---- the block, eval mode --------------------------------------------------------------------------------------------------------------
def _rand_block(cin, cout, context, bn_first, seed=0):
    from deeplip_amd.audio import FTDNN_Block
    blk = FTDNN_Block(cin, cout, context, bottleneck_dim=8, bypass_scale=0.66, bn_first=bn_first)
    g = torch.Generator().manual_seed(100 + seed)
    with torch.no_grad():
        for name, p in blk.named_parameters():
            if name == "bn.weight":
                p.copy_(torch.rand(p.shape, generator=g) * 0.4 + 0.8)
            elif p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            else:
                p.copy_(torch.randn(p.shape, generator=g) / np.sqrt(p[0].numel()))
        blk.bn.running_mean.copy_(torch.randn(cout, generator=g) * 0.1)
        blk.bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    return blk


BLOCK_CASES = [(32, 32, (-2, 0, 2), True),            # bypass on
               (32, 64, (-2, 0, 2), True),            # widths differ: no bypass
               (32, 32, (-2, -1, 0, 1, 2), True),     # five taps
               (32, 32, (0,), True),                  # one tap (a layer listed explicitly in factorized_layers)
               (32, 32, (-2, 0, 2), False),           # conv -> LeakyReLU -> BN
               (32, 32, (-3, 0), True)]               # shift != centre


@functools.lru_cache(maxsize=None)
def _block_case(i):
    cin, cout, context, bn_first = BLOCK_CASES[i]
    blk = _rand_block(cin, cout, list(context), bn_first, seed=i)
    x = torch.randn(2, cin, 23, generator=torch.Generator().manual_seed(7 + i))
    with torch.no_grad():
        want = ref.ftdnn_block(x.double(), ref.to64(blk.state_dict()), "", list(context), 0.66, bn_first, False).numpy()
    return blk, x, want


@pytest.mark.parametrize("mode", ["f32", "f16x3", "auto"])
@pytest.mark.parametrize("case", range(len(BLOCK_CASES)))
def test_block_eval_parity(case, mode):
    from deeplip_amd import _lib, arith
    arith.configure(mode)
    blk, x, want = _block_case(case)
    cin, cout, context, bn_first = BLOCK_CASES[case]
    assert (blk.bypass_scale != 0.0) == (cin == cout) and blk.bypass_shift == -context[0]
    blk = blk.eval().to(DEV)
    with torch.no_grad():
        y = blk(x.to(DEV))
    _lib.check_range(sync=True)
    assert tuple(y.shape) == want.shape
    e = rel_err(y.cpu().numpy(), want)
    print(f"\nblock {BLOCK_CASES[case]} {mode}: rel err {e:.3e}")
    assert e < BAR_OUT
    # a row run alone, and alone at a shorter length, has the bits it has in the batch
    with torch.no_grad():
        y1 = blk(x[1:2].contiguous().to(DEV))
        y1s = blk(x[1:2, :, :17].contiguous().to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y1[0], y[1]) and torch.equal(y1s[0], y[1, :, :y1s.shape[2]])


# ---- the encoder, eval mode ------------------------------------------------------------------------------------------------------------
ENC_CONTEXTS = [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0]]


def _enc_cfg(hidden=(32, 32, 32, 64), factorized=None, bn_first=True):
    sec = {"input_dim": 24, "hidden_dim": list(hidden), "context": ENC_CONTEXTS, "tdnn_layers": 4, "fc_layers": 3, "embedding_dim": 16,
           "pooling": "statistic", "bn_first": bn_first, "bottleneck_dim": 8}
    if factorized is not None:
        sec["factorized_layers"] = list(factorized)
    return {"arch": "ftdnn", "ftdnn": sec}


def _encoder(hidden=(32, 32, 32, 64), factorized=None, bn_first=True):
    from deeplip_amd import trainer_common as tc, weightgen as wg
    m = tc.build_speech_encoder(_enc_cfg(hidden, factorized, bn_first))
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, prefix="audio.")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m


def _enc_ref(m, x, training, factorized=(1, 2), grad=False):
    p = ref.to64(m.state_dict(), grad=grad)
    return p, ref.encoder(x, p, ENC_CONTEXTS, set(factorized), 0.66, m.bn_first, training)


@pytest.mark.parametrize("mode", ["f32", "f16x3", "auto"])
def test_encoder_eval_parity_and_ragged_rows(mode):
    from deeplip_amd import _lib, arith, trainer_common as tc, weightgen as wg
    arith.configure(mode)
    m = _encoder().eval().to(DEV)
    T, lo = 41, tc.encoder_min_frames(m)
    assert lo == 16
    x = torch.from_numpy(wg.audio_input(2, 24, T, key="ftdnn.eval"))
    with torch.no_grad():
        xv, xa = m.extract_embedding(x.to(DEV))
        _, (wv, wa) = _enc_ref(m, x.double(), False)
    _lib.check_range(sync=True)
    ev, ea = rel_err(xv.cpu().numpy(), wv.numpy()), rel_err(xa.cpu().numpy(), wa.numpy())
    print(f"\nencoder eval {mode}: xv {ev:.3e}, x_a {ea:.3e}")
    assert ev < BAR_OUT and ea < BAR_OUT
    # ragged: lengths [T, min_frames]; each row bit-identical to the row run alone
    xr = x.clone()
    xr[1, :, lo:] = 0.0
    with torch.no_grad():
        rv, ra = m.extract_embedding(xr.to(DEV), lengths=[T, lo])
        alone = [m.extract_embedding(xr[b:b + 1, :, :n].contiguous().to(DEV)) for b, n in ((0, T), (1, lo))]
    _lib.check_range(sync=True)
    for b in range(2):
        print(f"\nragged row {b} vs alone ({mode}): max |xv diff| {float((rv[b] - alone[b][0][0]).abs().max()):.3e}, "
              f"max |x_a diff| {float((ra[b] - alone[b][1][0]).abs().max()):.3e}", end="")
    for b in range(2):
        assert torch.equal(rv[b], alone[b][0][0]) and torch.equal(ra[b], alone[b][1][0]), b
    assert torch.equal(rv[0], xv[0])


# ---- training ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conv", ["f16x3", "f32"])
@pytest.mark.parametrize("case", [0, 1, 4, 5])
def test_block_train_gradients(case, conv):
    """Output and the gradients of the input and of every parameter of one block against fp64 autograd, both TRAIN_CONV modes."""
    from deeplip_amd import autograd as ag, autograd_video as av
    av.TRAIN_CONV = conv
    cin, cout, context, bn_first = BLOCK_CASES[case]
    blk = _rand_block(cin, cout, list(context), bn_first, seed=20 + case).to(DEV).train()
    B, T = 4, 23
    x = torch.randn(B, cin, T, generator=torch.Generator().manual_seed(31 + case))
    p = ref.to64(blk.state_dict(), grad=True)
    x64 = x.double().requires_grad_()
    want = ref.ftdnn_block(x64, p, "", list(context), 0.66, bn_first, True)
    dy = torch.randn(want.shape, generator=torch.Generator().manual_seed(41 + case))
    want.backward(dy.double())
    xg = x.permute(0, 2, 1).contiguous().to(DEV).requires_grad_()
    y, pend = ag.ftdnn_block_train(xg, blk, None, False)
    assert pend is None
    y.backward(dy.permute(0, 2, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    errs = {"y": rel_err(y.detach().cpu().permute(0, 2, 1).numpy(), want.detach().numpy()),
            "dx": rel_err(xg.grad.cpu().permute(0, 2, 1).numpy(), x64.grad.numpy())}
    for name, q in blk.named_parameters():
        if name == "context_layer.bias" and bn_first:
            # the bias sits right in front of a batch-statistics BatchNorm: its gradient is zero up to rounding on both sides
            assert float(q.grad.abs().max()) < 1e-4 * float(dy.abs().sum() / cout) + 1e-5
            continue
        errs["d " + name] = rel_err(q.grad.cpu().numpy(), p[name].grad.numpy())
    print(f"\nblock train {BLOCK_CASES[case]} {conv}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs.pop("y") < BAR_OUT
    assert all(v < BAR_GRAD for v in errs.values()), errs


ENC_TRAIN = [((32, 32, 32, 64), (1, 2)),            # two bypass blocks between plain ones (the last pooled on load)
             ((32, 64, 64, 64), (1, 2, 3))]         # a block without a bypass hands its BatchNorm over on load; a factorized last layer


@pytest.mark.parametrize("conv", ["f16x3", "f32"])
@pytest.mark.parametrize("hidden,factorized", ENC_TRAIN)
def test_encoder_train_gradients(hidden, factorized, conv):
    from deeplip_amd import autograd_video as av, weightgen as wg
    av.TRAIN_CONV = conv
    m = _encoder(hidden, factorized).to(DEV).train()
    x = torch.from_numpy(wg.audio_input(8, 24, 40, key="ftdnn.train"))
    g = torch.Generator().manual_seed(5)
    gv, ga = torch.randn(8, 16, generator=g), torch.randn(8, 16, generator=g)
    p, (wv, wa) = _enc_ref(m, x.double(), True, factorized, grad=True)
    torch.autograd.backward([wv, wa], [gv.double(), ga.double()])
    xv, xa = m.extract_embedding(x.to(DEV))
    torch.autograd.backward([xv, xa], [gv.to(DEV), ga.to(DEV)])
    torch.cuda.synchronize()
    ev, ea = rel_err(xv.detach().cpu().numpy(), wv.detach().numpy()), rel_err(xa.detach().cpu().numpy(), wa.detach().numpy())
    errs = {}
    for name, q in m.named_parameters():
        if q.grad is None:                  # bn2 sits behind extract_embedding (tdnn.py:103-111): no gradient on either side
            assert p[name].grad is None and name.startswith("bn2."), name
            continue
        if name.startswith("tdnn.") and name.endswith("context_layer.bias"):
            assert float(q.grad.abs().max()) < 1e-4 * float(p[name.replace("context_layer.bias", "bn.bias")].grad.abs().max()) + 1e-5, name
            continue
        errs[name] = rel_err(q.grad.cpu().numpy(), p[name].grad.numpy())
    worst = max(errs, key=errs.get)
    print(f"\nencoder train {hidden} {factorized} {conv}: xv {ev:.2e}, x_a {ea:.2e}, worst gradient {worst} {errs[worst]:.2e}")
    assert ev < BAR_OUT and ea < BAR_OUT
    assert errs[worst] < BAR_GRAD, errs


def test_two_sgd_steps_with_the_constraint_follow_the_fp64_trajectory():
    """SGD, then the semi-orthogonal step on every factor (semi_orth_every = 1), twice, against the same in fp64.  (At this learning
    rate an SGD step moves a factor by more than one application of the constraint contracts it -- the defects printed below grow in
    the reference too; the test is about the trajectory, the recorded-step test below about the defect.)"""
    from deeplip_amd import weightgen as wg
    from deeplip_amd.audio import SemiOrthStep
    lr = 0.05
    m = _encoder().to(DEV).train()
    p = ref.to64(m.state_dict(), grad=True)
    opt = torch.optim.SGD(m.parameters(), lr=lr)
    so = SemiOrthStep(m, 1)
    d0 = [ref.semi_orth_defect(w.detach().cpu().numpy().reshape(w.shape[0], -1)) for w in so.matrices()]
    g = torch.Generator().manual_seed(9)
    for step in range(2):
        x = torch.from_numpy(wg.audio_input(8, 24, 40, key=f"ftdnn.sgd{step}"))
        gv, ga = torch.randn(8, 16, generator=g), torch.randn(8, 16, generator=g)
        opt.zero_grad(set_to_none=True)
        xv, xa = m.extract_embedding(x.to(DEV))
        torch.autograd.backward([xv, xa], [gv.to(DEV), ga.to(DEV)])
        opt.step()
        so()
        wv, wa = ref.encoder(x.double(), p, ENC_CONTEXTS, {1, 2}, 0.66, True, True)
        torch.autograd.backward([wv, wa], [gv.double(), ga.double()])
        with torch.no_grad():
            for k, t in p.items():
                if t.requires_grad and t.grad is not None:
                    t -= lr * t.grad
                    t.grad = None
                    if k.endswith("factor.weight"):
                        t.copy_(torch.from_numpy(ref.semi_orth_step(t.numpy().reshape(t.shape[0], -1)).reshape(tuple(t.shape))))
    torch.cuda.synchronize()
    assert so.counter.cpu().tolist()[0] == 2
    errs = {k: rel_err(q.detach().cpu().numpy(), p[k].detach().numpy()) for k, q in m.named_parameters()}
    worst = max(errs, key=errs.get)
    d2 = [ref.semi_orth_defect(w.detach().cpu().numpy().reshape(w.shape[0], -1)) for w in so.matrices()]
    print(f"\ntwo SGD steps: worst parameter {worst} {errs[worst]:.2e}; factor defects {d0} -> {d2}")
    assert errs[worst] < BAR_OUT, errs


# ---- the recorded step and the entry point -----------------------------------------------------------------------------------------------
# (the learning rate: at the config's 0.01 -- LMCL at scale 30, momentum 0.9 -- five steps move an 8 x 96 factor by about its own size
# (measured: defect 0.79 -> 1.39 over five steps with the constraint applied twice), which swamps two applications of a step that
# roughly halves the defect; at 1e-4 the optimizer's drift is two orders below what the constraint removes)
OV = {"data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 200, "data.trial_targets": 40, "data.audio_frames": 48,
      "data.n_spk": 6, "data.utt_per_spk": 3, "train.bs": 8, "train.epoch": 1, "train.steps_per_epoch": 4, "train.crop_frames": None,
      "train.sgd.init_lr": 1e-4,
      "train.semi_orth_every": 2, "model.arch": "ftdnn", "model.ftdnn.hidden_dim": [32, 32, 32, 32, 64], "model.ftdnn.embedding_dim": 16,
      "model.ftdnn.bottleneck_dim": 8}


def _defects(tr):
    return [ref.semi_orth_defect(w.detach().cpu().numpy().reshape(w.shape[0], -1)) for w in tr.semi_orth.matrices()]


def _train_five(tmp_path, monkeypatch, graph_step):
    """A trainer and its recorded steps point at each other; dead ones go here, outside any capture (tests/test_asoftmax_gpu.py)."""
    import train_audio
    gc.collect()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tr = train_audio.Trainer(overrides={**OV, "train.graph_step": graph_step}, arith_mode="f32")
    assert tr.semi_orth is not None and tr.semi_orth.every == 2 and tr.model.factorized_layers == (1, 2)
    d0 = _defects(tr)
    tr.current_epoch = 1
    tr._adjust_margin()
    tr._train_epoch()                              # steps 1 .. 4: the constraint is due on 2 and 4
    torch.cuda.synchronize()
    d4 = _defects(tr)
    tr.train_opts["steps_per_epoch"] = 1
    tr.current_epoch = 2
    tr._adjust_margin()
    loss = tr._train_epoch()                       # step 5 (the same shape and margin: the recorded step is replayed)
    torch.cuda.synchronize()
    params = {k: v.detach().cpu().clone() for k, v in list(tr.model.state_dict().items()) + [("crit." + k, v) for k, v in tr.criterion.state_dict().items()]}
    out = {"loss": loss, "mode": tr.last_epoch_stats["step_mode"], "params": params, "d0": d0, "d4": d4,
           "counter": tr.semi_orth.counter.cpu().tolist()[0]}
    # a checkpoint round trip restores the counter
    path = tr.save("net_ckpt.pth")
    tr.semi_orth.counter.zero_()
    tr.load(path)
    out["counter_loaded"] = tr.semi_orth.counter.cpu().tolist()[0]
    tr.close()
    del tr
    gc.collect()
    return out


def test_recorded_step_applies_the_constraint_on_the_eager_schedule(tmp_path, monkeypatch):
    """Five steps with semi_orth_every = 2, recorded (the first step eager, four replays) and eager: the same trajectory, the factors'
    defect after step 4 below that at step 0, the counter at 5 and back there after a checkpoint round trip."""
    g = _train_five(tmp_path, monkeypatch, True)
    e = _train_five(tmp_path, monkeypatch, False)
    assert g["mode"] == "graph" and e["mode"] == "eager"
    assert g["counter"] == e["counter"] == 5 and g["counter_loaded"] == e["counter_loaded"] == 5
    errs = {k: rel_err(g["params"][k].double().numpy(), v.double().numpy()) for k, v in e["params"].items() if v.is_floating_point() and v.numel()}
    worst = max(errs, key=errs.get)
    print(f"\nrecorded vs eager, five steps: loss {g['loss']!r} vs {e['loss']!r}; worst tensor {worst} {errs[worst]:.2e}; "
          f"factor defects {g['d0']} -> {g['d4']} after step 4")
    assert abs(g["loss"] - e["loss"]) <= BAR_REPLAY * abs(e["loss"])
    assert errs[worst] <= BAR_REPLAY, errs
    # steps 2 and 4 applied the constraint: the factors are closer to semi-orthogonal than they started
    assert all(b < a for a, b in zip(g["d0"], g["d4"])) and all(b < a for a, b in zip(e["d0"], e["d4"]))


def test_train_audio_entry_point_with_ftdnn(tmp_path, monkeypatch, capsys):
    """train_audio.py --mode train on the tiny synthetic config: trains, averages, extracts the ragged test list through RaggedExtractor
    and prints an EER."""
    import train_audio
    gc.collect()
    monkeypatch.chdir(tmp_path)
    ov = {**OV, "data.test_ragged": True, "data.test_audio_frames": [20, 48]}
    ov.pop("train.crop_frames")
    monkeypatch.setattr("sys.argv", ["train_audio.py", "--mode", "train", "--gpus", "1", "--arith", "auto", "--set", "train.crop_frames=null"]
                        + [f"{k}={v}" for k, v in ov.items()])
    train_audio.main()
    out = capsys.readouterr().out
    gc.collect()
    assert "Epoch 1 loss" in out
    eers = [float(v) for v in re.findall(r"EER: ([0-9.]+)%", out)]
    assert len(eers) == 1 and 0.0 <= eers[0] <= 100.0
    runs = os.listdir("exp")
    assert len(runs) == 1 and os.path.exists(os.path.join("exp", runs[0], "net_avg.pth"))
