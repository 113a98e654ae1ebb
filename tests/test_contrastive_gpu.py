"""Contrastive with the pairs selected on the device (-m gpu): dlip_contrastive_loss_f32 and its backward (dlip_triplet_loss_bwd_f32 on
the signed pair weights) against the fp64 restatement of contrastive_ref.py -- upstream has no implementation.

Bars.  A hard-mode row is FRAGILE when its fp64 gap between the K-th and the (K+1)-th candidate cosine is below 100 x cos_err of its
case (cos_err = the fp32 restatement's worst cosine error): off fragile rows the pair sets are equal, on them every chosen negative is
within that tolerance of the K-th best; at most 5 % of the rows that have a choice to make are fragile (asserted on the CPU).  Loss and
dX on the ENGINE'S OWN pair sets: distance from fp64 at most max(project bar, 2 x the fp32 restatement's own distance), project bars
2e-5 (loss) and 1e-4 (dX, relative to its largest magnitude); both distances are printed.  Outputs and scratch are prefilled with
NaN / -2 (triplet.DEBUG_PREFILL)."""
import numpy as np
import pytest
import torch

import contrastive_ref as cr
from deeplip_amd import weightgen as wg

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["all", "hard_negative"]


@pytest.fixture(autouse=True)
def _prefill(monkeypatch):
    from deeplip_amd import triplet as tp
    monkeypatch.setattr(tp, "DEBUG_PREFILL", True)


def _crit(margin=cr.MARGIN, sel="hard_negative"):
    from deeplip_amd.pairs import make_pair_selector
    from models.audio_models.loss import Contrastive
    return Contrastive(margin, make_pair_selector(sel))


def run_engine(x, labels, margin, sel):
    crit = _crit(margin, sel)
    xg = x.to(DEV).requires_grad_()
    lab = labels.to(DEV)
    loss, n = crit(xg, lab)
    loss.backward()
    pos, neg = crit.pair_selector.get_pairs(xg.detach(), lab)
    torch.cuda.synchronize()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and n.dim() == 0 and n.dtype == torch.int32 and loss.is_cuda and n.is_cuda
    return float(loss.detach()), int(n), xg.grad.cpu().numpy(), [tuple(r) for r in pos.cpu().tolist()], [tuple(r) for r in neg.cpu().tolist()]


def check_loss_and_dx(x, pos, neg, margin, loss, dx, what):
    l64, d64 = cr.restate(x, pos, neg, margin, torch.float64)
    l32, d32 = cr.restate(x, pos, neg, margin, torch.float32)
    assert np.isfinite(loss) and np.isfinite(dx).all()
    if len(pos) + len(neg) == 0:
        assert loss == 0.0 and not dx.any()
        return
    own = (abs(l32 - l64) / abs(l64), cr.rel(d32, d64))
    got = (abs(loss - l64) / abs(l64), cr.rel(dx, d64))
    print(f"{what}: {len(pos)} + {len(neg)} pairs, loss {got[0]:.2e} (fp32 {own[0]:.2e}), dX {got[1]:.2e} (fp32 {own[1]:.2e})")
    assert got[0] <= max(cr.BAR_LOSS, 2 * own[0]) and got[1] <= max(cr.BAR_GRAD, 2 * own[1]), (got, own)


@pytest.mark.parametrize("sel", MODES)
@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_selection_loss_and_gradient_match_fp64(name, sel):
    x, labels = cr.case_inputs(name)
    lab = labels.numpy()
    loss, n, dx, pos, neg = run_engine(x, labels, cr.MARGIN, sel)
    pos64, neg64, rows = cr.select64(x, labels, sel)
    facts = cr.case_facts(name)
    tol = cr.FRAGILE_FACTOR * facts["cos_err"]
    assert n == len(pos) + len(neg)
    assert pos == sorted(pos) and neg == sorted(neg) and len(set(pos)) == len(pos) and len(set(neg)) == len(neg)
    assert set(pos) == set(pos64)
    assert all(a < j and lab[a] != lab[j] for a, j in neg)
    if sel == "all":
        assert set(neg) == set(neg64)
    else:
        fragile = set(facts["fragile"])
        by_row = {}
        for a, j in neg:
            by_row.setdefault(a, []).append(j)
        want = {}
        for a, j in neg64:
            want.setdefault(a, []).append(j)
        assert {a: len(v) for a, v in by_row.items()} == {a: len(v) for a, v in want.items()}       # K per row
        for a in set(want) - fragile:
            assert sorted(by_row[a]) == sorted(want[a]), a
        for a in fragile & set(want):
            K, order, c = rows[a]
            cos_a = dict(zip(order.tolist(), c.tolist()))
            assert all(cos_a[j] >= c[K - 1] - tol for j in by_row[a]), a
        # as many negatives as positives, except where a row runs out of later negatives
        short = sum(1 for a in range(len(lab)) if (lab[a + 1:] == lab[a]).sum() > (lab[a + 1:] != lab[a]).sum())
        assert (len(neg) == len(pos)) == (short == 0) and short == (1 if name == "b33" else 0)
    check_loss_and_dx(x, pos, neg, cr.MARGIN, loss, dx, f"{name} {sel}")


@pytest.mark.parametrize("sel", MODES)
def test_edge_batches(sel):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(12, 16, generator=g)
    # B = 1: no pair; B = 2: one pair, positive or negative
    loss, n, dx, pos, neg = run_engine(x[:1], torch.zeros(1, dtype=torch.int64), 0.1, sel)
    assert (loss, n, pos, neg) == (0.0, 0, [], []) and not dx.any()
    loss, n, dx, pos, neg = run_engine(x[:2], torch.zeros(2, dtype=torch.int64), 0.1, sel)
    assert (n, pos, neg) == (1, [(0, 1)], [])
    check_loss_and_dx(x[:2], pos, neg, 0.1, loss, dx, f"B 2 positive {sel}")
    loss, n, dx, pos, neg = run_engine(x[:2], torch.arange(2), -0.9, sel)
    assert (n, pos, neg) == ((1, [], [(0, 1)]) if sel == "all" else (0, [], []))
    check_loss_and_dx(x[:2], pos, neg, -0.9, loss, dx, f"B 2 negative {sel}")
    # all labels equal: no negatives, only positives in either mode
    loss, n, dx, pos, neg = run_engine(x, torch.full((12,), 3), 0.1, sel)
    assert n == 66 == len(pos) and neg == []
    check_loss_and_dx(x, pos, neg, 0.1, loss, dx, f"one label {sel}")
    # all labels distinct: `all` gives only negatives; `hard_negative` has no positive to balance: zero pairs, loss 0, dX exactly 0
    loss, n, dx, pos, neg = run_engine(x, torch.arange(12), -0.5, sel)
    if sel == "all":
        assert n == 66 == len(neg) and pos == []
        check_loss_and_dx(x, pos, neg, -0.5, loss, dx, "distinct labels all")
    else:
        assert (loss, n, pos, neg) == (0.0, 0, [], []) and not dx.any()


def test_ties_go_to_the_lower_index():
    """Rows 1 .. 4 are copies of one vector: equal cosines to the anchor bit for bit; the K = 2 hardest are the two lowest indices."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 8, generator=g)
    x[1:5] = x[1].clone()
    x[0] = x[1] + 0.05 * x[0]
    labels = torch.tensor([0, 1, 2, 3, 4, 0, 0, 5])
    _, n, _, pos, neg = run_engine(x, labels, 0.1, "hard_negative")
    assert [p for p in pos if p[0] == 0] == [(0, 5), (0, 6)] and [q for q in neg if q[0] == 0] == [(0, 1), (0, 2)]
    assert n == len(pos) + len(neg)


@pytest.mark.parametrize("B,E", [(1024, 32), (33, 20), (7, 4)])
def test_edge_shapes_complete_with_finite_results(B, E):
    g = torch.Generator().manual_seed(B + E)
    x = torch.randn(B, E, generator=g) * 0.3
    labels = torch.randint(0, max(B // 4, 1), (B,), generator=g)
    for sel in MODES:
        crit = _crit(0.1, sel)
        xg = x.to(DEV).requires_grad_()
        loss, n = crit(xg, labels.to(DEV))
        loss.backward()
        assert bool(torch.isfinite(loss)) and int(n) > 0 and bool(torch.isfinite(xg.grad).all())
        if B <= 64:
            pos, neg = crit.pair_selector.get_pairs(xg.detach(), labels.to(DEV))
            check_loss_and_dx(x, [tuple(r) for r in pos.cpu().tolist()], [tuple(r) for r in neg.cpu().tolist()], 0.1, float(loss.detach()),
                              xg.grad.cpu().numpy(), f"({B},{E}) {sel}")
        else:
            lab = labels.numpy()
            same = (lab[:, None] == lab[None, :])
            iu = np.triu_indices(B, 1)
            n_pos = int(same[iu].sum())
            later_pos = np.array([(lab[a + 1:] == lab[a]).sum() for a in range(B)])
            later_neg = (B - 1 - np.arange(B)) - later_pos
            assert int(n) == (B * (B - 1) // 2 if sel == "all" else n_pos + int(np.minimum(later_pos, later_neg).sum()))
        with torch.no_grad():                                           # the same forward launches without a tape
            l2, n2 = crit(x.to(DEV), labels.to(DEV))
        assert float(l2) == float(loss) and int(n2) == int(n)


def test_refused_shapes_and_label_types_raise_before_any_launch():
    from deeplip_amd._lib import DeepLipHipError
    for sel in MODES:
        crit = _crit(0.1, sel)
        lab = torch.zeros(8, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError):
            crit(torch.zeros(8, 6, device=DEV), lab)
        with pytest.raises(ValueError):
            crit(torch.zeros(1025, 8, device=DEV), torch.zeros(1025, dtype=torch.int64, device=DEV))
        with pytest.raises(ValueError):
            crit(torch.zeros(8, 8, device=DEV), lab.float())
        with pytest.raises(ValueError):
            crit(torch.zeros(8, 8, device=DEV), lab[:7])
        with pytest.raises(ValueError):
            crit.pair_selector.get_pairs(torch.zeros(8, 6, device=DEV), lab)
        with pytest.raises(DeepLipHipError):
            crit(torch.zeros(8, 8), lab)


def test_int32_and_int64_labels_agree():
    x, labels = cr.case_inputs("b64_g1")
    outs = []
    for dt in (torch.int64, torch.int32):
        xg = x.to(DEV).requires_grad_()
        loss, n = _crit()(xg, labels.to(DEV).to(dt))
        loss.backward()
        outs.append((float(loss), int(n), xg.grad.clone()))
    assert outs[0][:2] == outs[1][:2] and torch.equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("sel", MODES)
def test_autograd_through_the_criterion_is_the_bare_dx_times_the_upstream_scalar(sel):
    from deeplip_amd import pairs as pr
    x, labels = cr.case_inputs("b64_g1")
    xg, lab = x.to(DEV).requires_grad_(), labels.to(DEV)
    loss, n = _crit(cr.MARGIN, sel)(xg, lab)
    (loss * 3.0).backward()
    p = pr.loss_forward(x.to(DEV), lab, cr.MARGIN, pr.MODES[sel])
    bare = pr.loss_backward(x.to(DEV), p)
    scaled = pr.loss_backward(x.to(DEV), p, torch.full((1,), 3.0, device=DEV))
    assert float(p.loss) == float(loss) and int(p.n) == int(n) > 0
    assert torch.equal(xg.grad, scaled) and cr.rel(xg.grad.cpu().numpy(), 3.0 * bare.cpu().numpy()) <= 1e-6


def _net():
    from models.audio_models.tdnn import SpeakerEmbNet
    opts = {"arch": "tdnn", "tdnn": {"input_dim": 24, "hidden_dim": [64, 64, 64, 64, 128], "context": [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0], [0]],
                                     "tdnn_layers": 5, "fc_layers": 3, "embedding_dim": 64, "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}}
    net = SpeakerEmbNet(opts)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="contrastive.net.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV).train()


def _batch(seed, B=24, S=5, T=60):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 24, T, generator=g).to(DEV), torch.randint(0, S, (B,), generator=g).to(DEV)


@pytest.mark.parametrize("sel", MODES)
def test_recorded_step_replayed_on_a_second_batch_is_bit_identical_to_eager(sel):
    from deeplip_amd.train_plan import TrainStepGraph

    def run(recorded):
        torch.manual_seed(3)
        torch.cuda.manual_seed(3)
        net, crit = _net(), _crit(0.5, sel)
        opt = torch.optim.SGD(net.parameters(), lr=torch.tensor(0.05, device=DEV), momentum=0.9, fused=True)

        def one(x, lab):
            opt.zero_grad(set_to_none=True)
            loss, n = crit(net(x), lab)
            loss.backward()
            opt.step()
            return loss, n
        plan = TrainStepGraph(one, eager_steps=1 if recorded else 10 ** 6, device=torch.device(DEV), branch_streams=False, verify=False)
        outs = []
        for seed in (1, 2, 3, 4):
            loss, n = plan.step(*_batch(seed))
            plan.finish()
            outs.append((float(loss), int(n)))
        assert plan.recorded == recorded
        return outs, torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()

    o_g, p_g = run(True)
    o_e, p_e = run(False)
    assert len({l for l, _ in o_g}) > 1 and all(n > 0 for _, n in o_g)
    if sel == "hard_negative":
        assert len({n for _, n in o_g}) > 1                            # the batches differ in their number of pairs
    assert o_g == o_e and torch.equal(p_g, p_e)


OV = {"data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 200, "data.trial_targets": 40, "data.audio_frames": 120,
      "data.n_spk": 6, "data.utt_per_spk": 3, "train.bs": 16, "train.epoch": 2, "train.steps_per_epoch": 3}       # test_triplet_gpu.py's


def _train(tmp_path, monkeypatch, overrides):
    """(epoch statistics, facts about the trainer) of a two-epoch run.  A trainer and its recorded steps point at each other, so a dead
    one waits for Python's cyclic collector, and a recorded graph destroyed by the collector INSIDE a later capture aborts the process:
    the dead ones go here, outside any capture, before the next trainer is built and after this one is done."""
    import gc
    import train_audio
    gc.collect()
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tr = train_audio.Trainer(overrides={**OV, **overrides}, arith_mode="f32")
    w0 = torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).clone()
    tr._train()
    w1 = torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).clone()
    facts = {"class": type(tr.criterion), "crit_params": len(list(tr.criterion.parameters())), "groups": len(tr.optim.param_groups),
             "moved": not torch.equal(w0, w1)}
    st = tr.last_epoch_stats
    del tr
    gc.collect()
    return st, facts


def test_train_audio_with_the_online_contrastive_loss(tmp_path, monkeypatch):
    from models.audio_models.loss import Contrastive
    st_t, _ = _train(tmp_path, monkeypatch, {"train.loss": "Triplet"})
    for sel in ("hard_negative", "all"):
        st, facts = _train(tmp_path, monkeypatch, {"train.loss": "OnlineContrastive", "train.contrastive": {"margin": 0.5, "selector": sel}})
        assert facts["class"] is Contrastive and facts["crit_params"] == 0 and facts["groups"] == 1
        assert np.isfinite(st["loss"]) and st["pairs"] > 0 and "acc" not in st and "triplets" not in st and facts["moved"]
        assert st["step_mode"] == st_t["step_mode"] == "graph"
    assert "triplets" in st_t and "pairs" not in st_t
