"""OnlineTriplet with on-device negative mining (-m gpu): dlip_triplet_mine_f32 / dlip_triplet_loss_f32 / dlip_triplet_loss_bwd_f32
against values captured from the reference's classes (tests/golden/capture_triplet_golden.py -> triplet_golden.npz) and against an
fp64 restatement of loss.py:28-31 evaluated here on the CPU.

Bars.  A pair is FRAGILE when its stored fp64 gap (best value - second best, or |best value|) is below 100 x dot_err of its case
(dot_err = the reference's own fp32 rounding of G off the diagonal): the engine sums in another order than the host BLAS.  Off
fragile pairs the triplet sets are equal; on them the engine's choice is within 100 x dot_err of the best; fragile pairs are at most
2 % of a case's pairs.  Loss and dX: distance from the fp64 values at most max(1e-4, 2 x the reference fp32's own distance), relative
to the tensor's largest magnitude.  Outputs and scratch are prefilled with NaN / -2 (triplet.DEBUG_PREFILL)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from deeplip_amd import weightgen as wg

pytestmark = pytest.mark.gpu
DEV = "cuda"
FRAGILE_FACTOR, FRAGILE_SHARE = 100.0, 0.02


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "triplet_golden.npz"))


@pytest.fixture(autouse=True)
def _prefill(monkeypatch):
    from deeplip_amd import triplet as tp
    monkeypatch.setattr(tp, "DEBUG_PREFILL", True)


def cases(gold):
    d = json.loads(str(gold["cases"]))
    return d["margin"], d["cases"]


def case_inputs(gold, name):
    """The capture script's formula: x = gain * (0.2 * centre[label] + noise)."""
    margin, cs = cases(gold)
    c = cs[name]
    B, S, E, gain = c["B"], c["S"], c["E"], c["gain"]
    labels = np.minimum((wg.gen(f"triplet.{name}.labels", (B,), kind="uniform") * S).astype(np.int64), S - 1)
    centres = wg.gen(f"triplet.{name}.centres", (S, E))
    noise = wg.gen(f"triplet.{name}.noise", (B, E))
    x = (np.float32(gain) * (np.float32(0.2) * centres[labels] + noise)).astype(np.float32)
    assert np.array_equal(labels, gold[f"{name}.labels"]) and np.array_equal(x[:2, :8], gold[f"{name}.x_probe"])
    return torch.from_numpy(x), torch.from_numpy(labels), margin


def restate64(x, trip, margin):
    """loss.py:28-31 in fp64 on the given triplets: (loss, dX); cos(i,j) = x_i.x_j / (max(|x_i|, 1e-8) max(|x_j|, 1e-8))."""
    x64 = x.double().clone().requires_grad_()
    if len(trip) == 0:
        return 0.0, np.zeros(tuple(x.shape))
    xn = x64 / x64.norm(dim=1, keepdim=True).clamp_min(1e-8)
    C = xn @ xn.T
    t = torch.as_tensor(np.asarray(trip), dtype=torch.int64)
    loss = torch.relu(C[t[:, 0], t[:, 2]] - C[t[:, 0], t[:, 1]] + margin).mean()
    loss.backward()
    return float(loss), x64.grad.numpy()


def rel(a, b, scale=None):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(scale if scale is not None else np.abs(b).max(), 1e-30))


def sorted_rows(t):
    t = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def run_engine(x, labels, margin, sel, u=None):
    from models.audio_models.loss import OnlineTriplet
    crit = OnlineTriplet(margin, sel)
    xg = x.to(DEV).requires_grad_()
    lab = labels.to(DEV)
    ug = None if u is None else u.to(DEV)
    loss, n = crit(xg, lab, u=ug)
    loss.backward()
    trip = sel.get_triplets(xg.detach(), lab, u=ug)
    torch.cuda.synchronize()
    return float(loss.detach()), int(n), xg.grad.cpu().numpy(), sorted_rows(trip.cpu().numpy())


SMALL_AND_BIG = ["b64_g1", "b64_g002", "b256_g01", "b256_g1", "b60_g01"]


@pytest.mark.parametrize("name", SMALL_AND_BIG)
def test_hardest_matches_reference(gold, name):
    from models.audio_models.utils import HardestNegativeTripletSelector
    x, labels, margin = case_inputs(gold, name)
    loss, n, dx, trip = run_engine(x, labels, margin, HardestNegativeTripletSelector(margin))
    assert np.isfinite(loss) and np.isfinite(dx).all() and n == len(trip)
    k = f"{name}.hardest"
    ref = sorted_rows(gold[k + ".triplets"])
    tol = FRAGILE_FACTOR * float(gold[f"{name}.dot_err"])
    pairs, gap = gold[f"{name}.pairs"].astype(np.int64), gold[f"{name}.gap"]
    fragile = gap < tol
    print(f"{name}: {len(pairs)} pairs, {int(fragile.sum())} fragile, dot_err {float(gold[name + '.dot_err']):.3e}, n {n} (reference {int(gold[k + '.n'])})")
    assert fragile.mean() <= FRAGILE_SHARE
    lab = labels.numpy()
    g64 = (x.double() @ x.double().T).numpy()
    eng = {(int(a), int(p)): int(q) for a, p, q in trip}
    want = {(int(a), int(p)): int(q) for a, p, q in ref}
    pairset = {(int(a), int(p)) for a, p in pairs}
    assert set(eng) <= pairset                                       # a < p, one label
    for (a, p, q) in trip:
        assert lab[a] == lab[p] != lab[q] and a < p
    differs = 0
    for (a, p), fr in zip(map(tuple, pairs), fragile):
        if not fr:
            assert eng.get((a, p)) == want.get((a, p)), (a, p, eng.get((a, p)), want.get((a, p)))
            continue
        negs = np.where(lab != lab[a])[0]
        v = g64[a, negs] + margin - g64[a, p]
        best = v.max()
        q = eng.get((a, p))
        differs += q != want.get((a, p))
        if q is None:
            assert best <= tol, (a, p, best)
        else:
            vq = g64[a, q] + margin - g64[a, p]
            assert vq >= best - tol and vq > -tol, (a, p, q, vq, best)
    # loss and dX
    same64 = differs == 0 and (k + ".triplets64") not in gold.files
    l64r, d64r = restate64(x, trip, margin)
    own32 = rel(gold[k + ".dx"], gold[k + ".dx64"], float(gold[k + ".dx64_absmax"]))
    bar_dx = max(1e-4, 2 * own32)
    bar_loss = max(1e-4, 2 * abs(float(gold[k + ".loss"]) - float(gold[k + ".loss64"])) / abs(float(gold[k + ".loss64"])))
    e_loss, e_dx = abs(loss - l64r) / abs(l64r), rel(dx, d64r)
    print(f"  vs fp64 restatement on the engine's triplets: loss {e_loss:.3e} (bar {bar_loss:.1e}), dX {e_dx:.3e} (bar {bar_dx:.1e})")
    assert e_loss <= bar_loss and e_dx <= bar_dx
    if same64:
        rows = gold[f"{name}.dx_rows"]
        g_loss = abs(loss - float(gold[k + ".loss64"])) / abs(float(gold[k + ".loss64"]))
        g_dx = rel(dx[rows], gold[k + ".dx64"], float(gold[k + ".dx64_absmax"]))
        g_norm = abs(np.linalg.norm(dx.astype(np.float64)) - float(gold[k + ".dx64_norm"])) / float(gold[k + ".dx64_norm"])
        print(f"  vs the reference in fp64: loss {g_loss:.3e}, dX rows {g_dx:.3e}, |dX| {g_norm:.3e}")
        assert n == int(gold[k + ".n"]) and g_loss <= bar_loss and g_dx <= bar_dx and g_norm <= bar_dx


@pytest.mark.parametrize("name", SMALL_AND_BIG)
def test_all_triplets_match_reference(gold, name):
    from models.audio_models.utils import AllTripletSelector
    x, labels, margin = case_inputs(gold, name)
    loss, n, dx, trip = run_engine(x, labels, margin, AllTripletSelector())
    k = f"{name}.all"
    assert n == int(gold[k + ".n"]) == len(trip)
    if (k + ".triplets") in gold.files:
        assert np.array_equal(trip, sorted_rows(gold[k + ".triplets"]))
    lab = labels.numpy()
    assert (lab[trip[:, 0]] == lab[trip[:, 1]]).all() and (lab[trip[:, 0]] != lab[trip[:, 2]]).all() and (trip[:, 0] < trip[:, 1]).all()
    assert len(np.unique(trip, axis=0)) == len(trip)
    rows = gold[f"{name}.dx_rows"]
    bar_dx = max(1e-4, 2 * rel(gold[k + ".dx"], gold[k + ".dx64"], float(gold[k + ".dx64_absmax"])))
    bar_loss = max(1e-4, 2 * abs(float(gold[k + ".loss"]) - float(gold[k + ".loss64"])) / abs(float(gold[k + ".loss64"])))
    g_loss = abs(loss - float(gold[k + ".loss64"])) / abs(float(gold[k + ".loss64"]))
    g_dx = rel(dx[rows], gold[k + ".dx64"], float(gold[k + ".dx64_absmax"]))
    g_norm = abs(np.linalg.norm(dx.astype(np.float64)) - float(gold[k + ".dx64_norm"])) / float(gold[k + ".dx64_norm"])
    l64r, d64r = restate64(x, trip, margin)
    e_dx = rel(dx, d64r)
    print(f"{name} all: n {n}, loss {g_loss:.3e} (bar {bar_loss:.1e}), dX rows {g_dx:.3e}, |dX| {g_norm:.3e}, dX vs restatement {e_dx:.3e} (bar {bar_dx:.1e})")
    assert np.isfinite(dx).all() and g_loss <= bar_loss and g_dx <= bar_dx and g_norm <= bar_dx and e_dx <= bar_dx


def _candidate_sets(g64, lab, a, p, margin, tol, semihard):
    negs = np.where(lab != lab[a])[0]
    v = g64[a, negs] + margin - g64[a, p]
    if semihard:
        sure, possible = (v > tol) & (v < margin - tol), (v > -tol) & (v < margin + tol)
    else:
        sure, possible = v > tol, v > -tol
    return negs[sure], negs[possible]


@pytest.mark.parametrize("mode", ["random", "semihard"])
@pytest.mark.parametrize("name", ["b64_g1", "b64_g002", "b256_g01"])
def test_random_and_semihard_pick_from_the_fp64_candidate_sets(gold, name, mode):
    from models.audio_models.utils import RandomNegativeTripletSelector, SemihardNegativeTripletSelector
    x, labels, margin = case_inputs(gold, name)
    sel = (RandomNegativeTripletSelector if mode == "random" else SemihardNegativeTripletSelector)(margin)
    B = x.shape[0]
    tol = FRAGILE_FACTOR * float(gold[f"{name}.dot_err"])
    lab = labels.numpy()
    g64 = (x.double() @ x.double().T).numpy()
    pairs = [tuple(int(v) for v in r) for r in gold[f"{name}.pairs"]]
    gen = torch.Generator().manual_seed(11)
    u = torch.rand((B, B), generator=gen)
    loss, n, dx, trip = run_engine(x, labels, margin, sel, u)
    loss2, n2, dx2, trip2 = run_engine(x, labels, margin, sel, u)
    assert np.array_equal(trip, trip2) and loss == loss2 and n == n2 and np.array_equal(dx, dx2)      # the same u, the same bits
    eng = {(int(a), int(p)): int(q) for a, p, q in trip}
    assert set(eng) <= set(pairs) and n == len(trip)
    sets = {ap: _candidate_sets(g64, lab, ap[0], ap[1], margin, tol, mode == "semihard") for ap in pairs}
    for ap in pairs:
        sure, possible = sets[ap]
        if ap in eng:
            assert eng[ap] in possible, (ap, eng[ap])
        else:
            assert len(sure) == 0, ap
    l64r, d64r = restate64(x, trip, margin)
    e_loss = abs(loss - l64r) / max(abs(l64r), 1e-30) if len(trip) else abs(loss)
    e_dx = rel(dx, d64r) if len(trip) else float(np.abs(dx).max())
    print(f"{name} {mode}: n {n} of {len(pairs)} pairs, loss err {e_loss:.3e}, dX err {e_dx:.3e} (bar 1e-4)")
    assert e_loss <= 1e-4 and e_dx <= 1e-4
    # u = 0 / u -> 1: the first / the last candidate (pairs whose candidate set is unambiguous)
    for uval, pick in ((0.0, 0), (float(np.nextafter(np.float32(1), np.float32(0))), -1)):
        _, _, _, t = run_engine(x, labels, margin, sel, torch.full((B, B), uval))
        got = {(int(a), int(p)): int(q) for a, p, q in t}
        checked = 0
        for ap in pairs:
            sure, possible = sets[ap]
            if len(sure) == len(possible) and len(sure) > 0:
                assert got[ap] == sure[pick], (ap, uval)
                checked += 1
        assert checked > 0 or all(len(s[0]) == 0 for s in sets.values())


def test_random_draws_cover_every_candidate(gold):
    """64 different u (one seeded generator) on the (64, 8, 64) case: every candidate of one pair that has 4 to 8 of them is drawn at
    least once (a coverage check, not a distribution test)."""
    from deeplip_amd import triplet as tp
    from models.audio_models.utils import RandomNegativeTripletSelector
    x, labels, margin = case_inputs(gold, "b64_g1")
    tol = FRAGILE_FACTOR * float(gold["b64_g1.dot_err"])
    lab = labels.numpy()
    g64 = (x.double() @ x.double().T).numpy()
    target = None
    for a, p in gold["b64_g1.pairs"]:
        sure, possible = _candidate_sets(g64, lab, int(a), int(p), margin, tol, False)
        if len(sure) == len(possible) and 4 <= len(sure) <= 8:
            target = (int(a), int(p), set(int(v) for v in sure))
            break
    assert target is not None, "no pair with 4 to 8 hard candidates in the fixture"
    sel = RandomNegativeTripletSelector(margin)
    xg, lg = x.to(DEV), labels.to(DEV)
    gen = torch.Generator().manual_seed(5)
    seen = set()
    for _ in range(64):
        m = sel.mine(xg, lg, torch.rand((64, 64), generator=gen).to(DEV))
        seen.add(int(m.neg[target[0], target[1]]))
    assert tp.DEBUG_PREFILL and seen == target[2], (seen, target[2])


def _crit(margin=0.2, sel="hardest"):
    from deeplip_amd.triplet import make_selector
    from models.audio_models.loss import OnlineTriplet
    return OnlineTriplet(margin, make_selector(sel, margin))


@pytest.mark.parametrize("sel", ["hardest", "all", "random", "semihard"])
def test_zero_triplets_give_zero_loss_and_gradient(gold, sel):
    x, labels, margin = case_inputs(gold, "onelabel")                  # one label holds the batch: no negatives
    for lab in (labels, torch.arange(x.shape[0])):                     # ... and: no label twice, no positives
        xg = x.to(DEV).requires_grad_()
        loss, n = _crit(margin, sel)(xg, lab.to(DEV))
        loss.backward()
        assert float(loss) == 0.0 and int(n) == 0 == int(gold["onelabel.n"])
        assert torch.isfinite(xg.grad).all() and bool((xg.grad == 0).all())
        assert _crit(margin, sel).triplet_selector.get_triplets(xg.detach(), lab.to(DEV)).shape == (0, 3)


@pytest.mark.parametrize("B,E", [(1, 64), (7, 4), (1024, 32), (33, 20)])
def test_edge_shapes(B, E):
    g = torch.Generator().manual_seed(B + E)
    x = torch.randn(B, E, generator=g) * 0.3
    labels = torch.randint(0, max(B // 4, 1), (B,), generator=g)
    for sel in ("hardest", "all") if B <= 64 else ("hardest",):
        crit = _crit(0.2, sel)
        xg = x.to(DEV).requires_grad_()
        loss, n = crit(xg, labels.to(DEV))
        loss.backward()
        trip = sorted_rows(crit.triplet_selector.get_triplets(xg.detach(), labels.to(DEV)).cpu().numpy())
        assert int(n) == len(trip)
        l64, d64 = restate64(x, trip, 0.2)
        assert torch.isfinite(xg.grad).all()
        assert abs(float(loss) - l64) <= 1e-4 * max(abs(l64), 1e-30) and (len(trip) == 0 or rel(xg.grad.cpu().numpy(), d64) <= 1e-4)
        if B == 1:
            assert int(n) == 0 and float(loss) == 0.0
        with torch.no_grad():                                           # the same forward launches without a tape
            l2, n2 = crit(x.to(DEV), labels.to(DEV))
        assert float(l2) == float(loss) and int(n2) == int(n)


def test_refused_shapes_and_label_types_raise_before_any_launch():
    from deeplip_amd._lib import DeepLipHipError
    crit = _crit()
    lab = torch.zeros(8, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        crit(torch.zeros(8, 6, device=DEV), lab)
    with pytest.raises(ValueError):
        crit(torch.zeros(1025, 8, device=DEV), torch.zeros(1025, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError):
        crit(torch.zeros(8, 8, device=DEV), lab.float())
    with pytest.raises(ValueError):
        crit(torch.zeros(8, 8, device=DEV), lab[:7])
    with pytest.raises(DeepLipHipError):
        crit(torch.zeros(8, 8), lab)


def test_int32_and_int64_labels_agree(gold):
    x, labels, margin = case_inputs(gold, "b64_g1")
    outs = []
    for dt in (torch.int64, torch.int32):
        xg = x.to(DEV).requires_grad_()
        loss, n = _crit(margin)(xg, labels.to(DEV).to(dt))
        loss.backward()
        outs.append((float(loss), int(n), xg.grad.clone()))
    assert outs[0][:2] == outs[1][:2] and torch.equal(outs[0][2], outs[1][2])


def _net():
    from models.audio_models.tdnn import SpeakerEmbNet
    opts = {"arch": "tdnn", "tdnn": {"input_dim": 24, "hidden_dim": [64, 64, 64, 64, 128], "context": [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0], [0]],
                                     "tdnn_layers": 5, "fc_layers": 3, "embedding_dim": 64, "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}}
    net = SpeakerEmbNet(opts)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, prefix="triplet.net.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to(DEV).train()


def _batch(seed, B=24, S=5, T=60):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 24, T, generator=g).to(DEV), torch.randint(0, S, (B,), generator=g).to(DEV)


def test_autograd_through_the_criterion_matches_dx_injected_by_hand():
    from deeplip_amd import triplet as tp
    x, lab = _batch(1)
    crit = _crit(0.2, "hardest")
    net = _net()
    emb = net(x)
    loss, n = crit(emb, lab)
    assert int(n) > 0
    loss.backward()
    got = {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}
    net2 = _net()
    emb2 = net2(x)
    assert torch.equal(emb2.detach(), emb.detach())
    m = tp.mine(emb2.detach(), lab, 0.2, tp.MODE_HARDEST)
    _, n2, wc = tp.loss_forward(m, 0.2)
    emb2.backward(tp.loss_backward(emb2.detach(), m, wc, n2))
    assert len(got) > 4
    for k, p in net2.named_parameters():
        assert torch.equal(p.grad, got[k]), k


@pytest.mark.parametrize("sel", ["hardest", "semihard"])
def test_recorded_step_replayed_on_a_second_batch_is_bit_identical_to_eager(sel):
    from deeplip_amd.train_plan import TrainStepGraph

    def run(recorded):
        torch.manual_seed(3)
        torch.cuda.manual_seed(3)
        net, crit = _net(), _crit(0.2, sel)
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
    assert len({n for _, n in o_g}) > 1                                # the batches differ in their number of triplets
    assert o_g == o_e and torch.equal(p_g, p_e)


OV = {"data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 200, "data.trial_targets": 40, "data.audio_frames": 120,
      "data.n_spk": 6, "data.utt_per_spk": 3, "train.bs": 16, "train.epoch": 2, "train.steps_per_epoch": 3, "train.loss": "Triplet"}


def _train(tmp_path, monkeypatch, sel, graph_step=True, eager_launches=False):
    import train_audio
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tr = train_audio.Trainer(overrides={**OV, "train.triplet": {"margin": 0.2, "selector": sel}, "train.graph_step": graph_step},
                             arith_mode="f32")
    if eager_launches:
        tr.graph_step = False           # the same (fused) optimiser, every launch issued from Python: only the replay differs
    w0 = torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).clone()
    tr._train()
    w1 = torch.cat([p.detach().reshape(-1) for p in tr.model.parameters()]).clone()
    st = tr.last_epoch_stats
    assert len(list(tr.criterion.parameters())) == 0 and len(tr.optim.param_groups) == 1
    assert np.isfinite(st["loss"]) and st["triplets"] > 0 and "acc" not in st and not torch.equal(w0, w1)
    return tr, st, w1.cpu()


@pytest.mark.parametrize("sel", ["hardest", "semihard", "random", "all"])
def test_train_audio_with_the_triplet_loss(tmp_path, monkeypatch, sel):
    tr, st, w = _train(tmp_path, monkeypatch, sel)
    assert st["step_mode"] == "graph"
    tr_e, st_e, w_e = _train(tmp_path, monkeypatch, sel, graph_step=False)       # --eager-step
    assert st_e["step_mode"] == "eager"
    if sel == "hardest":
        tr_l, st_l, w_l = _train(tmp_path, monkeypatch, sel, eager_launches=True)
        assert st_l["step_mode"] == "eager" and st_l["loss"] == st["loss"] and st_l["triplets"] == st["triplets"] and torch.equal(w, w_l)
