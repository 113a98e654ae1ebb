"""Cohort score normalisation on the GPU: the selection kernel against fp64 statistics of the same fp32 values (one rounding:
rtol 1e-6), score_norm against its formula, cohort_stats / normalised_scores / the fusion scorings against an fp64 restatement
(normalise, ``@``, ``topk``, centred deviation with divisor K) at the project's bar, the entry points end to end over an on-disk
store, a recorded StepPlan, and train_audio's wiring."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import conftest

pytestmark = pytest.mark.gpu


def assert_close_rel(a, b, **kw):
    """conftest's bar, and every element finite first: a NaN compares false against any bound and would pass it."""
    assert np.isfinite(np.asarray(a, dtype=np.float64)).all(), (kw.get("what", ""), "non-finite elements")
    conftest.assert_close_rel(a, b, **kw)


# ------------------------------------------------------------------------------------------ the fp64 restatement (CPU torch)
def ref_topk_stats(s: torch.Tensor, k: int):
    top = s.double().topk(k, dim=1).values
    mu = top.mean(1, keepdim=True)
    return mu[:, 0], ((top - mu) ** 2).mean(1).sqrt()


def ref_l2n(x: torch.Tensor):
    x = x.double()
    return x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)


def ref_cohort_stats(emb, cohort, k=None):
    s = ref_l2n(emb) @ ref_l2n(cohort).T
    return ref_topk_stats(s, cohort.shape[0] if k is None else k)


def ref_norm(s, ia, ib, mu, sd, mode, eps=1e-6):
    za = (s - mu[ia]) / sd[ia].clamp_min(eps)
    zb = (s - mu[ib]) / sd[ib].clamp_min(eps)
    return {"z": za, "t": zb, "s": 0.5 * (za + zb)}[mode]


def ref_cosine(emb, ia, ib):
    n = ref_l2n(emb)
    return (n[ia] * n[ib]).sum(1)


def ref_normalised(emb, ia, ib, cohort, mode, k=None):
    mu, sd = ref_cohort_stats(emb, cohort, k)
    return ref_norm(ref_cosine(emb, ia, ib), ia, ib, mu, sd, mode)


def ref_znorm_cat(v, a):
    z = lambda x: (x.double() - x.double().mean(1, keepdim=True)) / x.double().std(1, unbiased=False, keepdim=True)   # noqa: E731
    return torch.cat([z(v), z(a)], 1)


@functools.lru_cache(maxsize=None)
def speaker_data(U, Nc, D, seed=0, trials=2000):
    """20 Gaussian speaker centroids + 0.8 noise per row (table and cohort alike), random trials."""
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(20, D, generator=g)
    emb = cent[torch.randint(0, 20, (U,), generator=g)] + 0.8 * torch.randn(U, D, generator=g)
    cohort = cent[torch.randint(0, 20, (Nc,), generator=g)] + 0.8 * torch.randn(Nc, D, generator=g)
    ia = torch.randint(0, U, (trials,), generator=g)
    ib = torch.randint(0, U, (trials,), generator=g)
    return emb, cohort, ia, ib


def dev_idx(i):
    return i.to(torch.int32).cuda()


def run_topk(s: torch.Tensor, k: int, n=None):
    from deeplip_amd import ops
    mean, sd = ops.topk_stats(s.cuda(), k, n)
    return mean.cpu(), sd.cpu()


# ------------------------------------------------------------------------------------------ the selection kernel
@pytest.mark.parametrize("R,N,K", [(3, 1, 1), (5, 7, 3), (4, 255, 255), (4, 256, 1), (4, 257, 256), (2, 1000, 300), (2, 4099, 300),
                                   (1, 32768, 300), (1, 32768, 32768)])
def test_topk_stats_matches_fp64(R, N, K):
    s = torch.randn(R, N, generator=torch.Generator().manual_seed(N + K))
    mean, sd = run_topk(s, K)
    wm, ws = ref_topk_stats(s, K)
    assert_close_rel(mean, wm, rtol=1e-6, what=f"mean {R, N, K}")
    assert_close_rel(sd, ws, rtol=1e-6, what=f"sd {R, N, K}")


@pytest.mark.parametrize("fill", [float("inf"), float("nan")])
def test_topk_stats_never_reads_the_padding(fill):
    from deeplip_amd import ops
    N, K = 300, 40
    s = torch.randn(6, N, generator=torch.Generator().manual_seed(1))
    wide = torch.full((6, N + 5), fill)
    wide[:, :N] = s
    dev = wide.cuda()
    mean, sd = ops.topk_stats(dev, K, n=N)
    m0, s0 = ops.topk_stats(s.cuda(), K)
    assert torch.equal(mean, m0) and torch.equal(sd, s0)
    wm, ws = ref_topk_stats(s, K)
    assert_close_rel(mean.cpu(), wm, rtol=1e-6, what="mean")
    assert_close_rel(sd.cpu(), ws, rtol=1e-6, what="sd")


def test_topk_stats_signs_and_zeros():
    g = torch.Generator().manual_seed(2)
    neg = -torch.rand(4, 500, generator=g) - 0.25                                     # rows that are all negative
    zeros = torch.randn(4, 500, generator=g)
    zeros[:, ::3] = 0.0
    zeros[:, 1::3] = -0.0                                                             # +0.0 and -0.0 in one row, inside the top K
    zeros[:, 2::3] = -zeros[:, 2::3].abs()
    assert (zeros == 0).sum() > 1000 and torch.signbit(zeros[zeros == 0]).any() and not torch.signbit(zeros[zeros == 0]).all()
    for s, k in ((neg, 1), (neg, 37), (neg, 500), (zeros, 100), (zeros, 334), (zeros, 400)):
        mean, sd = run_topk(s, k)
        wm, ws = ref_topk_stats(s, k)
        assert_close_rel(mean, wm, rtol=1e-6, what=f"mean k={k}")
        assert_close_rel(sd, ws, rtol=1e-6, what=f"sd k={k}")
    mean, sd = run_topk(zeros, 200)                                                   # only zeros of either sign are selected
    assert (mean == 0).all() and (sd == 0).all()


def test_topk_stats_counts_ties_exactly():
    s = torch.round(torch.randn(6, 2000, generator=torch.Generator().manual_seed(3)) * 8) / 8      # multiples of 1/8: the K-th value is shared
    for k in (100, 300, 1001, 1900):
        kth = s.topk(k, dim=1).values[:, -1:]
        assert ((s == kth).sum(1) > 1).all()
        mean, sd = run_topk(s, k)
        wm, ws = ref_topk_stats(s, k)
        assert_close_rel(mean, wm, rtol=1e-6, what=f"mean k={k}")
        assert_close_rel(sd, ws, rtol=1e-6, what=f"sd k={k}")
    # runs of equal values, every K: one copy of a tied value too many or too few moves the mean by 1 / K of a gap
    row = torch.tensor([[0.0] * 5 + [0.5] * 10 + [1.0] * 3, [0.5] * 9 + [-2.0] * 8 + [4.0]])
    for k in range(1, 19):
        mean, sd = run_topk(row, k)
        wm, ws = ref_topk_stats(row, k)
        assert_close_rel(mean, wm, rtol=1e-6, what=f"runs: mean k={k}")
        assert_close_rel(sd, ws, rtol=1e-6, what=f"runs: sd k={k}")


def test_topk_stats_constant_rows_and_every_output_written():
    from deeplip_amd import ops
    vals = torch.tensor([0.1, -3.7, 1e-20, 12345.678, 0.0])
    s = vals[:, None].repeat(1, 777).cuda()
    for k in (1, 300, 777):
        mean = torch.full((5,), float("nan"), device="cuda")
        sd = torch.full((5,), float("nan"), device="cuda")
        from deeplip_amd._lib import check, lib, ptr, stream_handle
        check(lib().dlip_topk_stats_f32(ptr(s), 5, 777, 777, k, ptr(mean), ptr(sd), stream_handle()), "dlip_topk_stats_f32")
        assert torch.equal(mean.cpu(), vals) and torch.equal(sd.cpu(), torch.zeros(5)), k
    m, d = ops.topk_stats(torch.randn(300, 33).cuda(), 5)                             # more rows than a wave of workgroups
    assert m.shape == (300,) and d.shape == (300,) and not torch.isnan(m).any() and not torch.isnan(d).any() and (d > 0).all()
    with pytest.raises(TypeError):
        ops.topk_stats(torch.zeros(3, 7, dtype=torch.float64, device="cuda"), 2)


# ------------------------------------------------------------------------------------------ score_norm
def test_score_norm_modes_weight_and_accumulate():
    from deeplip_amd import ops
    from deeplip_amd._lib import DeepLipHipError  # noqa: F401
    g = torch.Generator().manual_seed(4)
    U, n = 23, 1111
    s, mu, sd = torch.randn(n, generator=g), torch.randn(U, generator=g), torch.rand(U, generator=g) + 0.05
    ia, ib = torch.randint(0, U, (n,), generator=g), torch.randint(0, U, (n,), generator=g)
    args = (s.cuda(), dev_idx(ia), dev_idx(ib), mu.cuda(), sd.cuda())
    for mode in ("z", "t", "s"):
        want = ref_norm(s.double(), ia, ib, mu.double(), sd.double(), mode)
        # computed in fp64 and rounded once: rtol 1e-6 as for the statistics
        assert_close_rel(ops.score_norm(*args, mode=mode).cpu(), want, rtol=1e-6, what=mode)
        assert_close_rel(ops.score_norm(*args, mode=mode, weight=0.25).cpu(), 0.25 * want, rtol=1e-6, what=mode + " weighted")
    base = torch.randn(n, generator=g)
    out = base.clone().cuda()
    got = ops.score_norm(*args, mode="s", weight=0.5, out=out)
    assert got is out
    assert_close_rel(out.cpu(), base.double() + 0.5 * ref_norm(s.double(), ia, ib, mu.double(), sd.double(), "s"), rtol=1e-6, what="accumulate")
    # sd = 0: eps takes over and the result stays finite
    z = ops.score_norm(args[0], args[1], args[2], args[3], torch.zeros(U).cuda(), mode="s", eps=1e-6).cpu()
    assert torch.isfinite(z).all()
    assert_close_rel(z, ref_norm(s.double(), ia, ib, mu.double(), torch.zeros(U).double(), "s", eps=1e-6), rtol=1e-6, what="sd = 0")
    bad = ops.score_norm(args[0], torch.full((n,), U, dtype=torch.int32).cuda(), args[2], args[3], args[4]).cpu()
    assert torch.isnan(bad).all()                                                     # the caller's error comes out as NaN, nothing is read out of bounds
    with pytest.raises(ValueError):
        ops.score_norm(*args, mode="q")


# ------------------------------------------------------------------------------------------ cohort_stats / normalised_scores
SHAPES = [(37, 257, 64, 20), (64, 1000, 512, 300), (33, 4099, 512, 300), (16, 300, 512, 300)]


@pytest.mark.parametrize("U,Nc,D,K", SHAPES)
def test_cohort_stats_and_normalised_scores_match_fp64(U, Nc, D, K):
    from deeplip_amd import ops, scoring
    emb, cohort, ia, ib = speaker_data(U, Nc, D)
    mu, sd = ops.cohort_stats(emb.cuda(), cohort.cuda(), top_k=K)
    wmu, wsd = ref_cohort_stats(emb, cohort, K)
    assert_close_rel(mu.cpu(), wmu, what="mu")
    assert_close_rel(sd.cpu(), wsd, what="sd")
    for kind, mode, k in (("asnorm", "s", K), ("snorm", "s", None), ("znorm", "z", None), ("tnorm", "t", None)):
        got = scoring.normalised_scores(emb.cuda(), dev_idx(ia), dev_idx(ib), cohort.cuda(), kind, K)
        assert_close_rel(got.cpu(), ref_normalised(emb, ia, ib, cohort, mode, k), what=kind)


def test_cohort_stats_top_k_none_chunks_and_unused_rows():
    from deeplip_amd import ops, scoring
    U, Nc, D, K = 37, 257, 64, 20
    emb, cohort, ia, ib = speaker_data(U, Nc, D)
    e, c = emb.cuda(), cohort.cuda()
    a, b = ops.cohort_stats(e, c, top_k=None), ops.cohort_stats(e, c, top_k=Nc)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    whole, chunked = ops.cohort_stats(e, c, top_k=K), ops.cohort_stats(e, c, top_k=K, chunk_rows=5)     # 8 chunks, the last of 2 rows
    assert_close_rel(chunked[0].cpu(), whole[0].cpu(), rtol=1e-6, what="mu chunked")
    assert_close_rel(chunked[1].cpu(), whole[1].cpu(), rtol=1e-6, what="sd chunked")
    # rows no trial uses: a table twice as tall whose extra rows are never referenced gives the same scores
    ja, jb = 2 * ia[:300], 2 * ib[:300]
    tall = torch.full((2 * U, D), 1e30)
    tall[::2] = emb
    tr = scoring.trial_rows(dev_idx(ja), dev_idx(jb), 2 * U)
    assert tr.rows is not None and tr.n_used == len(set(ja.tolist()) | set(jb.tolist())) <= U
    got = scoring.normalised_scores(tall.cuda(), dev_idx(ja), dev_idx(jb), c, "asnorm", K)
    want = scoring.normalised_scores(e, dev_idx(ia[:300]), dev_idx(ib[:300]), c, "asnorm", K)
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        scoring.normalised_scores(e, dev_idx(ia + 1), dev_idx(ib), c, "asnorm", K)     # an index past the table: refused on the host


def test_fusion_scorings_match_fp64():
    from deeplip_amd import scoring
    U, Nc, D, K = 40, 300, 64, 30
    a, ca, ia, ib = speaker_data(U, Nc, D, seed=5, trials=500)
    v, cv, _, _ = speaker_data(U, Nc, D, seed=6, trials=500)
    dev = [t.cuda() for t in (a, v)] + [dev_idx(ia), dev_idx(ib)] + [ca.cuda(), cv.cuda()]
    # score fusion: each half normalised against its own cohort (for vectors this far from zero F.cosine_similarity's eps is idle)
    want = 0.5 * ref_normalised(a, ia, ib, ca, "s", K) + 0.5 * ref_normalised(v, ia, ib, cv, "s", K)
    assert_close_rel(scoring.score_fusion_normalised(*dev, "asnorm", K).cpu(), want, what="score fusion")
    fa, fc = ref_znorm_cat(v, a), ref_znorm_cat(cv, ca)
    want = ref_normalised(fa, ia, ib, fc, "s", K)
    assert_close_rel(scoring.feature_fusion_scores_normalised(*dev, "asnorm", K).cpu(), want, what="feature fusion")
    want = ref_normalised(fa, ia, ib, fc, "z", None)
    assert_close_rel(scoring.feature_fusion_scores_normalised(*dev, "znorm").cpu(), want, what="feature fusion znorm")


def test_speaker_mean_cohort():
    from deeplip_amd import scoring
    g = torch.Generator().manual_seed(7)
    emb = torch.randn(11, 16, generator=g)
    lab = [4, 2, 4, 9, 2, 4, 2, 2, 7, 4, 2]
    got = scoring.speaker_mean_cohort(emb.cuda(), lab).cpu()
    want = torch.stack([emb[[i for i, l in enumerate(lab) if l == s]].double().mean(0) for s in (2, 4, 7, 9)])
    assert_close_rel(got, want, rtol=1e-6, what="speaker means")
    assert torch.equal(got[2], emb[8]) and torch.equal(got[3], emb[3])                # speakers with a single row
    table = scoring.EmbeddingTable([f"u{i}" for i in range(11)], emb.cuda())
    assert torch.equal(scoring.speaker_mean_cohort(table, lab).cpu(), got)


def test_step_plan_replays_normalised_scores():
    from deeplip_amd import scoring
    from deeplip_amd.plan import StepPlan
    U, Nc, D, K = 37, 257, 64, 20
    emb, cohort, ia, ib = speaker_data(U, Nc, D)
    emb2 = speaker_data(U, Nc, D, seed=9)[0]
    ja, jb = dev_idx(ia.clamp_max(U - 6)), dev_idx(ib.clamp_max(U - 6))               # the last rows unused: the gather is recorded too
    rows = scoring.trial_rows(ja, jb, U)
    assert rows.rows is not None
    c = cohort.cuda()
    plan = StepPlan(lambda e, co: scoring.normalised_scores(e, ja, jb, co, "asnorm", K, rows=rows), emb.cuda(), c)
    try:
        first = plan.run().clone()
        assert torch.equal(first, scoring.normalised_scores(emb.cuda(), ja, jb, c, "asnorm", K))
        replay = plan(emb2.cuda(), c).clone()
        assert torch.equal(replay, scoring.normalised_scores(emb2.cuda(), ja, jb, c, "asnorm", K))
        assert not torch.equal(first, replay)
    finally:
        plan.close()


# ------------------------------------------------------------------------------------------ the entry points, end to end
def test_entry_points_end_to_end(tmp_path, monkeypatch):
    import models.audio_models.utils as au
    import test_scoring_entry as tse
    from deeplip_amd import scoring, scoring_entry as se
    monkeypatch.chdir(tmp_path)
    for env in ("DLIP_SCORE_NORM", "DLIP_SCORE_NORM_TOP_K", "DLIP_COHORT_DIR", "DLIP_COHORT_VIDEO_DIR"):
        monkeypatch.delenv(env, raising=False)
    r = np.random.default_rng(21)
    D, Nc, K = 64, 60, 15
    st = tse._store(tmp_path, r, n_spk=6, per=4, D=D, trials=300)
    run, y = st["run"], st["y"]
    vdir, vtrial = tse._write_lip_store(tmp_path, st, "utt")
    ca = r.normal(size=(Nc, D)).astype(np.float32) + 0.7
    cv = r.normal(size=(Nc, D)).astype(np.float32) - 0.3
    names = [f"c{j % 7}/m{j:03d}.wav" for j in range(Nc)]
    order = sorted(range(Nc), key=lambda j: names[j])                                  # the sorted walk both stores are read in
    scoring.EmbeddingTable(names, torch.from_numpy(ca)).save_npy_tree(str(tmp_path / "cohort_a"))
    scoring.EmbeddingTable(names, torch.from_numpy(cv)).save_npy_tree(str(tmp_path / "cohort_v"))
    ca, cv = torch.from_numpy(ca[order]), torch.from_numpy(cv[order])
    trial = str(tmp_path / "data/trial/A_grid_trial_2w")
    emb_dir = str(tmp_path / "exp" / run / "test_xv_grid")
    idx = {u: i for i, u in enumerate(st["utts"])}
    ia = torch.tensor([idx[a] for a, _ in st["pairs"]]); ib = torch.tensor([idx[b] for _, b in st["pairs"]])
    audio, video = torch.from_numpy(st["audio"]), torch.from_numpy(tse._oracle_video(st))
    kw = dict(trial_path=trial, emb_dir=emb_dir, return_scores=True)
    fkw = dict(kw, video_dir=vdir)
    norm = dict(score_norm="asnorm", top_k=K, cohort_dir=str(tmp_path / "cohort_a"))
    fnorm = dict(norm, cohort_video_dir=str(tmp_path / "cohort_v"))

    def same(got, want, what):
        e, t, s = got
        assert_close_rel(s, want.numpy(), what=what)
        assert (e, t) == scoring.eer_from_scores(y, s), what

    same(au.eer_cos_grid(run, **kw, **norm), ref_normalised(audio, ia, ib, ca, "s", K), "eer_cos_grid asnorm")
    same(au.eer_cos_grid(run, **kw, score_norm="znorm", cohort_dir=norm["cohort_dir"]), ref_normalised(audio, ia, ib, ca, "z"), "eer_cos_grid znorm")
    sv = (video.double()[ia] * video.double()[ib]).sum(1) / (video.double()[ia].norm(dim=1) * video.double()[ib].norm(dim=1)).clamp_min(1e-8)
    mu, sd = ref_cohort_stats(video, cv, K)
    want = 0.5 * ref_normalised(audio, ia, ib, ca, "s", K) + 0.5 * ref_norm(sv, ia, ib, mu, sd, "s")
    same(au.eer_cos_grid_scorefusion(run, **fkw, video_trial_path=vtrial, **fnorm), want, "scorefusion asnorm")
    want = ref_normalised(ref_znorm_cat(video, audio), ia, ib, ref_znorm_cat(cv, ca), "s", K)
    same(au.eer_cos_grid_featurefusion(run, **fkw, **fnorm), want, "featurefusion asnorm")

    # no normalisation keyword: today's path, bit for bit
    dev = torch.device("cuda", torch.cuda.current_device())
    y2, pairs = se._read_trials(trial)
    table, ta, tb = se._audio_table({"emb_dir": emb_dir}, pairs, dev)
    vt = se._video_table(vdir, [se._pattern("utt", u) for u in table.utt_ids], dev)
    for extra in ({}, {"score_norm": None}, {"score_norm": "none", "cohort_dir": str(tmp_path / "nowhere")}):
        assert np.array_equal(au.eer_cos_grid(run, **kw, **extra)[2], scoring.cosine_scores(table.emb, ta, tb).cpu().numpy())
        assert np.array_equal(au.eer_cos_grid_scorefusion(run, **fkw, video_trial_path=vtrial, **extra)[2],
                              scoring.score_fusion(table.emb, vt.emb, ta, tb).cpu().numpy())
        assert np.array_equal(au.eer_cos_grid_featurefusion(run, **fkw, **extra)[2],
                              scoring.feature_fusion_scores(table.emb, vt.emb, ta, tb).cpu().numpy())
    assert not np.array_equal(au.eer_cos_grid(run, **kw)[2], au.eer_cos_grid(run, **kw, **norm)[2])

    # the way a trainer reaches it: one argument, everything through set_paths / the environment
    try:
        se.set_paths("eer_cos_grid", trial=trial, emb_dir=emb_dir, score_norm="asnorm", top_k=K)
        monkeypatch.setenv("DLIP_COHORT_DIR", norm["cohort_dir"])
        assert au.eer_cos_grid(run) == au.eer_cos_grid(run, **kw, **norm)[:2]
        monkeypatch.delenv("DLIP_COHORT_DIR")
        with pytest.raises(ValueError, match="DLIP_COHORT_DIR"):
            au.eer_cos_grid(run)
    finally:
        se._process_paths.clear()
    with pytest.raises(ValueError, match="cohort_a_missing"):
        au.eer_cos_grid(run, **kw, score_norm="asnorm", cohort_dir=str(tmp_path / "cohort_a_missing"))
    with pytest.raises(ValueError, match="DLIP_COHORT_VIDEO_DIR"):
        au.eer_cos_grid_scorefusion(run, **fkw, video_trial_path=vtrial, **norm)


def test_train_audio_scores_with_asnorm(tmp_path, monkeypatch, capsys):
    """``test.score_norm=asnorm`` through train_audio's own ``__main__`` flow: the cohort (speaker means of the training list) is
    written once per training speaker, the one-argument ``utils.eer(log_time)`` is pointed at it, and the EER it prints is the EER
    of the normalised scores; ``Trainer.eer()`` agrees."""
    import train_audio
    from deeplip_amd import scoring, scoring_entry as se
    from models.audio_models import utils
    monkeypatch.chdir(tmp_path)
    ov = {"data.test_speakers": 4, "data.test_utt_per_spk": 3, "data.trials": 200, "data.trial_targets": 40, "data.audio_frames": 120,
          "data.n_spk": 6, "data.utt_per_spk": 3, "train.bs": 8, "train.epoch": 1, "test.score_norm": "asnorm", "test.score_norm_top_k": 4}
    monkeypatch.setattr("sys.argv", ["train_audio.py", "--mode", "test", "--gpus", "1", "--set"] + [f"{k}={v}" for k, v in ov.items()])
    try:
        train_audio.main()
        printed = [float(m) for m in re.findall(r"EER: ([0-9.]+)%", capsys.readouterr().out)]
        runs = os.listdir("exp")
        assert len(printed) == 1 and len(runs) == 1
        root = os.path.join("exp", runs[0])
        files = sorted(os.listdir(os.path.join(root, "cohort_xv")))
        assert files == [f"spk{s:05d}.npy" for s in range(6)]                          # one file per training speaker
        cohort = np.concatenate([np.load(os.path.join(root, "cohort_xv", f)) for f in files])
        assert cohort.shape == (6, 512) and np.abs(np.linalg.norm(cohort, axis=1) - 1).max() < 1e-5
        assert len(os.listdir(os.path.join(root, "train_xv"))) == 6                    # extract_train_xv ran
        e, t, s = utils.eer(runs[0], return_scores=True)
        y, _ = scoring.read_trial_list(os.path.join(root, "task.txt"))
        assert (e, t) == scoring.eer_from_scores(y, s)
        assert printed[0] == float("{:.6f}".format(e * 100))
        se.set_paths("eer", score_norm="none")
        raw = utils.eer(runs[0], return_scores=True)[2]
        assert not np.array_equal(raw, s) and np.abs(raw).max() <= 1 + 1e-5
        # the in-memory route agrees with the on-disk one
        tr = train_audio.Trainer(overrides=ov)
        tr.log_time = runs[0]
        tr.extract_test_xv()
        assert tuple(tr.eer()) == (e, t)
        tr.close()
    finally:
        se._process_paths.clear()
