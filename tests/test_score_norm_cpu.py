"""Cohort score normalisation without a GPU (-m "not gpu"): the two entry points in header / binding / library, their argument
refusals through ctypes, the refusals of ops / scoring before any launch, the keyword surface and resolution order of the
scoring entry points, and the host half of the cohort helpers."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

NAMES = ["eer", "eer_cos_lomgrid", "eer_cos_grid", "eer_plda_lomgrid", "eer_plda_grid", "eer_cos_lomgrid_scorefusion",
         "eer_cos_grid_scorefusion", "eer_cos_lomgrid_featurefusion", "eer_cos_grid_featurefusion"]
NORM_KEYS = ("score_norm", "top_k", "cohort_dir")


def _modules():
    import models.audio_models.utils as au
    import models.fusion_models.utils as fu
    return {"fusion": fu, "audio": au}


def test_abi_carries_the_score_norm_entry_points():
    import test_abi_cpu as abi
    from deeplip_amd import _lib, build
    names = ["dlip_topk_stats_f32", "dlip_score_norm_f32"]
    assert all(n in _lib.SIGNATURES and n in abi.header_symbols() for n in names)
    lib = _lib.lib()
    assert lib.dlip_abi_version() == _lib.ABI_VERSION >= 58
    assert all(hasattr(lib, n) for n in names)
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_matches_header()
    abi.test_binding_arity_matches_header()
    assert "score_norm_ops.hip" in build.SOURCES


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """DLIP_EINVAL (-1) straight from the host-side checks: nothing is launched, so fake non-null addresses are never touched."""
    from deeplip_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(4096)                       # non-null, never dereferenced

    def topk(s=p, R=2, N=8, ld=8, K=3, mean=p, sd=p):
        return lib.dlip_topk_stats_f32(s, R, N, ld, K, mean, sd, None)

    for bad in (dict(s=None), dict(mean=None), dict(sd=None), dict(R=0), dict(R=-1), dict(K=0), dict(K=9), dict(K=-3), dict(N=0),
                dict(ld=7), dict(N=32769, ld=32769, K=300), dict(N=40000, ld=40000, K=40000)):
        assert topk(**bad) == -1, bad

    def norm(s=p, ia=p, ib=p, n=5, mu=p, sd=p, U=3, mode=2, out=p):
        return lib.dlip_score_norm_f32(s, ia, ib, n, mu, sd, U, mode, 1e-6, 1.0, 0, out, None)

    for bad in (dict(s=None), dict(ia=None), dict(ib=None), dict(mu=None), dict(sd=None), dict(out=None), dict(n=0), dict(U=0),
                dict(mode=3), dict(mode=-1)):
        assert norm(**bad) == -1, bad


def test_ops_and_scoring_refuse_cpu_tensors_and_bad_shapes():
    from deeplip_amd import ops, scoring
    from deeplip_amd._lib import DeepLipHipError
    e, c = torch.zeros(6, 8), torch.zeros(5, 8)
    ia, ib = torch.zeros(4, dtype=torch.int32), torch.ones(4, dtype=torch.int32)
    with pytest.raises(DeepLipHipError):
        ops.topk_stats(torch.zeros(3, 7), 2)
    with pytest.raises(DeepLipHipError):
        ops.score_norm(torch.zeros(4), ia, ib, torch.zeros(6), torch.ones(6))
    with pytest.raises(DeepLipHipError):
        ops.cohort_stats(e, c, top_k=3)
    with pytest.raises(DeepLipHipError):
        scoring.normalised_scores(e, ia, ib, c, "asnorm", 3)
    with pytest.raises(DeepLipHipError):
        scoring.score_fusion_normalised(e, e, ia, ib, c, c)
    with pytest.raises(DeepLipHipError):
        scoring.feature_fusion_scores_normalised(e, e, ia, ib, c, c)
    with pytest.raises(DeepLipHipError):
        scoring.speaker_mean_cohort(e, [0, 0, 1, 1, 2, 2])
    # values are refused before the device is looked at: the same errors on a box with no GPU
    for k in (0, 6, -1):
        with pytest.raises(ValueError, match="top_k"):
            ops.cohort_stats(e, c, top_k=k)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.cohort_stats(torch.zeros(6, 6), torch.zeros(5, 6))
    with pytest.raises(ValueError, match="D="):
        ops.cohort_stats(e, torch.zeros(5, 12))
    with pytest.raises(ValueError, match="32768"):
        ops.cohort_stats(e, torch.zeros(32769, 8))
    with pytest.raises(ValueError, match="chunk_rows"):
        ops.cohort_stats(e, c, chunk_rows=0)
    for k, n in ((0, None), (8, None), (4, 3), (1, 9), (1, 0)):
        with pytest.raises(ValueError):
            ops.topk_stats(torch.zeros(3, 7), k, n)
    with pytest.raises(ValueError, match="32768"):
        ops.topk_stats(torch.zeros(1, 32769), 5)
    with pytest.raises(ValueError, match="top_k"):
        scoring.normalised_scores(e, ia, ib, c, "asnorm", 0)
    with pytest.raises(ValueError, match="multiple of 4"):
        scoring.normalised_scores(torch.zeros(6, 6), ia, ib, torch.zeros(5, 6))
    with pytest.raises(ValueError, match="32768"):
        scoring.normalised_scores(e, ia, ib, torch.zeros(32769, 8))
    with pytest.raises(ValueError, match="D="):
        scoring.normalised_scores(e, ia, ib, torch.zeros(5, 4))
    with pytest.raises(ValueError, match="none of"):
        scoring.normalised_scores(e, ia, ib, c, "qnorm")
    with pytest.raises(ValueError):
        scoring.normalised_scores(e, ia, ib, c, "none")
    with pytest.raises(ValueError, match="cohort rows"):
        scoring.feature_fusion_scores_normalised(e, e, ia, ib, c, torch.zeros(4, 8))


def test_kinds_and_top_k():
    from deeplip_amd import scoring
    assert scoring.score_norm_kind(None) is None and scoring.score_norm_kind("none") is None and scoring.score_norm_kind("None") is None
    assert scoring.score_norm_kind("ASnorm") == "asnorm"
    assert scoring.SCORE_NORM_KINDS == {"znorm": ("z", False), "tnorm": ("t", False), "snorm": ("s", False), "asnorm": ("s", True)}
    assert scoring.cohort_top_k("snorm", 300, 1000) is None and scoring.cohort_top_k("znorm", 5, 1000) is None
    assert scoring.cohort_top_k("asnorm", None, 1000) == 300 and scoring.cohort_top_k("asnorm", None, 57) == 57
    assert scoring.cohort_top_k("asnorm", 20, 57) == 20 and scoring.cohort_top_k("asnorm", 400, 57) == 57
    from deeplip_amd import ops
    assert ops.cohort_chunk_rows(25834, 16384) == 4096 and ops.cohort_chunk_rows(100, 16384) == 100
    assert ops.cohort_chunk_rows(25834, 16384) * 16384 * 4 <= 256 << 20 and ops.cohort_chunk_rows(50, 300, 5) == 5


def test_entry_points_take_the_new_keywords():
    """Still ONE positional parameter; the normalisation's parameters keyword-only with defaults of None, the lip cohort on the
    fusion variants only."""
    for mod in _modules().values():
        for n in NAMES:
            ps = inspect.signature(getattr(mod, n)).parameters
            first = list(ps.values())[0]
            assert first.name == "exp_dir" and first.kind == first.POSITIONAL_OR_KEYWORD
            assert [p.name for p in ps.values() if p.kind != p.KEYWORD_ONLY] == ["exp_dir"], n
            for k in NORM_KEYS:
                assert ps[k].kind == ps[k].KEYWORD_ONLY and ps[k].default is None, (n, k)
            assert ("cohort_video_dir" in ps) == n.endswith("fusion"), n
            if n.endswith("fusion"):
                assert ps["cohort_video_dir"].kind == ps["cohort_video_dir"].KEYWORD_ONLY and ps["cohort_video_dir"].default is None


def test_resolution_order_of_the_new_keys(tmp_path, monkeypatch):
    """keyword > set_paths(name) > set_paths() > environment > nothing; with nothing set the keys are absent and no
    normalisation is requested."""
    from deeplip_amd import scoring_entry as se
    monkeypatch.chdir(tmp_path)
    for env in ("DLIP_SCORE_NORM", "DLIP_SCORE_NORM_TOP_K", "DLIP_COHORT_DIR", "DLIP_COHORT_VIDEO_DIR"):
        monkeypatch.delenv(env, raising=False)
    assert {se._ENV[k] for k in ("score_norm", "top_k", "cohort_dir", "cohort_video_dir")} == \
        {"DLIP_SCORE_NORM", "DLIP_SCORE_NORM_TOP_K", "DLIP_COHORT_DIR", "DLIP_COHORT_VIDEO_DIR"}
    d = se.FUSION_DEFAULTS["eer_cos_grid"]
    res = lambda kw=None, name="eer_cos_grid": se._resolve(name, se.FUSION_DEFAULTS[name], "run", kw or {})   # noqa: E731
    try:
        p = res()
        assert not any(k in p for k in ("score_norm", "top_k", "cohort_dir", "cohort_video_dir"))
        assert se._norm_request("eer_cos_grid", p) is None
        assert d == {"trial": "data/data_audio/trial_grid_2w.txt", "sub": "test_em_grid"}      # the defaults table is untouched
        for key, env, vals in (("score_norm", "DLIP_SCORE_NORM", ("znorm", "tnorm", "snorm", "asnorm")),
                               ("top_k", "DLIP_SCORE_NORM_TOP_K", ("11", "12", "13", 14)),
                               ("cohort_dir", "DLIP_COHORT_DIR", ("c_env", "c_all", "c_one", "c_kw")),
                               ("cohort_video_dir", "DLIP_COHORT_VIDEO_DIR", ("v_env", "v_all", "v_one", "v_kw"))):
            monkeypatch.setenv(env, vals[0])
            assert res()[key] == vals[0]
            se.set_paths(**{key: vals[1]})
            assert res()[key] == vals[1]
            se.set_paths("eer_cos_grid", **{key: vals[2]})
            assert res()[key] == vals[2]
            assert res(name="eer_cos_lomgrid")[key] == vals[1]
            assert res({key: vals[3]})[key] == vals[3]
        with pytest.raises(KeyError):
            se.set_paths("eer", cohort="x")
    finally:
        se._process_paths.clear()


def test_requests_without_a_cohort_and_plda_requests_are_value_errors(tmp_path, monkeypatch):
    """Checked before any device work: the same on a box without a GPU."""
    from deeplip_amd import scoring_entry as se
    monkeypatch.chdir(tmp_path)
    for env in ("DLIP_SCORE_NORM", "DLIP_SCORE_NORM_TOP_K", "DLIP_COHORT_DIR", "DLIP_COHORT_VIDEO_DIR"):
        monkeypatch.delenv(env, raising=False)
    (tmp_path / "cohort").mkdir()
    try:
        for mod in _modules().values():
            for n in NAMES:
                f = getattr(mod, n)
                if "plda" in n:
                    with pytest.raises(ValueError, match="PLDA"):
                        f("run", score_norm="asnorm", cohort_dir=str(tmp_path / "cohort"))
                    monkeypatch.setenv("DLIP_SCORE_NORM", "snorm")          # the way a trainer's one-argument call reaches it
                    with pytest.raises(ValueError, match="PLDA"):
                        f("run")
                    monkeypatch.delenv("DLIP_SCORE_NORM")
                    continue
                with pytest.raises(ValueError, match="DLIP_COHORT_DIR"):
                    f("run", score_norm="asnorm")
                with pytest.raises(ValueError, match="nowhere"):
                    f("run", score_norm="snorm", cohort_dir=str(tmp_path / "nowhere"))
                with pytest.raises(ValueError, match="none of"):
                    f("run", score_norm="qnorm", cohort_dir=str(tmp_path / "cohort"))
                with pytest.raises(ValueError, match="top_k"):
                    f("run", score_norm="asnorm", top_k=0, cohort_dir=str(tmp_path / "cohort"))
                if n.endswith("fusion"):
                    with pytest.raises(ValueError, match="DLIP_COHORT_VIDEO_DIR"):
                        f("run", score_norm="asnorm", cohort_dir=str(tmp_path / "cohort"))
                    with pytest.raises(ValueError, match="nolips"):
                        f("run", score_norm="asnorm", cohort_dir=str(tmp_path / "cohort"), cohort_video_dir=str(tmp_path / "nolips"))
        se.set_paths("eer_cos_grid", score_norm="asnorm")
        with pytest.raises(ValueError, match="DLIP_COHORT_DIR"):
            _modules()["audio"].eer_cos_grid("run")
    finally:
        se._process_paths.clear()


def test_speaker_groups_host_half():
    from deeplip_amd import scoring
    order, gptr, labels = scoring.speaker_groups([3, 1, 3, 7, 1, 3])
    assert order.tolist() == [1, 4, 0, 2, 5, 3]                       # sorted by label, rows of one speaker in their own order
    assert gptr.tolist() == [0, 2, 5, 6] and gptr.dtype == np.int32   # the last speaker has a single row
    assert labels == [1, 3, 7]
    order, gptr, labels = scoring.speaker_groups(["s2", "s10", "s2"])
    assert order.tolist() == [1, 0, 2] and gptr.tolist() == [0, 1, 3] and labels == ["s10", "s2"]
    order, gptr, labels = scoring.speaker_groups(np.array([5]))
    assert order.tolist() == [0] and gptr.tolist() == [0, 1] and labels == [5]
    with pytest.raises(ValueError):
        scoring.speaker_groups([])
    with pytest.raises(ValueError, match="labels"):
        scoring.speaker_mean_cohort(torch.zeros(4, 8), [0, 1, 1])


def test_used_rows_host_half():
    from deeplip_amd import scoring
    used, ra, rb = scoring._used_rows_host(np.array([5, 2, 5]), np.array([2, 7, 7]), 9)
    assert used.tolist() == [2, 5, 7] and ra.tolist() == [1, 0, 1] and rb.tolist() == [0, 2, 2] and ra.dtype == np.int32
    used, ra, rb = scoring._used_rows_host(np.array([2, 0]), np.array([1, 1]), 3)
    assert used is None and ra.tolist() == [2, 0] and rb.tolist() == [1, 1]
    for ia, ib in (([0, 3], [1, 1]), ([-1, 0], [1, 1]), ([], [])):
        with pytest.raises(ValueError):
            scoring._used_rows_host(np.array(ia), np.array(ib), 3)


def test_load_cohort_walks_sorted(tmp_path):
    from deeplip_amd import scoring, scoring_entry as se
    t = scoring.EmbeddingTable(["s2/b.wav", "s1/z.wav", "s1/a.wav", "top.wav"], torch.arange(16, dtype=torch.float32).view(4, 4))
    t.save_npy_tree(str(tmp_path / "c"))
    got = se.load_cohort(str(tmp_path / "c"), None)
    assert got.utt_ids == ["top.npy", "s1/a.npy", "s1/z.npy", "s2/b.npy"]
    assert got.emb.tolist() == [t.emb[i].tolist() for i in (3, 2, 1, 0)]
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="no .npy"):
        se.load_cohort(str(tmp_path / "empty"), None)


def test_train_audio_reads_the_optional_keys():
    import os
    import yaml
    from conftest import ROOT
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        test = yaml.safe_load(f)["test"]
    assert not any(k in test for k in ("score_norm", "score_norm_top_k", "cohort"))        # the shipped config is as it was
    import train_audio
    tr = train_audio.Trainer.__new__(train_audio.Trainer)
    tr.test_opts = {}
    assert tr.score_norm() == (None, 300, "speaker_mean")
    tr.test_opts = {"score_norm": "asnorm", "score_norm_top_k": 50, "cohort": "utterances"}
    assert tr.score_norm() == ("asnorm", 50, "utterances")
    tr.test_opts = {"cohort": "everyone"}
    with pytest.raises(ValueError, match="test.cohort"):
        tr.score_norm()
