"""OnlineTriplet and the triplet selectors without a GPU (-m "not gpu"): the drop-in surface (shim imports, the reference's
constructor signatures), the refusal of CPU tensors, the new entry points in header / binding / library, the fixture's own
consistency, and train_audio's option parsing."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def test_shims_export_the_reference_names_and_signatures():
    from models.audio_models import loss, utils
    for name in ("TripletSelector", "AllTripletSelector", "FunctionNegativeTripletSelector", "HardestNegativeTripletSelector",
                 "RandomNegativeTripletSelector", "SemihardNegativeTripletSelector", "hardest_negative", "random_hard_negative",
                 "semihard_negative"):
        assert hasattr(utils, name), name
    for name in ("eer", "eer_cos_grid", "feature_normalize", "EmbeddingTable"):          # every earlier name stays
        assert hasattr(utils, name), name
    assert list(inspect.signature(loss.OnlineTriplet.__init__).parameters) == ["self", "margin", "triplet_selector"]
    assert list(inspect.signature(utils.FunctionNegativeTripletSelector.__init__).parameters) == ["self", "margin", "negative_selection_fn", "cpu"]
    assert inspect.signature(utils.FunctionNegativeTripletSelector.__init__).parameters["cpu"].default is True
    for f in (utils.HardestNegativeTripletSelector, utils.RandomNegativeTripletSelector, utils.SemihardNegativeTripletSelector):
        sig = inspect.signature(f)
        assert list(sig.parameters) == ["margin", "cpu"] and sig.parameters["cpu"].default is False
        assert isinstance(f(0.3, cpu=True), utils.FunctionNegativeTripletSelector) and f(0.3).margin == 0.3
    assert list(inspect.signature(utils.AllTripletSelector.__init__).parameters) == ["self"]
    crit = loss.OnlineTriplet(0.2, utils.HardestNegativeTripletSelector(0.2))
    assert crit.margin == 0.2 and list(crit.parameters()) == []
    with pytest.raises(NotImplementedError):
        utils.FunctionNegativeTripletSelector(0.2, lambda v: 0)
    with pytest.raises(NotImplementedError):
        utils.TripletSelector().get_triplets(None, None)
    with pytest.raises(TypeError):
        loss.OnlineTriplet(0.2, object())


def test_selection_functions_follow_numpy():
    from models.audio_models.utils import hardest_negative, random_hard_negative, semihard_negative
    v = np.array([-1.0, 0.3, 0.3, 0.1], dtype=np.float32)
    assert hardest_negative(v) == 1 and hardest_negative(-np.abs(v)) is None
    assert random_hard_negative(v) in (1, 2, 3) and random_hard_negative(np.array([-1.0])) is None
    assert semihard_negative(v, 0.2) == 3 and semihard_negative(v, 0.05) is None


def test_criterion_and_selectors_refuse_cpu_tensors():
    from deeplip_amd._lib import DeepLipHipError
    from models.audio_models.loss import OnlineTriplet
    from models.audio_models.utils import AllTripletSelector, HardestNegativeTripletSelector
    x, lab = torch.zeros(8, 16), torch.zeros(8, dtype=torch.int64)
    for sel in (HardestNegativeTripletSelector(0.2), AllTripletSelector()):
        with pytest.raises(DeepLipHipError):
            sel.get_triplets(x, lab)
        with pytest.raises(DeepLipHipError):
            OnlineTriplet(0.2, sel)(x, lab)


def test_abi_carries_the_triplet_entry_points():
    import test_abi_cpu as abi
    from deeplip_amd import _lib
    names = ["dlip_triplet_mine_f32", "dlip_triplet_loss_f32", "dlip_triplet_loss_bwd_f32"]
    assert _lib.ABI_VERSION >= 53 and all(n in _lib.SIGNATURES and n in abi.header_symbols() for n in names)
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_matches_header()
    abi.test_binding_arity_matches_header()
    from deeplip_amd import build
    assert "triplet_ops.hip" in build.SOURCES


def test_fixture_is_consistent():
    g = np.load(os.path.join(GOLDEN, "triplet_golden.npz"))
    assert os.path.getsize(os.path.join(GOLDEN, "triplet_golden.npz")) < 1 << 20
    d = json.loads(str(g["cases"]))
    shapes = {(c["B"], c["S"], c["E"]) for c in d["cases"].values()}
    assert {(64, 8, 64), (256, 57, 512), (60, 57, 512)} <= shapes and {c["gain"] for c in d["cases"].values()} >= {1.0, 0.1, 0.02}
    for name, c in d["cases"].items():
        lab = g[f"{name}.labels"]
        assert lab.shape == (c["B"],) and lab.min() >= 0 and lab.max() < c["S"]
        if c["S"] == 1:
            assert int(g[f"{name}.n"]) == 0
            continue
        pairs, gap = g[f"{name}.pairs"].astype(np.int64), g[f"{name}.gap"]
        assert (pairs[:, 0] < pairs[:, 1]).all() and (lab[pairs[:, 0]] == lab[pairs[:, 1]]).all() and (gap >= 0).all()
        assert (gap < 100 * float(g[f"{name}.dot_err"])).mean() <= 0.02
        for sel in ("hardest", "all"):
            for key in (f"{name}.{sel}.triplets", f"{name}.{sel}.triplets64"):
                if key not in g.files:
                    continue
                t = g[key].astype(np.int64)
                assert t.shape[1] == 3 and (t[:, 0] < t[:, 1]).all()
                assert (lab[t[:, 0]] == lab[t[:, 1]]).all() and (lab[t[:, 0]] != lab[t[:, 2]]).all()
                assert len(t) == int(g[f"{name}.{sel}.n64" if key.endswith("64") else f"{name}.{sel}.n"])
            assert np.isfinite(g[f"{name}.{sel}.dx64"]).all() and float(g[f"{name}.{sel}.loss64"]) > 0
        assert len(g[f"{name}.hardest.triplets"]) <= len(pairs)


def test_train_audio_builds_the_criterion_the_config_names():
    import train_audio
    from deeplip_amd import triplet as tp
    from models.audio_models.loss import AAMSoftmax, CrossEntropy, LMCL, OnlineTriplet
    crit = train_audio.build_criterion({"loss": "Triplet"}, 64, 5)
    assert isinstance(crit, OnlineTriplet) and crit.margin == 0.2 and crit.triplet_selector.mode == tp.MODE_HARDEST
    for name, mode in tp.MODES.items():
        crit = train_audio.build_criterion({"loss": "Triplet", "triplet": {"margin": 0.3, "selector": name}}, 64, 5)
        assert crit.triplet_selector.mode == mode and crit.margin == 0.3 and crit.triplet_selector.margin in (0.3, 0.0)
    with pytest.raises(ValueError):
        train_audio.build_criterion({"loss": "Triplet", "triplet": {"selector": "easiest"}}, 64, 5)
    with pytest.raises(ValueError):
        train_audio.build_criterion({"loss": "Triplet", "triplet": {"margn": 0.1}}, 64, 5)
    with pytest.raises(ValueError):
        train_audio.build_criterion({"loss": "Triplet", "freeze_encoder": True}, 64, 5)
    lm = train_audio.build_criterion({"loss": "LMCL", "scale": 30, "margin": [0.2, 0.35]}, 64, 5)
    assert isinstance(lm, LMCL) and lm.margin == 0.2 and lm.s == 30 and tuple(lm.weights.shape) == (5, 64)
    assert isinstance(train_audio.build_criterion({"loss": "AAMSoftmax", "scale": 30, "margin": [0.2, 0.2]}, 64, 5), AAMSoftmax)
    assert isinstance(train_audio.build_criterion({"loss": "CrossEntropy"}, 64, 5), CrossEntropy)
    assert isinstance(train_audio.build_criterion({"loss": "Contrastive"}, 64, 5), CrossEntropy)      # the fall-through stays
    import yaml
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "conf", "audio_config.yaml")) as f:
        opts = yaml.safe_load(f)["train"]
    assert opts["loss"] == "LMCL" and "triplet" not in opts                   # the shipped config: no active key changed
