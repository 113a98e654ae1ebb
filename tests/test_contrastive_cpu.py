"""Contrastive and the pair selectors without a GPU (-m "not gpu"): the interface, the refusal of CPU tensors, the new entry point in
header / binding / library, train_audio's option parsing, and the conditions the GPU tests' cases rest on (contrastive_ref.py), asserted
here so that a changed generator cannot hide them."""
import inspect
import os

import pytest
import torch

import contrastive_ref as cr
from conftest import GOLDEN


def test_interface_and_shims():
    from deeplip_amd import pairs
    from models.audio_models import loss, utils
    import models.fusion_models.utils as futils
    for mod in (utils, futils):
        for name in ("AllPairSelector", "HardNegativePairSelector", "make_pair_selector"):
            assert getattr(mod, name) is getattr(pairs, name), name
    assert list(inspect.signature(loss.Contrastive.__init__).parameters) == ["self", "margin", "pair_selector"]
    crit = loss.Contrastive(0.5, pairs.HardNegativePairSelector())
    assert crit.margin == 0.5 and list(crit.parameters()) == [] and crit.state_dict() == {}
    assert pairs.make_pair_selector("all").mode == pairs.MODE_ALL and pairs.make_pair_selector("hard_negative").mode == pairs.MODE_HARD_NEGATIVE
    assert "adambielski" in pairs.HardNegativePairSelector.__doc__ and "LDS" in pairs.HardNegativePairSelector.__doc__
    with pytest.raises(ValueError):
        pairs.make_pair_selector("easiest")
    with pytest.raises(TypeError):
        loss.Contrastive(0.5, object())
    with pytest.raises(NotImplementedError):
        pairs.PairSelector().get_pairs(None, None)


def test_criterion_and_selectors_refuse_cpu_tensors():
    from deeplip_amd import pairs
    from deeplip_amd._lib import DeepLipHipError
    from models.audio_models.loss import Contrastive
    x, lab = torch.zeros(8, 16, requires_grad=True), torch.zeros(8, dtype=torch.int64)
    for sel in (pairs.AllPairSelector(), pairs.HardNegativePairSelector()):
        with pytest.raises(DeepLipHipError):
            sel.get_pairs(x.detach(), lab)
        with pytest.raises(DeepLipHipError):
            Contrastive(0.5, sel)(x, lab)
        with pytest.raises(DeepLipHipError):
            Contrastive(0.5, sel)(x.detach(), lab)


def test_abi_carries_the_contrastive_entry_point():
    import test_abi_cpu as abi
    from deeplip_amd import _lib, build
    assert _lib.ABI_VERSION >= 66 and "dlip_contrastive_loss_f32" in _lib.SIGNATURES and "dlip_contrastive_loss_f32" in abi.header_symbols()
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_matches_header()
    abi.test_binding_arity_matches_header()
    assert "contrastive_ops.hip" in build.SOURCES


def test_train_audio_builds_the_criterion_the_config_names():
    import train_audio
    from deeplip_amd import pairs
    from models.audio_models.loss import Contrastive, CrossEntropy
    crit = train_audio.build_criterion({"loss": "OnlineContrastive"}, 64, 5)
    assert isinstance(crit, Contrastive) and crit.margin == 0.5 and crit.pair_selector.mode == pairs.MODE_HARD_NEGATIVE
    for name, mode in pairs.MODES.items():
        crit = train_audio.build_criterion({"loss": "OnlineContrastive", "contrastive": {"margin": 0.3, "selector": name}}, 64, 5)
        assert crit.pair_selector.mode == mode and crit.margin == 0.3
    with pytest.raises(ValueError):
        train_audio.build_criterion({"loss": "OnlineContrastive", "contrastive": {"selector": "easiest"}}, 64, 5)
    with pytest.raises(ValueError):
        train_audio.build_criterion({"loss": "OnlineContrastive", "contrastive": {"margn": 0.1}}, 64, 5)
    with pytest.raises(ValueError):
        train_audio.build_criterion({"loss": "OnlineContrastive", "freeze_encoder": True}, 64, 5)
    assert isinstance(train_audio.build_criterion({"loss": "Contrastive"}, 64, 5), CrossEntropy)      # upstream's fall-through stays
    assert "Online" in train_audio.build_criterion.__doc__
    import yaml
    with open(os.path.join(os.path.dirname(GOLDEN), "..", "conf", "audio_config.yaml")) as f:
        opts = yaml.safe_load(f)["train"]
    assert opts["loss"] == "LMCL" and "contrastive" not in opts and "asoftmax" not in opts      # the shipped config: no active key changed


@pytest.mark.parametrize("name", sorted(cr.CASES))
def test_cases_meet_the_conditions_on_margin_and_fragile_rows(name):
    f = cr.case_facts(name)
    print(f"{name}: cos_err {f['cos_err']:.3e}, {100 * f['active']:.2f} % of the negative pairs active at margin {cr.MARGIN}, nearest at "
          f"{f['clear'] / f['cos_err']:.0f} x cos_err, fragile rows {len(f['fragile'])}/{f['rows']}")
    assert f["active"] >= 0.01
    assert f["clear"] >= cr.MARGIN_CLEAR * f["cos_err"]
    assert f["rows"] > 0 and len(f["fragile"]) <= cr.FRAGILE_SHARE * f["rows"]


def test_restatement_is_the_cosine_embedding_loss():
    """The definition's own anchor: on all pairs the fp64 restatement equals torch.nn.CosineEmbeddingLoss (the clamp aside: no row is near it)."""
    x, labels = cr.case_inputs("b33")
    pos, neg, _ = cr.select64(x, labels, "all")
    loss, _ = cr.restate(x, pos, neg, cr.MARGIN, torch.float64)
    pairs_ = torch.tensor(pos + neg)
    y = torch.cat([torch.ones(len(pos)), -torch.ones(len(neg))]).double()
    want = torch.nn.CosineEmbeddingLoss(margin=cr.MARGIN)(x.double()[pairs_[:, 0]], x.double()[pairs_[:, 1]], y)
    assert len(pos) + len(neg) == 33 * 32 // 2 and abs(loss - float(want)) <= 1e-12
