"""Lipreading(backbone_type='shufflenet') without a GPU: construction for every width, the state-dict schema against the manifest
captured from the reference (tests/golden/capture_shufflenet_golden.py), strict loading, and the invariants of the packed channel
layout (deeplip_amd/shufflenet.py) and of the packed weights."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from deeplip_amd import shufflenet as sn
from deeplip_amd import weightgen as wg
from deeplip_amd.video import Lipreading

TCN_OPTS = {"num_layers": 4, "kernel_size": [3, 5, 7], "dropout": 0.2, "dwpw": False, "width_mult": 1}
WIDTHS = (0.5, 1.0, 1.5, 2.0)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "shufflenet_golden.npz"))


def make(width, relu_type="prelu", extract_feats=True):
    return Lipreading(hidden_dim=256, backbone_type="shufflenet", num_classes=54, relu_type=relu_type,
                      tcn_options=TCN_OPTS, width_mult=width, extract_feats=extract_feats)


@pytest.mark.parametrize("width", WIDTHS)
def test_state_dict_matches_reference_manifest(gold, width):
    m = make(width)
    want = json.loads(str(gold["manifest_w" + str(width).replace(".", "p")]))
    got = sorted([k, list(v.shape)] for k, v in m.state_dict().items())
    assert got == want
    assert len(got) == 543
    assert m.backend_out == (2048 if width == 2.0 else 1024) and m.frontend_nout == 24
    assert m.stage_out_channels == m.backend_out
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert torch.equal(m.state_dict()["trunk.0.0.banch1.0.weight"], torch.from_numpy(sd["trunk.0.0.banch1.0.weight"]))


def test_relu_variant_and_shim_imports():
    m = make(1.0, relu_type="relu")
    assert not any(k.startswith("frontend3D.2") for k in m.state_dict())
    from models.video_models.shufflenetv2 import InvertedResidual, ShuffleNetV2, channel_shuffle, conv_1x1_bn, conv_bn  # noqa: F401
    from models.video_models.model import ShuffleNetV2 as S2
    assert S2 is ShuffleNetV2
    with pytest.raises(NotImplementedError):
        ShuffleNetV2(width_mult=1.0)(torch.zeros(1, 3, 224, 224))
    with pytest.raises(ValueError):
        ShuffleNetV2(width_mult=0.75)


def test_channel_shuffle_restatement():
    x = torch.arange(2 * 6 * 1 * 1, dtype=torch.float32).view(2, 6, 1, 1)
    y = sn.channel_shuffle(x, 2)
    assert y[0, :, 0, 0].tolist() == [0, 3, 1, 4, 2, 5]


@pytest.mark.parametrize("C", [48, 96, 192, 116, 232, 464, 176, 352, 704, 244, 488, 976])
def test_layout_is_a_bijection_onto_logical_channels(C):
    lay = sn.unit_layout(C)
    h, hp = lay.half, lay.hp
    assert hp % 4 == 0 and h <= hp < h + 4 and lay.pitch == 2 * hp
    phys = lay.phys()
    assert len(set(phys.tolist())) == C and int(phys.min()) >= 0 and int(phys.max()) < lay.pitch
    pads = sorted(set(range(lay.pitch)) - set(phys.tolist()))
    assert pads == list(range(h, hp)) + list(range(hp + h, 2 * hp))
    # x1 / x2 of the next stride-1 unit are the aligned slices [0, hp) and [hp, 2hp)
    assert phys[:h].tolist() == list(range(h)) and phys[h:].tolist() == list(range(hp, hp + h))
    # the two branches' shuffled positions (channel_shuffle: j -> 2j, 2j + 1) cover the logical channels exactly once
    a, b = sn.shuffle_positions(h, hp, 0), sn.shuffle_positions(h, hp, 1)
    assert sorted(a.tolist() + b.tolist()) == sorted(phys.tolist())
    logical = torch.arange(2 * h)
    x = torch.arange(2 * h) * 10.0                                 # cat(first, second) in logical order
    shuffled = sn.channel_shuffle(x.view(1, 2 * h, 1, 1), 2).view(-1)
    stored = torch.zeros(lay.pitch)
    stored[a] = x[:h]
    stored[b] = x[h:]
    assert torch.equal(lay.to_logical(stored), shuffled)
    assert logical.numel() == C


def test_padded_layouts_are_the_odd_halves():
    padded = {C: sn.unit_layout(C).hp for C in (48, 96, 192, 116, 232, 464, 176, 352, 704, 244, 488, 976) if C // 2 % 4}
    assert padded == {116: 60, 244: 124}


@pytest.mark.parametrize("width", [1.0, 2.0])
def test_packed_weights_are_zero_on_padding_channels(width):
    m = make(width)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.eval()
    pk = m.trunk.pack("cpu")
    lays = pk["layouts"]
    for i, (u, p, lin) in enumerate(zip(m.trunk.units(), pk["units"], lays[:-1])):
        lout = lays[i + 1]
        assert (p.K, p.hp) == (lout.half, lout.hp)
        pads_in = sorted(set(range(lin.pitch)) - set(lin.phys().tolist()))
        if p.stride == 2:
            assert p.b1["dw_w"].shape == (9, lin.pitch) and p.b1["w"].shape[0] % 32 == 0 and p.b1["w"].shape[1] % 64 == 0
            assert not p.b1["dw_w"][:, pads_in].any() and not p.b1["dw_b"][pads_in].any() and not p.b1["w"][pads_in].any()
            assert not p.pw1.w[..., pads_in].any()
        assert p.pw1.w.shape[0] == p.hp and not p.pw1.w[p.K:].any() and not p.pw1.b[p.K:].any()
        assert not p.b2["dw_w"][:, p.K:].any() and not p.b2["w"][p.K:].any() and not p.b2["w"][:, p.K:].any()
    last_pads = sorted(set(range(lays[-1].pitch)) - set(lays[-1].phys().tolist()))
    assert not pk["last"].w[..., last_pads].any()
    assert len(pk["units"]) == 16 and sum(1 for p in pk["units"] if p.stride == 2) == 3


def test_stem_pack_and_input_sizes():
    m = make(1.0)
    p = sn.pack_stem24(m.frontend3D[0], m.frontend3D[1], None, "cpu")
    assert p.w.shape == (248, 32) and not p.w[245:].any() and not p.w[:, 24:].any()
    assert sn.final_map_size(88, 88) == (3, 3) and sn.final_map_size(112, 112) == (4, 4)
    sn.check_input_size(88, 88)
    sn.check_input_size(112, 112)
    for s in (64, 176):
        with pytest.raises(ValueError):
            sn.check_input_size(s, s)


def test_training_mode_raises_not_implemented():
    m = make(1.0)
    m.train()
    with pytest.raises(NotImplementedError, match="[Ss]huffle[Nn]et.*training|training.*[Ss]huffle"):
        m(torch.zeros(1, 1, 2, 88, 88), [2])
