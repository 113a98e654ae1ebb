"""Host-side pieces of the ResNet speech encoder's statistics / attentive pooling and two-layer head (-m "not gpu"): what the constructor
builds for every (pooling, fc_layers) pair, what it refuses, the shortest utterance, train_audio's fill-in of `feat_dim`, the op wrappers'
CPU refusal and the library's entry points (ABI 59).  DESIGN.md 4b holds the definitions."""
import ctypes

import pytest
import torch

POOLINGS = ("average", "statistic", "attentive_statistic")


def _opts(pooling="average", fc_layers=1, hidden=(16, 32), feat_dim=None, **kw):
    o = {"input_dim": 1, "hidden_dim": list(hidden), "residual_block_layers": [1] * len(hidden), "fc_layers": fc_layers,
         "embedding_dim": 12, "pooling": pooling}
    if feat_dim is not None:
        o["feat_dim"] = feat_dim
    o.update(kw)
    return {"arch": "resnet", "resnet": o}


def _net(*a, **kw):
    from models.resnet import SpeakerEmbNet
    return SpeakerEmbNet(_opts(*a, **kw))


def _trunk_keys(net):
    return {k for k in net.state_dict() if k.startswith(("conv1.", "bn1.", "layers."))}


@pytest.mark.parametrize("hidden", [(16, 32), (8, 16, 32)])
@pytest.mark.parametrize("feat_dim", [8, 9, 24])
@pytest.mark.parametrize("fc_layers", [1, 2])
@pytest.mark.parametrize("pooling", POOLINGS)
def test_state_dict_keys_and_shapes(pooling, fc_layers, feat_dim, hidden):
    net = _net(pooling, fc_layers, hidden, feat_dim, attention_hidden_size=5)
    sd = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    k = len(hidden) - 1
    C, E = hidden[-1], 12
    D = (((feat_dim - 1) >> k) + 1) * C
    P = C if pooling == "average" else 2 * D
    head = {k_: v for k_, v in sd.items() if k_ not in _trunk_keys(net)}
    want = {}
    if pooling == "attentive_statistic":
        want.update({"pooling.W": (5, D), "pooling.b": (1, 5), "pooling.v": (5, 1), "pooling.k": (1, 1)})
    if fc_layers == 1:
        want.update({"fc.weight": (E, P), "fc.bias": (E,)})
    else:
        want.update({"fc1.weight": (E, P), "fc1.bias": (E,), "fc2.weight": (E, E), "fc2.bias": (E,), "fc1_bn.weight": (E,),
                     "fc1_bn.bias": (E,), "fc1_bn.running_mean": (E,), "fc1_bn.running_var": (E,), "fc1_bn.num_batches_tracked": ()})
    assert head == want
    assert net.min_frames() == ((1 << k) + 1 if pooling == "statistic" else 1)
    assert net.frames_consumed() == 0


def test_average_single_layer_key_set_is_the_shipped_one():
    """(`average`, 1): the module a checkpoint of the shipped configuration loads into -- trunk keys + fc.weight / fc.bias, nothing
    else, with or without a feat_dim in the options."""
    want = {"conv1.weight", "fc.weight", "fc.bias"}
    for bn in ("bn1", "layers.0.0.bn1", "layers.0.0.bn2", "layers.1.0.bn1", "layers.1.0.bn2", "layers.1.0.downsample.1"):
        want |= {f"{bn}.{s}" for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    want |= {"layers.0.0.conv1.weight", "layers.0.0.conv2.weight", "layers.1.0.conv1.weight", "layers.1.0.conv2.weight",
             "layers.1.0.downsample.0.weight"}
    for fd in (None, 24):
        net = _net("average", 1, feat_dim=fd)
        assert set(net.state_dict()) == want
        assert tuple(net.fc.weight.shape) == (12, 32)
        assert net.feat_dim is None                       # ignored for average: any F is taken


def test_attention_hidden_size_defaults_to_64():
    assert _net("attentive_statistic", 1, feat_dim=8).pooling.hidden_size == 64


def test_refusals():
    for pooling in ("statistic", "attentive_statistic"):
        with pytest.raises(ValueError, match="feat_dim"):
            _net(pooling, 1)
    for fc in (0, 3):
        with pytest.raises(NotImplementedError):
            _net("average", fc)
    for pooling in ("mono_head_attention", "max"):
        with pytest.raises(NotImplementedError):
            _net(pooling, 1, feat_dim=8)
    with pytest.raises(ValueError):
        _net("statistic", 1, hidden=(16, 30), feat_dim=8)          # last width % 4


def test_wrong_feature_dimension_is_refused_before_any_launch():
    net = _net("statistic", 2, feat_dim=8).eval()
    with pytest.raises(ValueError, match="feat_dim"):
        net.extract_embedding(torch.zeros(2, 1, 9, 12))
    net.train()
    with pytest.raises(ValueError, match="feat_dim"):
        net.extract_embedding(torch.zeros(2, 1, 9, 12))


def test_train_audio_fills_feat_dim_from_the_data_section():
    import train_audio
    m = {"arch": "resnet", "resnet": _opts("statistic", 2)["resnet"]}
    assert "feat_dim" not in m["resnet"]
    net = train_audio.build_model(m, {"feat_dim": 24})
    assert net.feat_dim == 24 and tuple(net.fc1.weight.shape) == (12, 2 * 12 * 32) and m["resnet"]["feat_dim"] == 24
    net = train_audio.build_model({"arch": "resnet", "resnet": _opts("statistic", 2)["resnet"]}, {})
    assert net.feat_dim == 40                                      # the data section's own default
    net = train_audio.build_model({"arch": "resnet", "resnet": _opts("attentive_statistic", 1, feat_dim=9)["resnet"]}, {"feat_dim": 24})
    assert net.feat_dim == 9                                       # the model's own key wins


def test_shipped_config_builds_the_shipped_module():
    import os
    import yaml
    import train_audio
    from conftest import ROOT
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        opts = yaml.safe_load(f)
    r = opts["model"]["resnet"]
    assert r["pooling"] == "average" and r["fc_layers"] == 1
    net = train_audio.build_model(dict(opts["model"], arch="resnet"), opts["data"])
    assert net.min_frames() == 1 and tuple(net.fc.weight.shape) == (r["embedding_dim"], r["hidden_dim"][-1])
    assert not any(k.startswith(("fc1", "fc2", "pooling")) for k in net.state_dict())


def test_ops_refuse_cpu_tensors():
    from deeplip_amd import ops
    from deeplip_amd._lib import DeepLipHipError
    lens = torch.ones(2, dtype=torch.int32)
    x = torch.zeros(2, 3, 5, 4)
    with pytest.raises(DeepLipHipError):
        ops.statpool_nhwc(x)
    with pytest.raises(DeepLipHipError):
        ops.statpool_nhwc(x, lens, 1)
    with pytest.raises(DeepLipHipError):
        ops.swap_axes_nhwc(x)
    with pytest.raises(DeepLipHipError):
        ops.time_valid_lengths(lens, 1, 5)
    with pytest.raises(DeepLipHipError):       # (the attentive head's tail: one head of the multi-head entry points, no offsets array)
        ops.mh_attn_scores(torch.zeros(2, 5, 3), torch.zeros(3), torch.zeros(1), None)
    with pytest.raises(DeepLipHipError):
        ops.mh_attn_stat_pool(torch.zeros(2, 5, 12), torch.zeros(2, 1, 5), 1e-5)


def test_library_exports_the_entry_points():
    import test_abi_cpu as abi
    from deeplip_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for s in ("dlip_statpool_nhwc_f32", "dlip_statpool_nhwc_bwd_f32", "dlip_swap_axes_nhwc_f32", "dlip_time_valid_lengths_i32",
              "dlip_mh_attn_scores_f32", "dlip_mh_attn_stat_pool_f32", "dlip_mh_attn_stat_pool_bwd_f32"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES
    # (ABI 67) the single-head kernels' four entry points are gone: attentive pooling is one head of the dlip_mh_attn_* family
    for s in [f"dlip_attentive_stat_{p}_f32" for p in ("pool", "pool_bwd", "pool_eps", "pool_eps_bwd")]:
        assert not hasattr(lib, s) and s not in _lib.SIGNATURES and s not in abi.header_symbols(), s
    assert lib.dlip_abi_version() == _lib.ABI_VERSION == 67
