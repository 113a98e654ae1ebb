"""``arch: ftdnn`` without a GPU: the encoder ``build_speech_encoder`` returns, its state-dict schema, which layers are
factorized, what the constructors refuse, the frames it consumes, the new entry points in header / binding / library, and the fp64
reference of the semi-orthogonal step itself (tests/ftdnn_ref.py): it converges, from inputs that take each of its three nu branches."""
import ctypes

import numpy as np
import pytest
import torch

import ftdnn_ref as ref

CONTEXTS = [[-2, -1, 0, 1, 2], [-2, 0, 2], [-3, 0, 3], [0], [0]]


def cfg(arch="ftdnn", hidden=(32, 32, 32, 32, 64), contexts=CONTEXTS, feat=24, emb=16, **extra):
    sec = {"input_dim": feat, "hidden_dim": list(hidden), "context": [list(c) for c in contexts], "tdnn_layers": len(contexts), "fc_layers": 3,
           "embedding_dim": emb, "pooling": "statistic", "attention_hidden_size": 8, "bn_first": True}
    sec.update(extra)
    return {"arch": arch, arch: sec}


def build(**kw):
    from deeplip_amd import trainer_common as tc
    return tc.build_speech_encoder(cfg(**kw))


def test_build_speech_encoder_returns_the_ftdnn():
    from deeplip_amd.audio import FTDNN_Block, SpeakerEmbNet, TDNN_Block
    m = build(bottleneck_dim=8)
    assert isinstance(m, SpeakerEmbNet)
    assert [type(b) for b in m.tdnn] == [TDNN_Block, FTDNN_Block, FTDNN_Block, TDNN_Block, TDNN_Block]
    assert m.factorized_layers == (1, 2)


def test_the_upstream_section_builds_as_it_is():
    """conf/audio_config.yaml's own ftdnn section (no attention_hidden_size, no build-owned key): layers 1 and 2, bottleneck 128."""
    import os
    import yaml
    from deeplip_amd import trainer_common as tc
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "conf", "audio_config.yaml")) as f:
        model = yaml.safe_load(f)["model"]
    model["arch"] = "ftdnn"
    m = tc.build_speech_encoder(model)
    assert m.factorized_layers == (1, 2)
    assert tuple(m.tdnn[1].factor.weight.shape) == (128, 512, 3) and m.tdnn[1].bypass_scale == 0.66 and m.tdnn[1].bypass_shift == 2
    assert m.tdnn[2].bypass_shift == 3


def test_state_dict_keys():
    m = build(bottleneck_dim=8)
    keys = set(m.state_dict())
    bn = {"weight", "bias", "running_mean", "running_var", "num_batches_tracked"}
    for i in (1, 2):
        want = {f"tdnn.{i}.factor.weight", f"tdnn.{i}.context_layer.weight", f"tdnn.{i}.context_layer.bias"} | {f"tdnn.{i}.bn.{k}" for k in bn}
        assert {k for k in keys if k.startswith(f"tdnn.{i}.")} == want
        assert tuple(m.state_dict()[f"tdnn.{i}.factor.weight"].shape) == (8, 32, 3)
        assert tuple(m.state_dict()[f"tdnn.{i}.context_layer.weight"].shape) == (32, 8, 1)
    assert {k for k in keys if k.startswith("tdnn.0.")} == {"tdnn.0.context_layer.weight", "tdnn.0.context_layer.bias"} | {f"tdnn.0.bn.{k}" for k in bn}
    from models.audio_models import tdnn
    from deeplip_amd.audio import FTDNN_Block
    assert tdnn.FTDNN_Block is FTDNN_Block


def test_factorized_layers_default_and_explicit():
    from deeplip_amd.audio import FTDNN_Block, default_factorized_layers
    assert default_factorized_layers(CONTEXTS) == [1, 2]
    assert default_factorized_layers([[0], [-1, 0, 1], [0], [-2, 2]]) == [1, 3]
    m = build(bottleneck_dim=8, factorized_layers=[3, 1])
    assert m.factorized_layers == (1, 3)
    assert [isinstance(b, FTDNN_Block) for b in m.tdnn] == [False, True, False, True, False]
    assert m.tdnn[3].kernel_size == 1 and m.tdnn[3].bypass_shift == 0
    assert build(bottleneck_dim=8, factorized_layers=[]).factorized_layers == ()
    # widths that differ: no bypass
    assert build(bottleneck_dim=8, factorized_layers=[4]).tdnn[4].bypass_scale == 0.0


def test_refusals():
    from deeplip_amd import _lib, ops
    from deeplip_amd.audio import FTDNN_Block, SemiOrthStep
    with pytest.raises(ValueError, match="exceeds input_dim"):
        FTDNN_Block(8, 8, [-1, 0, 1], bottleneck_dim=28)                  # Bn > Cin k = 24
    FTDNN_Block(8, 8, [-1, 0, 1], bottleneck_dim=24)                      # the square edge is allowed
    with pytest.raises(ValueError, match="multiple of 4"):
        FTDNN_Block(32, 32, [-2, 0, 2], bottleneck_dim=6)
    with pytest.raises(ValueError, match="exceeds 128"):
        FTDNN_Block(512, 512, [-2, 0, 2], bottleneck_dim=132)             # what the step's LDS plan carries
    with pytest.raises(ValueError, match="factorized_layers"):
        build(bottleneck_dim=8, factorized_layers=[0, 1])
    with pytest.raises(ValueError, match="factorized_layers"):
        build(bottleneck_dim=8, factorized_layers=[5])
    with pytest.raises(ValueError, match="does not span"):
        FTDNN_Block(32, 32, [1, 2, 3], bottleneck_dim=8)                  # a bypass with 0 outside the context
    assert FTDNN_Block(32, 64, [1, 2, 3], bottleneck_dim=8).bypass_scale == 0.0      # ... which only matters where there is a bypass
    assert FTDNN_Block(32, 32, [1, 2, 3], bottleneck_dim=8, bypass_scale=0.0).bypass_scale == 0.0
    # CPU tensors: no CPU path anywhere
    y, x = torch.zeros(1, 4, 8), torch.zeros(1, 6, 8)
    with pytest.raises(_lib.DeepLipHipError):
        ops.ftdnn_bypass(y, x, 0.66, 2)
    with pytest.raises(_lib.DeepLipHipError):
        ops.ftdnn_bypass_bwd(y, x, 0.66, 2)
    with pytest.raises(_lib.DeepLipHipError):
        ops.semi_orth_table([torch.zeros(8, 24)])
    with pytest.raises(_lib.DeepLipHipError):
        SemiOrthStep(build(bottleneck_dim=8), 4)
    with pytest.raises(ValueError):
        SemiOrthStep(build(bottleneck_dim=8), -1)
    with pytest.raises(ValueError, match="no factorized layer"):
        SemiOrthStep(build(arch="tdnn"), 4)


def test_frames_consumed_equals_the_tdnns():
    from deeplip_amd import trainer_common as tc
    f, t = build(bottleneck_dim=8), build(arch="tdnn")
    assert f.frames_consumed() == t.frames_consumed() == 14
    assert tc.encoder_min_frames(f) == tc.encoder_min_frames(t) == 16
    for b, c in zip(f.tdnn, t.tdnn):
        assert (b.kernel_size, b.dilation, b.padding, b.input_dim, b.output_dim) == (c.kernel_size, c.dilation, c.padding, c.input_dim, c.output_dim)


def test_entry_points_in_header_binding_and_library():
    from deeplip_amd import _lib
    c_f, c_i32, c_i64 = _lib.c_f, _lib.c_i32, _lib.c_i64
    assert _lib.ABI_VERSION == 67                                         # pure additions
    want = {"dlip_semi_orth_step_f32": [c_f, c_i32, c_i32, c_i32, c_f, c_i32, c_f, c_i64, c_f],
            "dlip_ftdnn_bypass_f32": [c_f, c_f, c_f, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_float, c_i32, c_f],
            "dlip_ftdnn_bypass_bwd_f32": [c_f, c_f, c_i32, c_i32, c_i32, c_i32, c_i32, ctypes.c_float, c_f],
            "dlip_semi_orth_workspace_bytes": [c_i32]}
    for name, args in want.items():
        assert _lib.SIGNATURES[name] == args, name
    assert {"dlip_semi_orth_step_f32", "dlip_ftdnn_bypass_f32", "dlip_ftdnn_bypass_bwd_f32"} <= _lib.STREAM_LAST
    assert _lib.PROTOTYPES["dlip_semi_orth_workspace_bytes"][0] is c_i64
    assert _lib.HEADER["DLIP_SEMI_ORTH_MAX_ROWS"] == 128
    lib = _lib.lib()
    assert lib.dlip_abi_version() == 67
    for name in want:
        assert hasattr(lib, name)
    per = (_lib.HEADER["DLIP_SEMI_ORTH_SPLITS"] + 1) * 128 * 128 * 4
    assert lib.dlip_semi_orth_workspace_bytes(2) == 256 + 2 * per
    assert lib.dlip_semi_orth_workspace_bytes(0) < 0 and lib.dlip_semi_orth_workspace_bytes(_lib.HEADER["DLIP_SEMI_ORTH_MAX_MATS"] + 1) < 0
    # argument errors are found on the host, before any launch (stream=None: torch.cuda is not touched)
    for args in ((None, 1, 8, 24, None, 4, None, 0), ):
        with pytest.raises(_lib.DeepLipHipError):
            _lib.call("dlip_semi_orth_step_f32", *args, stream=None)


# ---- the reference step alone ---------------------------------------------------------------------------------------------------
def _converges(M, within=12):
    d = [ref.semi_orth_defect(M)]
    for _ in range(within):
        M = ref.semi_orth_step(M)
        d.append(ref.semi_orth_defect(M))
    return d


def test_reference_step_converges_small():
    M = ref.uniform_matrix(8, 24, seed=1)
    ratio = ref.semi_orth_quantities(M)[4]
    d = _converges(M)
    print(f"\n8 x 24: first ratio {ratio:.4f}, defect {d[0]:.3e} -> {d[-1]:.3e}")
    assert ratio > 1.1                                                   # the nu = 1/32 branch
    assert d[0] > 0.5 and d[-1] < 1e-6


def test_reference_step_converges_shipped_shape():
    M = ref.uniform_matrix(128, 1536, seed=2)
    ratio = ref.semi_orth_quantities(M)[4]
    d = _converges(M)
    print(f"\n128 x 1536: first ratio {ratio:.4f}, defect {d[0]:.3e} -> {d[-1]:.3e}")
    assert 1.02 < ratio <= 1.1                                           # the nu = 1/16 branch
    assert d[-1] < 1e-6


def test_reference_step_branches_and_fixed_point():
    nus = [ref.semi_orth_quantities(M)[5] for M in (ref.uniform_matrix(8, 24, 1), ref.uniform_matrix(128, 1536, 2), ref.converged_matrix(8, 24, 1))]
    assert nus == [0.03125, 0.0625, 0.125]                               # all three branches
    M = ref.converged_matrix(8, 24, 1)
    assert np.abs(ref.semi_orth_step(M) - M).max() < 1e-12               # a semi-orthogonal matrix is a fixed point, whatever its scale
    assert np.abs(ref.semi_orth_step(3.0 * M) - 3.0 * M).max() < 1e-12
    assert [ref.semi_orth_due(n, 4) for n in range(1, 10)] == [False, False, False, True, False, False, False, True, False]
    assert not any(ref.semi_orth_due(n, 0) for n in range(1, 10))


def test_a_bad_schedule_is_refused():
    from deeplip_amd.audio import SemiOrthStep
    for every in (True, 2.0, "4"):
        with pytest.raises(ValueError, match="semi_orth_every"):
            SemiOrthStep(build(bottleneck_dim=8), every)
