"""BNBilinear without a GPU (-m "not gpu"): construction and state dict on the CPU, LowFER's factors load into it, the shim import
the reference's train_fusion.py:84 relies on, the new entry points in header / binding / library, and the shapes and tensors the
host refuses before any launch."""
import inspect
import os

import pytest
import torch

from conftest import ROOT


def test_constructs_on_the_cpu_with_lowfer_names_and_shapes():
    from deeplip_amd.fusion import BNBilinear
    m = BNBilinear(64, 96, 40)
    assert m.k == 30 and m.o == 40
    sd = m.state_dict()
    assert set(sd) == {"U", "V", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked"}
    assert tuple(sd["U"].shape) == (64, 30 * 40) and tuple(sd["V"].shape) == (96, 30 * 40)
    assert all(tuple(sd[f"bn1.{n}"].shape) == (40,) for n in ("weight", "bias", "running_mean", "running_var"))
    assert all(not t.is_cuda and t.dtype == torch.float32 for t in (sd["U"], sd["V"]))
    for t in (sd["U"], sd["V"]):                                        # uniform(-1, 1), as LowFER draws them
        assert float(t.min()) >= -1.0 and float(t.max()) <= 1.0 and float(t.std()) > 0.5
    assert {n for n, _ in m.named_parameters()} == {"U", "V", "bn1.weight", "bn1.bias"}
    m5 = BNBilinear(8, 8, 3, k=5)
    assert tuple(m5.U.shape) == (8, 15)
    assert list(inspect.signature(BNBilinear.__init__).parameters) == ["self", "d1", "d2", "o", "k"]


def test_lowfer_factors_load_into_it():
    from deeplip_amd.fusion import BNBilinear, LowFER
    low = LowFER(32, 32, 16)
    m = BNBilinear(32, 32, 16)
    sd = {k: v for k, v in low.state_dict().items() if k in ("U", "V")}
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("bn1.") for k in res.missing_keys)
    assert torch.equal(m.U, low.U) and torch.equal(m.V, low.V)


def test_shim_exports_the_class_the_reference_trainer_names():
    from deeplip_amd import fusion
    from models.fusion_models import LBP
    assert LBP.BNBilinear is fusion.BNBilinear and LBP.LowFER is fusion.LowFER
    m = LBP.BNBilinear(16, 16, 8)                                         # the reference's call shape: (D, D, o)
    assert m.k == 30


def test_abi_carries_the_bilinear_entry_points():
    import test_abi_cpu as abi
    from deeplip_amd import _lib, build
    names = ["dlip_bilinear_pool_f32", "dlip_bilinear_pool_bwd_w_f32", "dlip_bilinear_pool_bwd_x_f32", "dlip_bilinear_finish_f32"]
    assert _lib.ABI_VERSION >= 54 and all(n in _lib.SIGNATURES and n in abi.header_symbols() for n in names)
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_matches_header()
    abi.test_binding_arity_matches_header()
    assert "bilinear_ops.hip" in build.SOURCES


def test_refused_shapes_raise_value_error():
    from deeplip_amd.fusion import BNBilinear
    for bad in ((6, 8, 4), (8, 10, 4), (0, 8, 4), (8, 8, 0)):
        with pytest.raises(ValueError):
            BNBilinear(*bad)
    with pytest.raises(ValueError):
        BNBilinear(8, 8, 4, k=0)


def test_cpu_tensors_are_refused():
    from deeplip_amd import autograd as ag, ops
    from deeplip_amd._lib import DeepLipHipError
    from deeplip_amd.fusion import BNBilinear
    m = BNBilinear(8, 8, 4, k=3)
    e = torch.zeros(4, 8)
    for mode in (m.train, m.eval):
        mode()
        with pytest.raises(DeepLipHipError):
            m(e, e)
    with pytest.raises(DeepLipHipError):
        ops.bilinear_pool(e, e, m.U.detach(), m.V.detach(), 3)
    with pytest.raises(DeepLipHipError):
        ag.bilinear_pool(e, e, m.U, m.V, 3)


def test_shipped_config_keeps_linear_and_documents_the_block():
    import yaml
    with open(os.path.join(ROOT, "conf", "fusion_config.yaml")) as f:
        model = yaml.safe_load(f)["model"]
    assert model["fusion"] == "linear" and model["bilinear"] == {"out_dim": 512, "rank": 30}
