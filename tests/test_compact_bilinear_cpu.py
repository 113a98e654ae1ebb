"""CompactBilinearPooling without a GPU (-m "not gpu"): upstream's constructor, attribute names and state-dict keys, the count
sketches and their seeding, the shim import the reference's train_fusion.py:31-32 relies on, the sketches the pack refuses, the new
entry points in header / binding / library, the shipped config, and the test files' own fp64 oracle (FFT form against the direct
circular convolution)."""
import inspect
import os

import pytest
import torch

from conftest import ROOT


def fft_form64(x1, x2, S1, S2, sum_pool=True):
    """The layer as upstream writes it, in fp64: x [B,C,H,W], S [C,D]."""
    D = S1.shape[1]
    psi1 = x1.double().permute(0, 2, 3, 1) @ S1.double()
    psi2 = x2.double().permute(0, 2, 3, 1) @ S2.double()
    cbp = torch.fft.irfft(torch.fft.rfft(psi1, dim=-1) * torch.fft.rfft(psi2, dim=-1), n=D, dim=-1) * D
    return cbp.sum(dim=[1, 2]) if sum_pool else cbp


def direct_form64(x1, x2, S1, S2, sum_pool=True):
    """out[k] = D sum_{(m + n) mod D = k} psi1[m] psi2[n]: the circular convolution written out, no FFT."""
    D = S1.shape[1]
    psi1 = x1.double().permute(0, 2, 3, 1) @ S1.double()
    psi2 = x2.double().permute(0, 2, 3, 1) @ S2.double()
    k = torch.arange(D)
    rolled = psi2[..., (k[:, None] - k[None, :]) % D]                    # [..., k, m] = psi2[(k - m) mod D]
    cbp = (rolled * psi1[..., None, :]).sum(-1) * D
    return cbp.sum(dim=[1, 2]) if sum_pool else cbp


def test_keys_shapes_and_one_signed_one_per_row():
    from deeplip_amd.fusion import CompactBilinearPooling
    m = CompactBilinearPooling(40, 24, 16)
    assert list(inspect.signature(CompactBilinearPooling.__init__).parameters) == ["self", "in_channels1", "in_channels2", "out_channels",
                                                                                   "sum_pool"]
    assert inspect.signature(CompactBilinearPooling.__init__).parameters["sum_pool"].default is True
    sd = m.state_dict()
    assert list(sd) == ["tensor_sketch1", "tensor_sketch2"]
    assert tuple(sd["tensor_sketch1"].shape) == (40, 16) and tuple(sd["tensor_sketch2"].shape) == (24, 16)
    assert {n for n, _ in m.named_parameters()} == {"tensor_sketch1", "tensor_sketch2"}
    for p in m.parameters():
        assert isinstance(p, torch.nn.Parameter) and not p.requires_grad and p.dtype == torch.float32 and not p.is_cuda
        assert torch.equal((p != 0).sum(1), torch.ones(p.shape[0], dtype=torch.long))
        assert torch.equal(p.abs().sum(1), torch.ones(p.shape[0]))
    assert m.__dict__["_dlip_precision"] == "f32" and m.sum_pool is True
    assert CompactBilinearPooling(4, 4, 8, sum_pool=False).sum_pool is False


def test_manual_seed_reproduces_the_sketches_in_the_documented_order():
    from deeplip_amd.fusion import CompactBilinearPooling
    torch.manual_seed(7)
    a = CompactBilinearPooling(12, 9, 30)
    torch.manual_seed(7)
    b = CompactBilinearPooling(12, 9, 30)
    assert torch.equal(a.tensor_sketch1, b.tensor_sketch1) and torch.equal(a.tensor_sketch2, b.tensor_sketch2)
    torch.manual_seed(7)                                                  # h1, s1, h2, s2 from the global generator
    want = []
    for c in (12, 9):
        h = torch.randint(30, (c,))
        s = 2 * torch.randint(2, (c,), dtype=torch.float32) - 1
        S = torch.zeros(c, 30)
        S[torch.arange(c), h] = s
        want.append(S)
    assert torch.equal(a.tensor_sketch1, want[0]) and torch.equal(a.tensor_sketch2, want[1])
    torch.manual_seed(8)
    c = CompactBilinearPooling(12, 9, 30)
    assert not torch.equal(a.tensor_sketch1, c.tensor_sketch1)


def test_strict_loads_work_for_the_layer_and_the_head():
    from deeplip_amd.fusion import BNCompactBilinear, CompactBilinearPooling
    a, b = CompactBilinearPooling(12, 9, 30), CompactBilinearPooling(12, 9, 30)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys and torch.equal(a.tensor_sketch1, b.tensor_sketch1)
    assert not b.tensor_sketch1.requires_grad
    h = BNCompactBilinear(16, 8, 12)
    assert set(h.state_dict()) == {"cbp.tensor_sketch1", "cbp.tensor_sketch2", "bn1.weight", "bn1.bias", "bn1.running_mean",
                                   "bn1.running_var", "bn1.num_batches_tracked"}
    assert {n for n, p in h.named_parameters() if p.requires_grad} == {"bn1.weight", "bn1.bias"}
    h2 = BNCompactBilinear(16, 8, 12)
    h2.load_state_dict(h.state_dict(), strict=True)
    assert torch.equal(h2.cbp.tensor_sketch2, h.cbp.tensor_sketch2)
    assert list(inspect.signature(BNCompactBilinear.__init__).parameters) == ["self", "d1", "d2", "o"]


def test_shim_exports_the_class_the_reference_trainer_imports():
    from deeplip_amd import fusion
    from models.fusion_models.compact_bilinear_pooling import CompactBilinearPooling
    assert CompactBilinearPooling is fusion.CompactBilinearPooling
    m = CompactBilinearPooling(16, 16, 512)                               # the reference's call shape: (D, D, 512)
    assert m.out_channels == 512


def test_pack_reads_h_s_and_bin_sorted_lists_out_of_the_dense_sketch():
    from deeplip_amd import ops
    S = torch.zeros(6, 4)
    h = torch.tensor([2, 0, 2, 3, 0, 2])
    s = torch.tensor([1., -1., -1., 1., 1., 1.])
    S[torch.arange(6), h] = s
    p = ops.compact_bilinear_pack(S)
    assert p["C"] == 6 and p["D"] == 4
    assert p["h"].tolist() == h.tolist() and p["s"].tolist() == s.tolist()
    assert p["rowptr"].tolist() == [0, 2, 2, 5, 6]                        # bin 1 is empty
    assert p["idx"].tolist() == [1, 4, 0, 2, 5, 3]                        # ascending channel inside a bin
    assert p["sgn"].tolist() == [-1., 1., 1., -1., 1., 1.]
    assert all(p[k].dtype == torch.int32 for k in ("h", "rowptr", "idx")) and p["sgn"].dtype == torch.float32


@pytest.mark.parametrize("what", ["two nonzeros", "a 0.5", "an empty row"])
def test_a_sketch_that_is_not_one_signed_one_per_row_is_refused_with_the_row_named(what):
    from deeplip_amd import ops
    from deeplip_amd.fusion import CompactBilinearPooling
    m = CompactBilinearPooling(8, 8, 16)
    S = m.tensor_sketch2.detach().clone()
    col = int(S[5].abs().argmax())
    if what == "two nonzeros":
        S[5, (col + 1) % 16] = 1.0
    elif what == "a 0.5":
        S[5, col] = 0.5
    else:
        S[5, col] = 0.0
    m.load_state_dict({"tensor_sketch1": m.tensor_sketch1.detach(), "tensor_sketch2": S}, strict=True)      # a broken checkpoint loads ...
    with pytest.raises(ValueError, match=r"tensor_sketch2: row 5\b"):
        m._pack(torch.device("cpu"))                                                                        # ... and is refused at pack time
    with pytest.raises(ValueError, match=r"row 5\b"):
        ops.compact_bilinear_pack(S)
    ops.compact_bilinear_pack(m.tensor_sketch1)


def test_refused_constructor_arguments_raise_value_error():
    from deeplip_amd.fusion import BNCompactBilinear, CompactBilinearPooling
    for bad in ((0, 8, 4), (8, 0, 4), (8, 8, 0), (8, 8, 4097)):
        with pytest.raises(ValueError):
            CompactBilinearPooling(*bad)
    with pytest.raises(ValueError):
        BNCompactBilinear(8, 8, 5000)
    CompactBilinearPooling(8, 8, 4096)


def test_cpu_tensors_are_refused():
    from deeplip_amd import autograd as ag, ops
    from deeplip_amd._lib import DeepLipHipError
    from deeplip_amd.fusion import BNCompactBilinear, CompactBilinearPooling
    m = CompactBilinearPooling(8, 8, 4)
    x = torch.zeros(4, 8, 3, 3)
    with pytest.raises(DeepLipHipError):
        m(x, x)
    head = BNCompactBilinear(8, 8, 4)
    e = torch.zeros(4, 8)
    for mode in (head.train, head.eval):
        mode()
        with pytest.raises(DeepLipHipError):
            head(e, e)
    p1, p2 = ops.compact_bilinear_pack(m.tensor_sketch1), ops.compact_bilinear_pack(m.tensor_sketch2)
    with pytest.raises(DeepLipHipError):
        ops.compact_bilinear(e, e, p1, p2)
    with pytest.raises(DeepLipHipError):
        ag.compact_bilinear(e, e, p1, p2)


def test_abi_carries_the_compact_bilinear_entry_points():
    import test_abi_cpu as abi
    from deeplip_amd import _lib, build
    names = ["dlip_compact_bilinear_f32", "dlip_compact_bilinear_bwd_f32"]
    assert _lib.ABI_VERSION >= 55 and all(n in _lib.SIGNATURES and n in abi.header_symbols() for n in names)
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_matches_header()
    abi.test_binding_arity_matches_header()
    assert "compact_bilinear_ops.hip" in build.SOURCES
    text = open(os.path.join(ROOT, "include", "deeplip_hip.h")).read()
    assert text.count("train_fusion.py:31-32,83") >= 3                    # the block and each entry point cite the call site


def test_shipped_config_keeps_linear_and_documents_the_block():
    import yaml
    with open(os.path.join(ROOT, "conf", "fusion_config.yaml")) as f:
        model = yaml.safe_load(f)["model"]
    assert model["fusion"] == "linear" and model["bilinear"] == {"out_dim": 512, "rank": 30}
    assert model["compact_bilinear"] == {"out_dim": 512}


def test_frozen_sketches_stay_out_of_the_optimizer():
    """What train_fusion._init_optim hands the optimizer: trainable parameters only, so the sketches get no update, no weight
    decay and no gradient bucket; the start-of-run broadcast walks parameters() and so still carries them."""
    import train_fusion
    from deeplip_amd.fusion import BNCompactBilinear
    src = inspect.getsource(train_fusion.Trainer._init_optim)
    assert "if p.requires_grad" in src
    assert "for p in list(self.model_fusion.parameters()) + list(self.criterion.parameters()):" in src       # the broadcast: unfiltered
    h = BNCompactBilinear(8, 8, 4)
    assert [n for n, p in h.named_parameters() if not p.requires_grad] == ["cbp.tensor_sketch1", "cbp.tensor_sketch2"]


@pytest.mark.parametrize("shape", [(3, 1, 7, 5, 30), (2, 9, 12, 10, 16), (2, 1, 8, 8, 1), (2, 4, 6, 6, 4)])
@pytest.mark.parametrize("sum_pool", [True, False])
def test_the_oracle_agrees_with_itself_fft_form_against_direct_form(shape, sum_pool):
    """Guards the yardstick of tests/test_compact_bilinear_gpu.py: upstream's FFT form and the direct circular convolution, both in
    fp64, agree to rounding (1e-12 relative to the largest element; observed 4e-15)."""
    from deeplip_amd.fusion import CompactBilinearPooling
    B, P, c1, c2, D = shape
    g = torch.Generator().manual_seed(B + P + c1 + D)
    hw = (3, 3) if P == 9 else (2, 2) if P == 4 else (1, 1)
    x1 = torch.randn(B, c1, *hw, generator=g)
    x2 = torch.randn(B, c2, *hw, generator=g)
    m = CompactBilinearPooling(c1, c2, D)
    a = fft_form64(x1, x2, m.tensor_sketch1, m.tensor_sketch2, sum_pool)
    b = direct_form64(x1, x2, m.tensor_sketch1, m.tensor_sketch2, sum_pool)
    assert tuple(a.shape) == ((B, D) if sum_pool else (B,) + hw + (D,)) and a.shape == b.shape
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)
