"""ASoftmax without a GPU (-m "not gpu"): signature, refused margins, parameters and state dict, the lambda schedule, the refusal of
CPU tensors, the new entry points in header / binding / library and train_audio's option parsing."""
import inspect

import pytest
import torch


def test_signature_and_refused_margins():
    from models.audio_models.loss import ASoftmax
    sig = inspect.signature(ASoftmax.__init__).parameters
    assert list(sig) == ["self", "embedding_size", "num_classes", "m", "lambda_min", "lambda_base", "gamma", "power"]
    assert [sig[k].default for k in list(sig)[3:]] == [4, 5.0, 1000.0, 0.12, 1.0]
    for m in (1, 2, 3, 4):
        crit = ASoftmax(16, 5, m=m)
        assert crit.margin == m and tuple(crit.weights.shape) == (5, 16)
    for m in (0, 5, -1, 2.5, True):
        with pytest.raises(ValueError):
            ASoftmax(16, 5, m=m)
    for name in ("forward", "predict", "anneal", "set_lambda"):
        assert callable(getattr(ASoftmax, name))


def test_parameters_and_state_dict_are_lmcl_shaped():
    from models.audio_models.loss import ASoftmax, LMCL
    crit = ASoftmax(16, 5)
    assert [k for k, _ in crit.named_parameters()] == ["weights"]
    assert list(crit.state_dict()) == ["weights"] == list(LMCL(16, 5, 30, 0.2).state_dict())
    assert [k for k, _ in crit.named_buffers()] == ["lam"] and crit.lam.dtype == torch.float32 and tuple(crit.lam.shape) == (1,)
    crit.load_state_dict(LMCL(16, 5, 30, 0.2).state_dict())           # compatible in shape


def test_lambda_schedule():
    from models.audio_models.loss import ASoftmax
    crit = ASoftmax(16, 5)
    assert crit.schedule(0) == 1000.0 and float(crit.lam) == 1000.0
    assert crit.schedule(100) == pytest.approx(1000.0 / 13.0, rel=1e-12)
    assert crit.schedule(10 ** 6) == 5.0                              # 1000 / 120001 is below lambda_min
    assert crit.anneal(100) == crit.schedule(100) and float(crit.lam) == pytest.approx(1000.0 / 13.0, rel=1e-6) and crit.it == 0
    assert crit.anneal(10 ** 6) == 5.0 and float(crit.lam) == 5.0
    assert crit.anneal(0) == 1000.0 and float(crit.lam) == 1000.0
    # it=None advances the criterion's own counter and uses the new count
    for step in (1, 2, 3):
        assert crit.anneal() == crit.schedule(step) and crit.it == step
    assert float(crit.lam) == pytest.approx(1000.0 / 1.36, rel=1e-6)
    crit2 = ASoftmax(16, 5, lambda_min=3.0, lambda_base=10.0, gamma=1.0, power=2.0)
    assert crit2.schedule(1) == 3.0 and crit2.schedule(0) == 10.0 and crit2.schedule(0.5) == pytest.approx(10.0 / 2.25)
    assert crit.set_lambda(0.0) == 0.0 and float(crit.lam) == 0.0


def test_criterion_refuses_cpu_tensors():
    from deeplip_amd._lib import DeepLipHipError
    from models.audio_models.loss import ASoftmax
    crit = ASoftmax(16, 5)
    x, lab = torch.zeros(8, 16), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(DeepLipHipError):
        crit(x, lab)
    with pytest.raises(DeepLipHipError):
        with torch.no_grad():
            crit(x, lab)
    with pytest.raises(DeepLipHipError):
        crit.predict(x, lab)


def test_abi_carries_the_asoftmax_entry_points():
    import test_abi_cpu as abi
    from deeplip_amd import _lib, build
    names = ["dlip_asoftmax_logits_f32", "dlip_row_norm_f32", "dlip_row_norm_bwd_f32"]
    assert _lib.ABI_VERSION >= 66 and all(n in _lib.SIGNATURES and n in abi.header_symbols() for n in names)
    abi.test_library_exports_every_declared_symbol()
    abi.test_binding_matches_header()
    abi.test_binding_arity_matches_header()
    assert "asoftmax_ops.hip" in build.SOURCES


def test_train_audio_builds_the_criterion_the_config_names():
    import train_audio
    from models.audio_models.loss import ASoftmax
    for kind in ("ASoftmax", "A-Softmax"):
        crit = train_audio.build_criterion({"loss": kind}, 64, 5)
        assert isinstance(crit, ASoftmax) and (crit.m, crit.lambda_min, crit.lambda_base, crit.gamma, crit.power) == (4, 5.0, 1000.0, 0.12, 1.0)
        crit = train_audio.build_criterion({"loss": kind, "asoftmax": {"m": 2, "lambda_min": 1.0, "power": 2.0}}, 64, 5)
        assert (crit.m, crit.margin, crit.lambda_min, crit.lambda_base, crit.gamma, crit.power) == (2, 2, 1.0, 1000.0, 0.12, 2.0)
        assert tuple(crit.weights.shape) == (5, 64)
        with pytest.raises(ValueError):
            train_audio.build_criterion({"loss": kind, "asoftmax": {"lambda": 3.0}}, 64, 5)
        with pytest.raises(ValueError):
            train_audio.build_criterion({"loss": kind, "asoftmax": {"m": 5}}, 64, 5)
