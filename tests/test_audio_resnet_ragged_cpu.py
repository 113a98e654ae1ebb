"""Host-side pieces of the ResNet speech encoder's ragged batches (-m "not gpu"): the length recurrence the kernels' shift trick rests
on, the encoder's minimum length, the op wrappers' CPU refusal and the library's two entry points (ABI 56)."""
import ctypes

import pytest
import torch


def test_length_after_k_stride2_stages_is_one_shift():
    """A stride-2 3x3 convolution with padding 1 maps L frames to (L - 1) // 2 + 1; k of them to ((L - 1) >> k) + 1."""
    for L in range(1, 71):
        cur = L
        for k in range(0, 4):
            assert ((L - 1) >> k) + 1 == cur, (L, k)
            cur = (cur - 1) // 2 + 1
    from deeplip_amd import ops
    for L in range(1, 71):                       # ... and it is the convolution's own output size
        assert ops.conv_out_size(L, 3, 2, 1, 1) == (L - 1) // 2 + 1


def test_frames_consumed_is_zero():
    from models.resnet import SpeakerEmbNet
    net = SpeakerEmbNet({"arch": "resnet", "resnet": {"input_dim": 1, "hidden_dim": [8, 8], "residual_block_layers": [1, 1],
                                                     "fc_layers": 1, "embedding_dim": 8, "pooling": "average"}})
    assert net.frames_consumed() == 0


def test_ops_refuse_cpu_tensors():
    from deeplip_amd import ops
    from deeplip_amd._lib import DeepLipHipError
    lens = torch.ones(2, dtype=torch.int32)
    with pytest.raises(DeepLipHipError):
        ops.time_tail_zero(torch.zeros(2, 3, 5, 4), lens, 0)
    with pytest.raises(DeepLipHipError):
        ops.avgpool_time_ragged(torch.zeros(2, 3, 5, 4), lens, 1)


def test_library_exports_the_ragged_entry_points():
    from deeplip_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    for s in ("dlip_time_tail_zero_f32", "dlip_avgpool_time_ragged_f32"):
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES
    assert lib.dlip_abi_version() == _lib.ABI_VERSION >= 56
