"""_lib.call on the device: its implicit stream is the CURRENT one -- the stream a recording captures."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_a_call_without_a_stream_goes_to_the_capturing_stream():
    """The launch is recorded, not executed: y holds NaN until the replay, and the replay alone writes PReLU(x) into it.  A launch
    that went to any stream but the capturing one would have run (or failed) at record time and left the NaNs after the replay."""
    from deeplip_amd._lib import call
    g0 = torch.Generator().manual_seed(5)
    x = torch.randn(3, 8, generator=g0).cuda()
    slope = torch.rand(8, generator=g0).cuda()
    y = torch.empty_like(x)
    call("dlip_prelu_rows_fwd_f32", x, slope, y, 3, 8)      # eager once: the process's first launch registers its status block
    want = torch.where(x >= 0, x, x * slope)
    assert torch.equal(y, want) and bool((x < 0).any()) and bool((x >= 0).any())
    y.fill_(float("nan"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call("dlip_prelu_rows_fwd_f32", x, slope, y, 3, 8)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)
