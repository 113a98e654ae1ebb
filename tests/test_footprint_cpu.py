"""The footprint checker of tests/footprint.py checks: on CPU tensors, no GPU.  tests/test_conv_footprint_gpu.py rests on it."""
import struct

import numpy as np
import pytest
import torch

import footprint as fp
from footprint import Fenced, FenceArena, FootprintError, POISON, ZEROS


def test_poison_is_nan_in_all_three_readings():
    raw = struct.pack("<q", POISON)
    assert np.isnan(np.frombuffer(raw, dtype=np.float64)).all()
    assert np.isnan(np.frombuffer(raw, dtype=np.float32)).all() and np.frombuffer(raw, dtype=np.float32).size == 2
    assert np.isnan(np.frombuffer(raw, dtype=np.float16)).all() and np.frombuffer(raw, dtype=np.float16).size == 4
    f = Fenced(64, fill=POISON)
    assert bool(torch.isnan(f.buf.view(torch.float64)).all()) and bool(torch.isnan(f.buf.view(torch.float32)).all())
    assert bool(torch.isnan(f.buf.view(torch.float16)).all())
    assert tuple(np.frombuffer(raw, dtype=np.uint32)) == fp.POISON_WORDS
    assert torch.equal(Fenced(16, fill=fp.finite(1.5)).buf.view(torch.float32), torch.full((Fenced(16).total // 4,), 1.5))
    assert torch.equal(Fenced(16, fill=fp.finite(-2.0)).buf.view(torch.float32), torch.full((Fenced(16).total // 4,), -2.0))


@pytest.mark.parametrize("shape,dtype", [((3, 5, 7, 12), torch.float32), ((70, 30), torch.float32), ((5, 200, 2), torch.float64),
                                         ((17,), torch.int32), ((1, 1, 300, 4096), torch.float32), ((3,), torch.uint8)])
def test_payload_views(shape, dtype):
    es = torch.empty((), dtype=dtype).element_size()
    n = int(np.prod(shape)) * es
    f = Fenced(n, fill=POISON, pitch_bytes=shape[-1] * es)
    t = f.view(shape, dtype)
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert (t.data_ptr() - f.buf.data_ptr()) % 256 == 0 and f.fence % 256 == 0
    assert f.fence >= 64 << 10 and f.fence >= 256 * shape[-1] * es          # one 256-row tile of the row pitch, never under 64 KiB
    assert f.buf.data_ptr() + f.fence == t.data_ptr()
    assert t.data_ptr() + n == f.buf.data_ptr() + f.hi and f.total - f.hi >= f.fence
    f.check()


def test_one_flipped_byte_in_a_fence_is_reported_with_its_place():
    f = Fenced(1000, fill=POISON, name="y")
    f.view((250,)).fill_(1.0)
    f.check()
    f.buf[f.lo - 3] ^= 1                       # leading fence
    assert f.violations() == (-3, 1, "fence")
    with pytest.raises(FootprintError, match=r"first at byte -3 relative to the payload, 1 bytes differ"):
        f.check()
    f.buf[f.lo - 3] ^= 1
    f.check()
    f.buf[f.hi] ^= 0x80                        # the very first byte behind the payload
    f.buf[f.total - 1] ^= 0x80                 # ... and the very last of the allocation
    assert f.violations() == (1000, 2, "fence")
    for fill in (ZEROS, fp.finite(0.25)):
        g = Fenced(40, fill=fill)
        g.check()
        g.buf[g.hi + 5] = 77
        assert g.violations() == (45, 1, "fence")


def test_one_flipped_byte_in_a_neighbour_channel():
    t = torch.randn(2, 3, 4, 8)
    for fill in (POISON, ZEROS):
        w = fp.wide(t, 4, 12, fill)
        assert tuple(w.full.shape) == (2, 3, 4, 24) and torch.equal(w.own, t) and w.full.is_contiguous()
        assert w.full.data_ptr() % 256 == w.fenced.buf.data_ptr() % 256
        w.check()
        flat = w.fenced.payload
        flat[5 * 96 + 2] ^= 1                  # a LEFT channel (channel 0, byte 2) of row 5
        v = w.neighbour_violations()
        assert v[:2] == (5 * 96 + 2, 1) and "channel 0 of row 5" in v[2]
        with pytest.raises(FootprintError):
            w.check_neighbours()
        flat[5 * 96 + 2] ^= 1
        w.check()
        flat[23 * 96 + 95] ^= 1                # the last byte of the last RIGHT channel of the last row
        v = w.neighbour_violations()
        assert v[:2] == (23 * 96 + 95, 1) and "channel 23 of row 23" in v[2]
        w.fenced.check()                       # (the fences themselves are intact)
    w = fp.wide(t, 4, 12, POISON)
    assert bool(torch.isnan(w.full[..., :4]).all()) and bool(torch.isnan(w.full[..., 12:]).all())
    one = fp.wide(torch.randn(5, 32), 0, 32)   # one-sided: a pitch, no offset
    assert one.own.data_ptr() == one.full.data_ptr() and one.full.shape[1] == 64
    with pytest.raises(ValueError):
        fp.wide(t, 3, 5)


def test_one_flipped_byte_behind_a_vector():
    for n in (30, 31, 64):                     # the payload's end need not be 8-byte aligned: the fill is phased by the allocation
        v = fp.vector(torch.arange(n, dtype=torch.float32))
        assert torch.equal(v.t, torch.arange(n, dtype=torch.float32))
        behind = v.fenced.buf[v.fenced.hi:v.fenced.hi + 16].view(torch.float32)
        assert bool(torch.isnan(behind).all())             # a read of element n, n + 1, ... gets NaN
        v.check()
        v.fenced.buf[v.fenced.hi] ^= 4
        assert v.fenced.violations() == (4 * n, 1, "fence")
        with pytest.raises(FootprintError):
            v.check()


def test_unwritten_and_written_payloads():
    a = FenceArena(POISON)
    t = a.take((7, 40), "cpu", torch.float32)
    assert a.unwritten(t)
    t[:, :39] = 1.0
    assert a.unwritten(t)                      # one column left
    t[:, 39] = 0.0
    assert not a.unwritten(t)
    d = a.take((5, 3, 2), "cpu", torch.float64)
    assert a.unwritten(d)
    d[:4] = 2.0
    assert a.unwritten(d)
    d[4] = -1.0
    assert not a.unwritten(d)
    s = a.take((2, 64), "cpu", torch.float32)  # split format: fp16 halves
    s.view(torch.float16)[:, :126] = 1.0
    assert a.unwritten(s)
    s.view(torch.float16)[:, 126:] = 1.0
    assert not a.unwritten(s)
    a.check_all()


def test_a_kernel_that_writes_one_element_past_K_fails():
    """A torch stand-in for a kernel with a missing ``k < K`` store mask, in one row of a channel-sliced output."""
    K, left, right = 12, 4, 8
    for fill in (POISON, ZEROS):
        a = FenceArena(fill)
        out = a.wide(torch.zeros(70, K), left, right, name="y")

        def kernel(y_full, rows, cols):
            y_full[:rows, left:left + cols] = 1.0
        kernel(out.full, 70, K)
        a.check_all()
        out.full[33, left + K] = 1.0           # one element past K in row 33
        with pytest.raises(FootprintError, match=r"neighbour channel 16 of row 33"):
            a.check_all("fp32 register kernel, tile 0")
        b = FenceArena(fill)
        y = b.filled((70, K), "cpu", name="y")
        y.fill_(1.0)
        b.check_all()
        torch.as_strided(y, (71, K), (K, 1))[70, 0] = 1.0      # ... and one row past M of an exactly sized output
        # (1.0f is 00 00 80 3F: over zeros its first two bytes change nothing)
        first, n = (70 * K * 4, 4) if fill == POISON else (70 * K * 4 + 2, 2)
        with pytest.raises(FootprintError, match=rf"first at byte {first} relative to the payload, {n} bytes differ"):
            b.check_all()


def test_arena_serves_the_dtypes_ops_allocates():
    a = FenceArena(POISON)
    assert a.keep == [] and a.modules == {}
    for dt in (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8):
        t = a.take((3, 5), torch.device("cpu"), dt)
        assert t.dtype == dt and tuple(t.shape) == (3, 5) and t.is_contiguous() and t.data_ptr() % 256 == a.taken[-1][0].buf.data_ptr() % 256
    assert tuple(a.take((0,), "cpu", torch.float32).shape) == (0,)
    assert int(a.take((4,), "cpu", torch.int64)[0]) == POISON
    assert len(a.taken) == 7
    a.check_all()
    x = a.fenced(torch.randn(3, 4, 8))
    assert x.is_contiguous() and tuple(x.shape) == (3, 4, 8)
    assert a.vector(None) is None
    a.taken[2][0].buf[10] ^= 1
    with pytest.raises(FootprintError, match=r"take#2 .*first at byte -\d+ relative to the payload"):
        a.check_all()


def test_arena_stands_in_for_the_plan_arena(monkeypatch):
    """ops._empty asks ARENA.take(shape, device, dtype): the stand-in answers like deeplip_amd.plan.Arena."""
    from deeplip_amd import ops
    a = FenceArena(ZEROS)
    monkeypatch.setattr(ops, "ARENA", a)
    t = ops._empty([2, 3], "cpu")
    d = ops._empty((4,), "cpu", torch.float64)
    assert t.dtype == torch.float32 and tuple(t.shape) == (2, 3) and d.dtype == torch.float64 and len(a.taken) == 2
    assert float(t.abs().max()) == 0.0
    a.check_all()
