"""Segment boundaries of the LDS-DMA ring kernel's ping-pong 256 x 128 tile with split-format output (conv_igemm_f16x3_dma.hip, HEAD;
dlip_debug_set(11, 0 | 1 | 2)): route 0 stages the output tile in the ring's LDS and then sets the next segment up, route 1 takes
the epilogue straight from the accumulators, route 2 also issues the next segment's first slices in front of the finished segment's
hand-off / epilogue.

None of the routes moves a range cut or changes the order of a sum, so for one setting of the balanced split every route gives the
bits of route 0.  Every shape is the smallest at which one piece can go wrong (see the cases)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_rel

gpu = pytest.mark.gpu

TILE_256x128 = 5
ROUTES = (0, 1, 2)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from deeplip_amd import ops as _ops
    return _ops


@pytest.fixture
def dbg():
    """dlip_debug_set for the test, every key it touched back at the built-in choice afterwards."""
    from deeplip_amd import _lib
    touched = set()

    def set_(key, value):
        touched.add(key)
        _lib.debug_set(key, value)
    yield set_
    for k in touched:
        _lib.debug_set(k, -1)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _split_value(x):
    """x rounded to what the split activation format holds (hi + lo)."""
    hi = x.half()
    return hi.float() + (x - hi.float()).half().float()


def _split_encode(x):
    """The split activation format: per 32-channel block, 32 hi halves then 32 lo halves."""
    xs = x.reshape(-1, x.shape[-1] // 32, 32)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return torch.stack([hi, lo], dim=2).reshape(-1, x.shape[-1] * 2).view(torch.float32).reshape(x.shape)


def _split_decode(y):
    """... and its inverse, in fp64: hi + lo."""
    h = y.contiguous().view(torch.float16).reshape(-1, y.shape[-1] // 32, 2, 32).double()
    return (h[:, :, 0] + h[:, :, 1]).reshape(y.shape)


def ticket_words():
    """The ticket words of the current stream's split workspace (its first 65 536 int32)."""
    from deeplip_amd import _lib
    buf = _lib._workspaces[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]
    return buf[: 4 << 16].view(torch.int32)


def route_launches():
    """Launches of the scoped instances per route so far (the library's dlip_conv_ring_head_query)."""
    from deeplip_amd import _lib
    out = (C.c_int64 * 4)()
    fn = _lib.lib().dlip_conv_ring_head_query
    fn.argtypes, fn.restype = [C.POINTER(C.c_int64)], C.c_int
    _lib.check(fn(out), "dlip_conv_ring_head_query")
    return [int(v) for v in out[:3]]


def _bits(y):
    return y.contiguous().view(torch.int32)


def _check_routes(dbg, launch, check_fp64):
    """launch() -> the split-format output on the device.  For the split off and forced: routes 1 and 2 give route 0's bits and each
    launch takes the route asked for; every output meets the fp64 bar; three launches in a row give the same bits and leave the
    ticket words at zero."""
    from deeplip_amd import _lib
    dbg(_lib.DBG_DMA_TILE, TILE_256x128)
    dbg(_lib.DBG_WIN, 0)            # (stride-1 3x3 launches of K <= 128 would otherwise go to the window kernel)

    def run(route):
        dbg(_lib.DBG_RING_HEAD, route)
        n0 = route_launches()
        y = launch()
        torch.cuda.synchronize()
        n1 = route_launches()
        assert [b - a for a, b in zip(n0, n1)] == [1 if r == route else 0 for r in ROUTES], f"route {route}: the launch took another"
        return y

    for split in (0, 2):
        dbg(_lib.DBG_STREAMK, split)
        ys = [run(r) for r in ROUTES]
        for r in (1, 2):
            assert torch.equal(_bits(ys[0]), _bits(ys[r])), f"split {split}: route {r} differs from route 0"
        for r in ROUTES:
            check_fp64(ys[r], f"split {split} route {r}")
        if split == 2:
            for r in (1, 2):
                again = [run(r) for _ in range(2)]
                assert torch.equal(_bits(ys[r]), _bits(again[0])) and torch.equal(_bits(ys[r]), _bits(again[1])), f"route {r}: bits differ between launches"
            assert int(ticket_words().abs().max()) == 0


def _conv_inputs(N, H, W, Cin, K, stride, with_res):
    x = _split_value(rnd(N, H, W, Cin, seed=1) * 2.0)
    w = rnd(K, 3, 3, Cin, seed=2, scale=1.0 / np.sqrt(9 * Cin))
    b = rnd(K, seed=3, scale=0.1)
    slope = torch.rand(K, generator=torch.Generator().manual_seed(5)) * 0.3
    ps = 0.5 + torch.rand(K, generator=torch.Generator().manual_seed(6))
    pt = rnd(K, seed=7, scale=0.1)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    res = _split_value(rnd(N, Ho, Wo, K, seed=4)) if with_res else None
    return x, w, b, slope, ps, pt, res


def _conv_ref(x, w, b, slope, ps, pt, res, stride):
    """fp64 Conv2d + residual + per-channel leaky slope + post affine, NHWC."""
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    if res is not None:
        ref = ref + res.double()
    return torch.where(ref >= 0, ref, ref * slope.double()) * ps.double() + pt.double()


def _conv_launcher(ops, x, w, b, slope, ps, pt, res, stride, alias=False):
    from deeplip_amd import packing
    ws, sc = packing.split_weights(w.double())
    kw = dict(stride=(stride, stride), pad=(1, 1), slope=slope.cuda(), post_scale=ps.cuda(), post_shift=pt.cuda(), w_scale=sc.cuda(),
              x_split=True, out_split=True)
    xd, wd, bd = _split_encode(x.cuda()), ws.cuda(), b.cuda()
    rd = _split_encode(res.cuda()) if res is not None else None
    if alias:      # the residual buffer IS the output buffer (a fresh copy per launch)
        def launch():
            buf = rd.clone()
            return ops.conv_nhwc(xd, wd, bd, residual=buf, out=buf, **kw)
        return launch
    return lambda: ops.conv_nhwc(xd, wd, bd, residual=rd, **kw)


# N, H, W, C, K, stride, residual, forced DBG_NINNER (or None), forced DBG_GROUPED (or None)
SMALL = [
    # 9 tiles of 18 slices on 10 workgroups: every workgroup crosses one tile boundary mid-tile (partial -> partial, a hand-off on
    # both sides, the broadcast word away from stage 0); the last tile has rows past M
    (17, 11, 11, 64, 128, 1, True, None, None),
    (17, 11, 11, 64, 128, 1, False, None, None),
    # two column blocks: consecutive segments change column block (second parameter table, b_off), and the paired lanes' tickets
    (40, 6, 6, 64, 256, 1, True, 0, 0),
    (40, 6, 6, 64, 256, 1, True, 1, 0),
    (40, 6, 6, 64, 256, 1, True, 2, 0),
    # border groups: consecutive segments in different groups (nk, sub-filter, out_row)
    (300, 3, 3, 64, 128, 1, True, None, 1),
    (40, 6, 6, 32, 128, 1, True, None, 1),
    (40, 6, 6, 32, 128, 1, False, None, 1),
    # K no multiple of 128: weight rows and output chunks past K
    (70, 3, 3, 64, 96, 1, True, None, None),
    (70, 3, 3, 64, 96, 1, False, None, 1),
]


@gpu
@pytest.mark.parametrize("case", SMALL, ids=lambda c: "x".join("n" if v is None else str(int(v)) for v in c))
def test_routes_give_the_same_bits(ops, dbg, case):
    from deeplip_amd import _lib
    N, H, W, Cin, K, stride, with_res, ninner, grouped = case
    x, w, b, slope, ps, pt, res = _conv_inputs(N, H, W, Cin, K, stride, with_res)
    ref = _conv_ref(x, w, b, slope, ps, pt, res, stride).numpy()
    if ninner is not None:
        dbg(_lib.DBG_NINNER, ninner)
    if grouped is not None:
        dbg(_lib.DBG_GROUPED, grouped)
    launch = _conv_launcher(ops, x, w, b, slope, ps, pt, res, stride)
    _check_routes(dbg, launch, lambda y, what: assert_close_rel(_split_decode(y.cpu()).numpy(), ref, what=what))


@gpu
@pytest.mark.parametrize("mode", ["plain", "residual", "aliased"])
def test_ranges_of_several_tiles(ops, dbg, mode):
    """(2200, 11 x 11, 32 -> 128): 1 040 tiles of 9 slices on one workgroup per CU -- ranges of several tiles (partial, whole, whole
    ..., partial): the main path, a whole-tile epilogue with the next head in flight.  With and without a residual, and with the
    residual buffer as the output buffer.  fp64 on the rows of a seeded sample of 34 images (4 114 rows) and the last image."""
    N, H, W, Cin, K = 2200, 11, 11, 32, 128
    nk, tiles = 9 * (Cin // 32), -(-N * H * W // 256) * (K // 128)
    # the launch arithmetic restated: one eight-wave workgroup per CU, at least 16 slices per workgroup, at most 64 parts per tile
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    iters = tiles * nk
    G = cus if iters >= 16 * cus else max(iters // 16, 1)
    G = min(G, tiles * 64)
    assert tiles == 1040 and iters / G > 2 * nk, "a range must hold more than two tiles"
    x, w, b, slope, ps, pt, res = _conv_inputs(N, H, W, Cin, K, 1, mode != "plain")
    pick = torch.randperm(N - 1, generator=torch.Generator().manual_seed(20))[:34].sort().values
    pick = torch.cat([pick, torch.tensor([N - 1])])
    ref = _conv_ref(x[pick], w, b, slope, ps, pt, res[pick] if res is not None else None, 1).numpy()
    launch = _conv_launcher(ops, x, w, b, slope, ps, pt, res, 1, alias=mode == "aliased")
    pick_d = pick.cuda()
    _check_routes(dbg, launch, lambda y, what: assert_close_rel(_split_decode(y[pick_d].cpu()).numpy(), ref, what=what))


@gpu
@pytest.mark.parametrize("grouped", [0, 1])
def test_second_source(ops, dbg, grouped):
    """DUAL: conv3x3(h) + conv1x1 stride 2 (x) in one reduction (ops.conv2_nhwc), 3 x 3 output from a 6 x 6 second source, grouped
    and not: with the split forced a segment is entered at a k0 inside the second source's slices."""
    from deeplip_amd import _lib, packing
    N, K, C2 = 40, 128, 32
    h = _split_value(rnd(N, 3, 3, 64, seed=52) * 2.0)
    x = _split_value(rnd(N, 6, 6, C2, seed=51) * 2.0)
    w2 = rnd(K, 64, 3, 3, seed=53, scale=1.0 / np.sqrt(9 * 64))
    wd = rnd(K, C2, 1, 1, seed=54, scale=1.0 / np.sqrt(C2))
    b = rnd(K, seed=55, scale=0.1)
    slope = torch.rand(K, generator=torch.Generator().manual_seed(5)) * 0.3
    ref = F.conv2d(h.permute(0, 3, 1, 2).double(), w2.double(), None, padding=1) + \
        F.conv2d(x.permute(0, 3, 1, 2).double(), wd.double(), None, stride=2) + b.double().view(1, K, 1, 1)
    ref = torch.where(ref >= 0, ref, ref * slope.double().view(1, K, 1, 1)).permute(0, 2, 3, 1).numpy()
    rows = torch.cat([w2.double().permute(0, 2, 3, 1).reshape(K, -1), wd.double().reshape(K, C2)], dim=1)
    ws, sc = packing.split_weights(rows)
    hd, xd, wsd, bd, scd, sld = _split_encode(h).cuda(), _split_encode(x).cuda(), ws.cuda(), b.cuda(), sc.cuda(), slope.cuda()
    dbg(_lib.DBG_GROUPED, grouped)
    launch = lambda: ops.conv2_nhwc(hd, xd, wsd, bd, scd, pad=(1, 1), stride2=(2, 2), slope=sld, out_split=True)   # noqa: E731
    _check_routes(dbg, launch, lambda y, what: assert_close_rel(_split_decode(y.cpu()).numpy(), ref, what=what))


def test_key_is_the_enum_next_value():
    from deeplip_amd import _lib
    assert _lib.DBG_RING_HEAD == 11 and _lib.HEADER["DLIP_DBG_COUNT"] == 12
