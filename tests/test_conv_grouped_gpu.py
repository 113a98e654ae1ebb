"""Border groups of the LDS-DMA ring kernel: a padded convolution on the 256 x 128 tile run as its (at most 3 x 3) padding-free
sub-convolutions in ONE launch (conv_igemm_f16x3_dma.hip, ConvGroup; dlip_debug_set(10, 1 | 0) = whenever legal | never).

A slice of zeros adds +-0 to an accumulator that starts at +0, so with the balanced split off a grouped launch gives the ungrouped
launch's values element for element; with the split on the part boundaries move and the bar is the project's own (assert_close_rel
against Conv2d in fp64).  Every shape is the smallest at which one piece of the construction can go wrong (see CASES)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_rel

gpu = pytest.mark.gpu

TILE_256x128 = 5


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
    """CPU statement of the split activation format: per 32-channel block, 32 hi halves then 32 lo halves."""
    xs = x.reshape(-1, x.shape[-1] // 32, 32)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return torch.stack([hi, lo], dim=2).reshape(-1, x.shape[-1] * 2).view(torch.float32).reshape(x.shape)


def _split_decode(y):
    """... and its inverse, in fp64: hi + lo."""
    h = y.contiguous().view(torch.float16).reshape(-1, y.shape[-1] // 32, 2, 32).double()
    return (h[:, :, 0] + h[:, :, 1]).reshape(y.shape)


def grouped_query(N, H, W, Cin, R, S, stride, pad, nk2=0):
    """The group table the launch would build (the library's own conv_groups): dict of its totals."""
    from deeplip_amd import _lib
    geom = (C.c_int32 * 13)(N, H, W, Cin, R, S, stride, stride, pad, pad, 1, 1, nk2)
    out = (C.c_int64 * 8)()
    fn = _lib.lib().dlip_conv_grouped_query
    fn.argtypes, fn.restype = [C.POINTER(C.c_int32), C.POINTER(C.c_int64)], C.c_int
    _lib.check(fn(geom, out), "dlip_conv_grouped_query")
    return dict(zip(("legal", "by_rule", "groups", "slices", "tiles", "useful", "total", "launches"), [int(v) for v in out]))


def grouped_launches():
    return grouped_query(1, 3, 3, 32, 3, 3, 1, 1)["launches"]


def ticket_words():
    """The ticket words of the current stream's split workspace (its first 65 536 int32)."""
    from deeplip_amd import _lib
    buf = _lib._workspaces[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]
    return buf[: 4 << 16].view(torch.int32)


# ---- the rule on the CPU: totals of the group table ----
def _python_groups(H, W, R, S, stride, pad):
    """The same rule recomputed: per output index the valid taps, classes = runs of equal ranges, groups = class pairs."""
    def classes(In, T):
        Out = (In + 2 * pad - (T - 1) - 1) // stride + 1
        runs = []
        for o in range(Out):
            taps = tuple(t for t in range(T) if 0 <= o * stride - pad + t < In)
            if runs and runs[-1][0] == taps:
                runs[-1][1] += 1
            else:
                runs.append([taps, 1])
        return runs, Out
    rows, Ho = classes(H, R)
    cols, Wo = classes(W, S)
    return [(len(tr) * len(tc), nr * nc) for tr, nr in rows for tc, nc in cols], Ho * Wo


@pytest.mark.parametrize("geom,useful,total", [((3, 3, 1), 49, 81), ((6, 6, 1), 256, 324), ((11, 11, 2), 64 * 4, 81 * 4), ((6, 6, 2), 64, 81)],
                         ids=["3x3s1", "6x6s1", "11to6s2", "6to3s2"])
def test_group_table_totals(geom, useful, total):
    """Sum over the groups of taps x positions: 49 (of 81) on a 3x3 map, 256 (of 324) on 6x6, 64/81 of the taps on the stride-2
    11 -> 6 and 6 -> 3 convolutions; slices and tiles of the launch follow from the same table."""
    H, W, stride = geom
    N, Cin = 1856, 64
    q = grouped_query(N, H, W, Cin, 3, 3, stride, 1)
    groups, howo = _python_groups(H, W, 3, 3, stride, 1)
    assert q["legal"] == 1 and q["groups"] == len(groups)
    assert q["useful"] == sum(t * p for t, p in groups) and q["total"] == 9 * howo
    assert q["useful"] * total == useful * q["total"]
    assert q["tiles"] == sum(-(-N * p // 256) for t, p in groups)
    assert q["slices"] == sum(-(-N * p // 256) * t * (Cin // 32) for t, p in groups)


def test_group_table_small_maps_and_limits():
    assert grouped_query(50, 2, 2, 64, 3, 3, 1, 1)["groups"] == 4          # no interior class: empty groups are dropped
    q = grouped_query(50, 1, 1, 64, 3, 3, 1, 1)
    assert (q["groups"], q["useful"], q["total"]) == (1, 1, 9)            # a single one-tap group
    assert grouped_query(50, 6, 6, 64, 3, 3, 1, 0)["legal"] == 0          # no padding: nothing to group
    assert grouped_query(50, 9, 9, 64, 5, 5, 1, 2)["legal"] == 0          # five classes per dimension
    # layer 4 at the bench's batch: 9 groups x 8 row tiles, 64 / 96 / 144 slices
    q = grouped_query(64 * 29, 3, 3, 512, 3, 3, 1, 1)
    assert (q["groups"], q["tiles"], q["slices"]) == (9, 72, 8 * 16 * 49)


def test_built_in_rule_at_the_bench_shapes():
    """The built-in rule at B = 64 clips: layers 3 (6x6 maps, 72 slices) and 4 take the grouped twin, the stride-2 11 -> 6 convolution
    (36 slices) and layer 2.0 do not (measured per layer: the rule's comment)."""
    N = 64 * 29
    want = {(6, 6, 256, 1): 1, (6, 6, 256, 2): 1, (3, 3, 512, 1): 1, (11, 11, 128, 2): 0, (11, 11, 128, 1): 0, (22, 22, 64, 2): 0}
    for (H, W, Cin, stride), by_rule in want.items():
        assert grouped_query(N, H, W, Cin, 3, 3, stride, 1)["by_rule"] == by_rule, (H, W, Cin, stride)


# ---- on the GPU ----
CASES = [  # N, H, W, C, K, stride, residual + split-format output (EPI 1)
    (70, 3, 3, 64, 128, 1, False),      # 9 one-position groups, every group one partial tile (M_g = 70 < 256)
    (70, 3, 3, 64, 128, 1, True),
    (300, 3, 3, 64, 128, 1, False),     # groups of two tiles, the second partial; split ranges cross groups whose nk differ
    (40, 6, 6, 32, 128, 1, False),      # multi-position groups (sub-rectangle decode); one slice per tap
    (40, 6, 6, 32, 128, 1, True),
    (33, 3, 5, 96, 192, 1, False),      # non-square map, partial second column block (weight rows past K)
    (50, 2, 2, 64, 128, 1, False),      # no interior class
    (50, 1, 1, 64, 128, 1, False),      # a single one-tap group
    (37, 6, 6, 64, 128, 2, False),      # stride 2, even size: padding on the low side only
    (37, 5, 5, 64, 128, 2, False),      # stride 2, odd size: both sides
    (37, 11, 11, 64, 128, 2, False),    # 11 -> 6
]


def _conv_case(case):
    N, H, W, Cin, K, stride, epi1 = case
    x = _split_value(rnd(N, H, W, Cin, seed=1) * 2.0)
    w = rnd(K, 3, 3, Cin, seed=2, scale=1.0 / np.sqrt(9 * Cin))
    b = rnd(K, seed=3, scale=0.1)
    slope = torch.rand(K, generator=torch.Generator().manual_seed(5)) * 0.3
    ps = 0.5 + torch.rand(K, generator=torch.Generator().manual_seed(6))
    pt = rnd(K, seed=7, scale=0.1)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    res = _split_value(rnd(N, Ho, Wo, K, seed=4)) if epi1 else None
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    if res is not None:
        ref = ref + res.double()
    ref = torch.where(ref >= 0, ref, ref * slope.double()) * ps.double() + pt.double()
    return x, w, b, slope, ps, pt, res, ref


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_grouped_matches_ungrouped_and_fp64(ops, dbg, case):
    from deeplip_amd import _lib, packing
    N, H, W, Cin, K, stride, epi1 = case
    x, w, b, slope, ps, pt, res, ref = _conv_case(case)
    ws, sc = packing.split_weights(w.double())
    kw = dict(stride=(stride, stride), pad=(1, 1), slope=slope.cuda(), post_scale=ps.cuda(), post_shift=pt.cuda(), w_scale=sc.cuda(),
              x_split=True, out_split=epi1, residual=_split_encode(res).cuda() if epi1 else None)
    xd, wd, bd = _split_encode(x).cuda(), ws.cuda(), b.cuda()
    dbg(_lib.DBG_DMA_TILE, TILE_256x128)
    dbg(_lib.DBG_WIN, 0)            # (stride-1 3x3 launches of K <= 128 would otherwise go to the window kernel)

    def run(grouped, split):
        dbg(_lib.DBG_GROUPED, 1 if grouped else 0)
        dbg(_lib.DBG_STREAMK, split)
        n0 = grouped_launches()
        y = ops.conv_nhwc(xd, wd, bd, **kw)
        torch.cuda.synchronize()
        assert grouped_launches() - n0 == (1 if grouped else 0), "the launch took the other route"
        y = y.cpu()
        return _split_decode(y) if epi1 else y.double()

    plain_u, plain_g = run(False, 0), run(True, 0)
    assert torch.equal(plain_u, plain_g)                                             # (a) same values, split off
    split_u, split_g = run(False, 2), run(True, 2)
    for name, y in (("ungrouped plain", plain_u), ("grouped plain", plain_g), ("ungrouped split", split_u), ("grouped split", split_g)):
        assert_close_rel(y.numpy(), ref.numpy(), what=name)                          # (b) fp64 Conv2d
    again = [run(True, 2) for _ in range(2)]
    assert torch.equal(split_g, again[0]) and torch.equal(split_g, again[1])         # (c) three launches, the same bits
    assert int(ticket_words().abs().max()) == 0                                      # ... and the ticket words back at zero


@gpu
@pytest.mark.parametrize("ninner", [0, 1, 2])
def test_grouped_serves_the_outer_tile_order_only(ops, dbg, ninner):
    """K = 256 (two column blocks).  The twin implements ONE tile order (column block outer); a launch whose order is forced inner
    or paired (dlip_debug_set(5, 1 | 2)) stays on the ungrouped kernel even where grouping is forced."""
    from deeplip_amd import _lib, packing
    case = (40, 6, 6, 64, 256, 1, False)
    x, w, b, slope, ps, pt, res, ref = _conv_case(case)
    ws, sc = packing.split_weights(w.double())
    kw = dict(pad=(1, 1), slope=slope.cuda(), post_scale=ps.cuda(), post_shift=pt.cuda(), w_scale=sc.cuda(), x_split=True)
    xd, wd, bd = _split_encode(x).cuda(), ws.cuda(), b.cuda()
    dbg(_lib.DBG_DMA_TILE, TILE_256x128)
    dbg(_lib.DBG_WIN, 0)            # (stride-1 3x3 launches of K <= 128 would otherwise go to the window kernel)
    dbg(_lib.DBG_NINNER, ninner)
    outs = {}
    for split in (0, 2):
        dbg(_lib.DBG_STREAMK, split)
        for grouped in (0, 1):
            dbg(_lib.DBG_GROUPED, grouped)
            n0 = grouped_launches()
            y = ops.conv_nhwc(xd, wd, bd, **kw)
            torch.cuda.synchronize()
            assert grouped_launches() - n0 == (1 if grouped and ninner == 0 else 0)
            outs[split, grouped] = y.cpu()
            assert_close_rel(y.cpu().double().numpy(), ref.numpy(), what=f"split {split} grouped {grouped}")
    assert torch.equal(outs[0, 0], outs[0, 1])
    if ninner:
        assert torch.equal(outs[2, 0], outs[2, 1])      # the same (ungrouped) launch twice
    assert int(ticket_words().abs().max()) == 0


@gpu
@pytest.mark.parametrize("out_split", [False, True])
def test_grouped_second_source(ops, dbg, out_split):
    """DUAL: conv3x3(h) + conv1x1 stride 2 (x) in one reduction (ops.conv2_nhwc), 3 x 3 output from a 6 x 6 second source: the
    second source's weights sit behind the FULL 9 taps whatever the group's sub-filter, its pixel is the full-grid pixel."""
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
    ref = torch.where(ref >= 0, ref, ref * slope.double().view(1, K, 1, 1)).permute(0, 2, 3, 1)
    rows = torch.cat([w2.double().permute(0, 2, 3, 1).reshape(K, -1), wd.double().reshape(K, C2)], dim=1)
    ws, sc = packing.split_weights(rows)
    hd, xd = _split_encode(h).cuda(), _split_encode(x).cuda()
    dbg(_lib.DBG_DMA_TILE, TILE_256x128)
    dbg(_lib.DBG_WIN, 0)            # (stride-1 3x3 launches of K <= 128 would otherwise go to the window kernel)

    def run(grouped, split):
        dbg(_lib.DBG_GROUPED, grouped)
        dbg(_lib.DBG_STREAMK, split)
        n0 = grouped_launches()
        y = ops.conv2_nhwc(hd, xd, ws.cuda(), b.cuda(), sc.cuda(), pad=(1, 1), stride2=(2, 2), slope=slope.cuda(), out_split=out_split)
        torch.cuda.synchronize()
        assert grouped_launches() - n0 == grouped
        return _split_decode(y.cpu()) if out_split else y.cpu().double()

    plain_u, plain_g = run(0, 0), run(1, 0)
    assert torch.equal(plain_u, plain_g)
    split_u, split_g = run(0, 2), run(1, 2)
    for name, y in (("ungrouped plain", plain_u), ("grouped plain", plain_g), ("ungrouped split", split_u), ("grouped split", split_g)):
        assert_close_rel(y.numpy(), ref.numpy(), what=name)
    assert torch.equal(split_g, run(1, 2)) and torch.equal(split_g, run(1, 2))
    assert int(ticket_words().abs().max()) == 0
