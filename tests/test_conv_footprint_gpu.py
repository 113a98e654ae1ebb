"""Do the convolution kernels stay inside their buffers?  (tests/footprint.py; tests/test_footprint_cpu.py proves the checker.)

Every case is ONE launch geometry on ONE forced route, run twice with identical geometry, pointer alignment and route: once with
everything around its tensors POISONED (NaN in every reading), once with it ZEROED.

  W  the launch writes nothing outside its output: every fence of every allocation (the inputs' too) and every neighbour channel of a
     channel-sliced tensor is bit-identical to its fill afterwards, and no poison is left in the output's own extent;
  R  the result does not depend on memory the launch does not own: the poisoned run's output is bit-identical to the zeroed run's
     (the kernels are held to run-to-run bit identity, the balanced split included: no tolerance), the range status words stay clean;
  V  rel_err < 2e-5 (the TOL of tests/test_kernels_gpu.py) against an fp64 torch.nn.functional statement of the same operation.

Whatever the entry point allows is embedded: x as a channel slice with neighbours on both sides, the residual wider than K, the output
as a channel slice with neighbours on both sides, bias / slope / post scale / post shift / w_scale and the packed weights with the fill
directly behind their last element, and everything the ops.* wrapper allocates itself through a FenceArena in ops.ARENA.  Where an
entry point takes no pitch (conv2_nhwc, conv_pool, the stems, the weight gradient) the tensors keep their row fences.

Shapes are the smallest at which the edge exists (ragged M, K below / just above a column tile, C below a slice), not the workload's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err
from footprint import POISON, ZEROS, FenceArena, Fenced, has_poison

pytestmark = pytest.mark.gpu

TOL = 2e-5
CFG = [(128, 128), (128, 64), (64, 64), (64, 128), (96, 128)]                  # the register kernels' tile menu (conv_common.h)
DMA_CFG = [(128, 128), (128, 64), (64, 128), (64, 64), (128, 64), (256, 128)]   # the ring kernel's
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


@pytest.fixture(autouse=True)
def _clean_status():
    from deeplip_amd import _lib
    torch.cuda.synchronize()
    _lib.status_words().zero_()
    yield
    torch.cuda.synchronize()
    _lib.status_words().zero_()


@pytest.fixture(autouse=True)
def _slabs_left_clean():
    """mark_slabs() poisons the split workspace the whole process shares: whatever a test of this file does or fails at, no poison
    is left in it for the tests behind."""
    yield
    from deeplip_amd import _lib
    torch.cuda.synchronize()
    for buf in _lib._workspaces.values():
        buf[4 << 16: (4 << 16) + SLAB_MARK].zero_()


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


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


# ---- the two runs ----
def both_fills(ops, monkeypatch, route, body):
    """body(arena) -> {name: device tensor}, everything it hands to the launch made through ``arena``.  W and R as in the module's
    docstring; returns the poisoned run's outputs on the host."""
    from deeplip_amd import _lib
    outs = {}
    for fill, what in ((POISON, "poisoned"), (ZEROS, "zeroed")):
        arena = FenceArena(fill)
        monkeypatch.setattr(ops, "ARENA", arena)
        try:
            got = body(arena)
            torch.cuda.synchronize()
        finally:
            monkeypatch.setattr(ops, "ARENA", None)
        arena.check_all(f"{route}; {what} surroundings")                                                   # W: fences and neighbours
        words = _lib.status_words().tolist()
        assert not any(words), f"[{route}; {what} surroundings] range status words {words}"                # R: status clean
        for k, t in got.items():
            if fill == POISON:                                                                             # W: the output is all written
                assert not has_poison(t), f"[{route}] {k}: poison left in the output's own extent"
            if t.is_floating_point():
                assert not bool(torch.isnan(t).any()), f"[{route}; {what} surroundings] {k}: NaN in the output"
        outs[fill] = {k: t.detach().cpu().clone() for k, t in got.items()}
    for k, a in outs[POISON].items():                                                                      # R: same bits
        b = outs[ZEROS][k]
        assert a.shape == b.shape, (route, k)
        diff = _bits(a) != _bits(b)
        assert not bool(diff.any()), (f"[{route}] {k}: {int(diff.sum())} elements depend on memory outside the launch's tensors, first at "
                                      f"flat index {int(torch.nonzero(diff.view(-1))[0, 0])} of {tuple(a.shape)}")
    return outs[POISON]


def plan(d, mode):
    from deeplip_amd import _lib
    bm, bn = C.c_int32(), C.c_int32()
    _lib.call("dlip_conv_plan", C.byref(d), mode, C.byref(bm), C.byref(bn))
    return bm.value, bn.value


def kind(d):
    from deeplip_amd import _lib
    return int(_lib.lib().dlip_conv_kernel_kind(C.byref(d)))


def ring_head_launches():
    from deeplip_amd import _lib
    out = (C.c_int64 * 4)()
    fn = _lib.lib().dlip_conv_ring_head_query
    fn.argtypes, fn.restype = [C.POINTER(C.c_int64)], C.c_int
    _lib.check(fn(out), "dlip_conv_ring_head_query")
    return [int(v) for v in out[:3]]


def grouped_launches():
    from deeplip_amd import _lib
    geom = (C.c_int32 * 13)(1, 3, 3, 32, 3, 3, 1, 1, 1, 1, 1, 1, 0)
    out = (C.c_int64 * 8)()
    fn = _lib.lib().dlip_conv_grouped_query
    fn.argtypes, fn.restype = [C.POINTER(C.c_int32), C.POINTER(C.c_int64)], C.c_int
    _lib.check(fn(geom, out), "dlip_conv_grouped_query")
    return int(out[7])


# ---- one convolution: inputs and fp64 reference (made once per geometry), and its embedded launch ----
def _hw(H, stride, pad, dil):
    """N,H,W,C,K,R,S,stride,pad,dil: a 1-D case (H == 1) applies the three to the width only; a pad given as a pair is taken as it is."""
    st, dl = ((1, stride), (1, dil)) if H == 1 else ((stride, stride), (dil, dil))
    pd = tuple(pad) if isinstance(pad, tuple) else ((0, pad) if H == 1 else (pad, pad))
    return st, pd, dl


@functools.lru_cache(maxsize=None)
def conv_data(geom, split_in, use_res, post):
    from deeplip_amd import packing
    N, H, W, Cc, K, R, S, stride, pad, dil = geom
    st, pd, dl = _hw(H, stride, pad, dil)
    x = rnd(N, H, W, Cc, seed=1) * 2.0
    if split_in:
        x = _split_value(x)
    w = rnd(K, R, S, Cc, seed=2, scale=1.0 / np.sqrt(Cc * R * S))
    b = rnd(K, seed=3, scale=0.1)
    slope = torch.rand(K, generator=torch.Generator().manual_seed(5)) * 0.3
    ps = 0.5 + torch.rand(K, generator=torch.Generator().manual_seed(6))
    pt = rnd(K, seed=7, scale=0.1)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), b.double(), stride=st, padding=pd, dilation=dl).permute(0, 2, 3, 1)
    res = None
    if use_res:
        res = rnd(*ref.shape, seed=4)
        if split_in:
            res = _split_value(res)
        ref = ref + res.double()
    ref = torch.where(ref >= 0, ref, ref * slope.double())
    if post:
        ref = ref * ps.double() + pt.double()
    ws, sc = packing.split_weights(w.double())
    return dict(x=x, w=w, b=b, slope=slope, ps=ps if post else None, pt=pt if post else None, res=res, ws=ws, sc=sc, ref=ref.contiguous(),
                st=st, pd=pd, dl=dl)


def launch_conv(ops, arena, D, geom, kind_, *, out_split=False, out_lr=None, route=None, stats_chunks=0):
    """kind_: 'f32' (dlip_conv_nhwc_f32) | 'f16x3' (split weights, fp32 activations) | 'split' (split-format x and residual).
    ``route(d)``: the case's route assertions on the REAL descriptor (the picker may look at ldx / ldy / ldr).
    ``stats_chunks`` > 0: the statistics epilogue, whose wrapper takes pitches but no channel offsets: one-sided slices."""
    from deeplip_amd._lib import ConvDesc
    N, H, W, Cc, K, R, S, stride, pad, dil = geom
    split_in = kind_ == "split"
    iu, ou = (32 if split_in else 4), (32 if out_split else 4)
    Ho, Wo = D["ref"].shape[1:3]
    enc = _split_encode if split_in else (lambda t: t)
    xw = arena.wide(enc(D["x"]).cuda(), 0 if stats_chunks else iu, 2 * iu, "x")
    rw = arena.wide(enc(D["res"]).cuda(), 0, iu, "residual") if D["res"] is not None else None        # a pitch, no offset: one-sided
    left, right = out_lr if out_lr is not None else ((0, ou) if stats_chunks else (ou, 2 * ou))
    yw = arena.wide_out((N, Ho, Wo, K), "cuda", left, right, "y")
    vec = lambda t, n: arena.vector(t.cuda() if t is not None else None, n)                          # noqa: E731
    d = ConvDesc(N, H, W, Cc, K, R, S, D["st"][0], D["st"][1], D["pd"][0], D["pd"][1], D["dl"][0], D["dl"][1], Ho, Wo,
                 xw.width, yw.width, rw.width if rw is not None else 0)
    if route is not None:
        route(d)
    kw = dict(stride=D["st"], pad=D["pd"], dil=D["dl"], residual=rw.full if rw is not None else None, slope=vec(D["slope"], "slope"),
              post_scale=vec(D["ps"], "post_scale"), post_shift=vec(D["pt"], "post_shift"), out=yw.full, out_channel_offset=left,
              in_channels=Cc, in_channel_offset=xw.left)
    out = {}
    if kind_ == "f32":
        ops.conv_nhwc(xw.full, vec(D["w"], "w"), vec(D["b"], "bias"), **kw)
    else:
        if stats_chunks:
            out["stats"] = kw["stats"] = arena.filled((stats_chunks * K * 2,), "cuda", torch.float64, "stats")
        ops.conv_nhwc(xw.full, vec(D["ws"], "w_split"), vec(D["b"], "bias"), w_scale=vec(D["sc"], "w_scale"), x_split=split_in,
                      out_split=out_split, **kw)
    y = yw.own.contiguous()
    if out_split:
        out["y.split"] = y
        y = ops.split_unpack(y)
    out["y"] = y
    return out


def assert_v(got, D, route, key="y"):
    err = rel_err(got[key].double().numpy(), D["ref"].numpy())
    assert err < TOL, f"[{route}] rel_err {err:.3e} against fp64"


# ---- a. the fp32 register kernel, b. the split-weight register kernel: every tile forced ----
REG_SHAPES = [
    (2, 5, 7, 8, 12, 3, 3, 1, 1, 1),        # M = 70 ragged in every tile, K = 12 below every column tile, C = 8 < 32
    (1, 1, 37, 36, 200, 1, 5, 1, 8, 2),     # K = 128 + 72, C = 32 + 4, dilation with full padding
    (3, 6, 6, 64, 132, 3, 3, 2, 1, 1),      # stride 2, K = 128 + 4: a 4-wide column tail
]
_ids = lambda g: "x".join(str(v) for v in g)     # noqa: E731


@pytest.mark.parametrize("tile", range(5))
@pytest.mark.parametrize("geom", REG_SHAPES, ids=_ids)
def test_f32_register_kernel(ops, dbg, monkeypatch, geom, tile):
    """dlip_conv_nhwc_f32 with residual, slope and post affine; x, residual and y as channel slices: W, R, V."""
    from deeplip_amd import _lib
    dbg(_lib.DBG_CONV_TILE, tile)
    route = f"fp32 register kernel, tile {tile} = {CFG[tile]}"
    D = conv_data(geom, False, True, True)

    def chk(d):
        assert plan(d, 0) == CFG[tile], route
    got = both_fills(ops, monkeypatch, route, lambda a: launch_conv(ops, a, D, geom, "f32", route=chk))
    assert_v(got, D, route)


@pytest.mark.parametrize("tile", range(5))
@pytest.mark.parametrize("geom", REG_SHAPES, ids=_ids)
def test_split_weight_register_kernel(ops, dbg, monkeypatch, geom, tile):
    """dlip_conv_nhwc_f16x3 on fp32 activations (the register-staged kernel); channel slices everywhere: W, R, V."""
    from deeplip_amd import _lib
    dbg(_lib.DBG_CONV_TILE, tile)
    route = f"split-weight register kernel, tile {tile} = {CFG[tile]}"
    D = conv_data(geom, False, True, True)

    def chk(d):
        assert plan(d, 1) == CFG[tile], route
    got = both_fills(ops, monkeypatch, route, lambda a: launch_conv(ops, a, D, geom, "f16x3", route=chk))
    assert_v(got, D, route)


@pytest.mark.parametrize("tile", range(5))
def test_split_input_odd_output_width_falls_back_inside_its_slice(ops, dbg, monkeypatch, tile):
    """Split-format input with K % 4 != 0 (the ring kernel's 16-byte epilogue cannot write it): the register-staged kernel, into
    channels [16, 46) of a 64-channel output.  (The shape of test_kernels_gpu.py::test_conv_split_input_odd_output_width.)"""
    from deeplip_amd import _lib
    geom = (2, 1, 50, 64, 30, 1, 3, 1, (0, 1), 1)
    dbg(_lib.DBG_CONV_TILE, tile)
    route = f"split-weight register kernel from split input (K % 4 != 0), tile {tile} = {CFG[tile]}"
    D = conv_data(geom, True, False, True)

    def chk(d):
        assert d.K % 4 != 0 and d.ldy == 64 and plan(d, 1) == CFG[tile], route      # (K % 4: dlip_conv_nhwc_f16x3's dma_ok is false)
    got = both_fills(ops, monkeypatch, route, lambda a: launch_conv(ops, a, D, geom, "split", out_lr=(16, 18), route=chk))
    assert_v(got, D, route)


# ---- c. the ring kernel ----
# Why these two are the smallest shapes at which the FORCED balanced split cuts a tile on all six tiles of the menu (slabs_used() below
# asserts that it does).  The launch gives a workgroup at least 16 slices and cuts nothing when that leaves as many workgroups as tiles:
# (3, 5, 5, 64, 96, 3x3) is 1..4 tiles of 18 slices, (1, 1, 41, 96, 160, 1x3 dilation 2) is 2..3 tiles of 9 -- never cut.  So
#   * the first has M = 75 and K = 64 + 32 with C = 128 (36 slices: one tile is cut in two, four tiles go to nine workgroups);
#   * the second has three channel slices, dilation 2 and K = 128 + 32 with M = 257 and five taps (W = 265): at least four
#     tiles on every tile of the menu, one row past the 256-row tile, and 15 slices per tile, so that ranges of 16 or more slices cut
#     tiles (with 9 slices and an even number of tiles -- two column blocks -- every range is two whole tiles).
RING_SHAPES = [
    ((3, 5, 5, 128, 96, 3, 3, 1, 1, 1), True),      # M = 75, K = 64 + 32, residual
    ((1, 1, 265, 96, 160, 1, 5, 1, 0, 2), False),   # three channel slices, K = 128 + 32, M = 256 + 1
]


def _ring_off_others(dbg):
    from deeplip_amd import _lib
    dbg(_lib.DBG_WIN, 0)
    dbg(_lib.DBG_ROWS, 0)


SLAB_MARK = 32 << 20      # bytes of the slabs the checks below look at: more than any launch of this file uses


def _workspace():
    """The current stream's split workspace: (ticket words, the first SLAB_MARK bytes of its slabs as 8-byte words)."""
    from deeplip_amd import _lib
    _lib.ensure_conv_workspace()
    buf = _lib._workspaces[(torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)]
    return buf[: 4 << 16].view(torch.int32), buf[4 << 16: (4 << 16) + SLAB_MARK].view(torch.int64)


def mark_slabs():
    """The slabs carry nothing from one launch to the next: poison them, and slabs_used() says whether a launch really cut a tile."""
    _workspace()[1].fill_(POISON)


def slabs_written(slab_bytes, n):
    """Which of the first ``n`` slabs of ``slab_bytes`` hold no poison any more; the marked region is zeroed again (the workspace is
    shared by every later test of the process)."""
    s = _workspace()[1]
    w = s[: n * slab_bytes // 8].view(n, slab_bytes // 8)
    out = [not bool(v) for v in (w == POISON).any(dim=1).tolist()]
    s.zero_()
    return out


def slabs_used():
    """Whether the launch since mark_slabs() wrote any slab; zeroes the marked region again."""
    s = _workspace()[1]
    used = not bool((s == POISON).all())
    s.zero_()
    return used


@pytest.mark.parametrize("tile", range(6))
@pytest.mark.parametrize("geom,use_res", RING_SHAPES, ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_ring_kernel(ops, dbg, monkeypatch, geom, use_res, tile):
    """conv_igemm_f16x3_dma_kernel, every tile of its menu, fp32 and split output, the balanced split off and forced; on the
    256 x 128 tile with split output also the three segment-boundary routes.  Channel slices everywhere: W, R, V."""
    from deeplip_amd import _lib
    _ring_off_others(dbg)
    dbg(_lib.DBG_DMA_TILE, tile)
    D = conv_data(geom, True, use_res, True)
    for split in (0, 2):
        dbg(_lib.DBG_STREAMK, split)
        for out_split in (False, True):
            for head in ((0, 1, 2) if tile == TILE_256x128 and out_split else (None,)):
                dbg(_lib.DBG_RING_HEAD, head if head is not None else -1)
                route = (f"ring kernel, tile {tile} = {DMA_CFG[tile]}, {'split' if out_split else 'fp32'} output, balanced split "
                         f"{'forced' if split else 'off'}" + (f", head route {head}" if head is not None else ""))

                def chk(d):
                    assert kind(d) == 0 and plan(d, 3) == DMA_CFG[tile], route

                def body(a):
                    n0 = ring_head_launches()
                    mark_slabs()
                    out = launch_conv(ops, a, D, geom, "split", out_split=out_split, route=chk)
                    torch.cuda.synchronize()
                    n1 = ring_head_launches()
                    want = [int(h == head) for h in (0, 1, 2)] if head is not None else [0, 0, 0]
                    assert [q - p for p, q in zip(n0, n1)] == want, route
                    assert slabs_used() == (split == 2), f"{route}: the launch " + ("cut no tile" if split else "used the split workspace")
                    assert int(_workspace()[0].abs().max()) == 0, f"{route}: ticket words not back at zero"
                    return out
                got = both_fills(ops, monkeypatch, route, body)
                assert_v(got, D, route)


@pytest.mark.parametrize("ninner", [1, 2])
def test_ring_kernel_column_block_orders(ops, dbg, monkeypatch, ninner):
    """Column block inner and paired (dlip_debug_set(5, 1 | 2)) with the balanced split forced: two column blocks, residual, split
    output.  The order a launch took cannot be queried; the launch falls back from paired to inner unless its workgroups divide by
    the column blocks, so the test restates that arithmetic.  The smallest case of test_conv_dma_paired_column_blocks (N = 40) is 76
    tiles of 36 slices on 171 workgroups -- odd, never paired; N = 39 is 74 tiles on 166."""
    from deeplip_amd import _lib
    geom = (39, 11, 11, 128, 256, 3, 3, 1, 1, 1)
    _ring_off_others(dbg)
    dbg(_lib.DBG_NINNER, ninner)
    dbg(_lib.DBG_STREAMK, 2)
    route = f"ring kernel, column-block order {ninner}, split output, balanced split forced"
    D = conv_data(geom, True, True, False)

    def chk(d):
        assert kind(d) == 0 and plan(d, 3) == (128, 128), route
        tiles, nk = -(-d.N * d.Ho * d.Wo // 128) * 2, 9 * (d.C // 32)
        G = tiles * nk // 16             # at least 16 slices per workgroup (far fewer workgroups than the chip has slots)
        assert (tiles, G) == (74, 166) and G % 2 == 0 and G * nk != tiles * nk, route

    def body(a):
        mark_slabs()
        out = launch_conv(ops, a, D, geom, "split", out_split=True, route=chk)
        torch.cuda.synchronize()
        assert slabs_used(), f"{route}: the launch cut no tile"
        assert int(_workspace()[0].abs().max()) == 0, f"{route}: ticket words not back at zero"
        return out
    got = both_fills(ops, monkeypatch, route, body)
    assert_v(got, D, route)


@pytest.mark.parametrize("geom,epi1", [((50, 1, 1, 64, 128, 3, 3, 1, (1, 1), 1), False), ((70, 3, 3, 64, 128, 3, 3, 1, 1, 1), True)],
                         ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_ring_kernel_grouped_twin(ops, dbg, monkeypatch, geom, epi1):
    """Border groups (dlip_debug_set(10, 1)) at the smallest cases of tests/test_conv_grouped_gpu.py: a single one-tap group, and
    nine one-position groups with residual and split output; the balanced split off and forced."""
    from deeplip_amd import _lib
    _ring_off_others(dbg)
    dbg(_lib.DBG_DMA_TILE, TILE_256x128)
    dbg(_lib.DBG_GROUPED, 1)
    D = conv_data(geom, True, epi1, True)
    for split in (0, 2):
        dbg(_lib.DBG_STREAMK, split)
        route = f"ring kernel, grouped twin, {'split' if epi1 else 'fp32'} output, balanced split {'forced' if split else 'off'}"

        def chk(d):
            assert kind(d) == 0 and plan(d, 3) == DMA_CFG[TILE_256x128], route

        def body(a):
            n0 = grouped_launches()
            mark_slabs()
            out = launch_conv(ops, a, D, geom, "split", out_split=epi1, route=chk)
            torch.cuda.synchronize()
            assert grouped_launches() - n0 == 1, route
            # (the single one-tap group is one tile of two slices: nothing to cut; the nine tiles of 98 slices in all go to six workgroups)
            assert slabs_used() == (split == 2 and geom[1] == 3), route
            assert int(_workspace()[0].abs().max()) == 0, f"{route}: ticket words not back at zero"
            return out
        got = both_fills(ops, monkeypatch, route, body)
        assert_v(got, D, route)


# ---- d. the window kernel ----
WIN = [  # rows of test_kernels_gpu.py's WIN_CASES: geometry, residual, split output
    ((4, 11, 11, 96, 48, 3, 3, 1, 2, 2), False, False),     # ragged K = 48 (no split residual / output: K % 32), dilation 2
    ((1, 3, 3, 64, 64, 3, 3, 1, 1, 1), True, True),         # image smaller than a tile, split output, residual
    ((3, 7, 9, 64, 96, 3, 3, 1, 1, 1), False, False),       # 64 < K < 128
]


@pytest.mark.parametrize("geom,use_res,out_split", WIN, ids=lambda v: _ids(v) if isinstance(v, tuple) else str(v))
def test_window_kernel(ops, monkeypatch, geom, use_res, out_split):
    route = f"window kernel, {'split' if out_split else 'fp32'} output"
    D = conv_data(geom, True, use_res, False)

    def chk(d):
        assert kind(d) == 1, route
    got = both_fills(ops, monkeypatch, route, lambda a: launch_conv(ops, a, D, geom, "split", out_split=out_split, route=chk))
    assert_v(got, D, route)


# ---- e. the rows kernel ----
ROWS = [(1, 40, 64, 256, 1, 1, False), (1, 70, 32, 288, 2, 3, True)]      # B, T, C, K, S, dilation, post affine (K = 256 + 32)


def _rows_geom(c):
    B, T, Cc, K, S, dil, _ = c
    return (B, 1, T, Cc, K, 1, S, 1, 0, dil)


@pytest.mark.parametrize("mi", [3, 4, 5])
@pytest.mark.parametrize("case", ROWS, ids=_ids)
def test_rows_kernel(ops, dbg, monkeypatch, case, mi):
    from deeplip_amd import _lib
    dbg(_lib.DBG_ROWS, mi)
    geom = _rows_geom(case)
    D = conv_data(geom, True, False, case[6])
    for out_split in (False, True):
        route = f"rows kernel, MI {mi}, {'split' if out_split else 'fp32'} output"

        def chk(d):
            assert kind(d) == 2 and plan(d, 3) == (32 * mi, 256), route
        got = both_fills(ops, monkeypatch, route, lambda a: launch_conv(ops, a, D, geom, "split", out_split=out_split, route=chk))
        assert_v(got, D, route)


@pytest.mark.parametrize("mi", [3, 4, 5])
def test_rows_kernel_statistics_epilogue(ops, dbg, monkeypatch, mi):
    """conv_nhwc(stats=...) at the smallest rows shape (forced: conv_stats_chunks is non-zero for it): every one of the [chunks][K][2]
    doubles is written and nothing behind them.  The wrapper refuses channel offsets here: x and y are one-sided slices (a pitch)."""
    from deeplip_amd import _lib
    dbg(_lib.DBG_ROWS, mi)
    geom = _rows_geom(ROWS[0])
    N, _, T, Cc, K, _, S, _, _, dil = geom
    n = ops.conv_stats_chunks(N, 1, T, Cc, K, 1, S, dil=(1, dil))
    assert n > 0
    route = f"rows kernel, MI {mi}, statistics epilogue ({n} chunks)"
    D = conv_data(geom, True, False, False)

    def chk(d):
        assert kind(d) == 2 and plan(d, 3) == (32 * mi, 256) and int(_lib.lib().dlip_conv_stats_chunks(C.byref(d))) == n, route
    got = both_fills(ops, monkeypatch, route, lambda a: launch_conv(ops, a, D, geom, "split", route=chk, stats_chunks=n))
    assert_v(got, D, route)
    rows = D["ref"].reshape(-1, K)
    tot = got["stats"].view(n, K, 2).sum(0)
    # (fp32 sums within a chunk of <= 80 rows of a TOL-grade y)
    assert rel_err(tot[:, 0].numpy(), rows.sum(0).numpy()) < TOL and rel_err(tot[:, 1].numpy(), (rows * rows).sum(0).numpy()) < TOL, route


def _pool_refs(rows, G, group, lens=None):
    seg = [rows[g * group: g * group + (group if lens is None else lens[g])] for g in range(G)]
    return torch.stack([s.mean(0) for s in seg]), torch.stack([s.std(0) for s in seg])


def _pool_body(ops, arena, D, group, lens, with_znorm):
    """conv_pool takes no pitch: x keeps its row fences; the partials and the finished rows come from the arena."""
    x = arena.fenced(_split_encode(D["x"]).cuda(), "x")
    vec = lambda t, n: arena.vector(t.cuda() if t is not None else None, n)      # noqa: E731
    ln = arena.fenced(torch.tensor(lens, dtype=torch.int32).cuda(), "lengths") if lens is not None else None
    p = ops.conv_pool(x, vec(D["ws"], "w_split"), vec(D["b"], "bias"), vec(D["sc"], "w_scale"), group, pad=D["pd"], dil=D["dl"],
                      slope=vec(D["slope"], "slope"), post_scale=vec(D["ps"], "post_scale"), post_shift=vec(D["pt"], "post_shift"), lengths=ln)
    # (the partial block itself is an output too: every double of it is written -- padding columns and empty segments included)
    out = {"partials": p.partials, "mean": ops.pool_finish(p, "mean"), "meanstd": ops.pool_finish(p, "meanstd")}
    mss = ops.pool_finish(p, "meanstd", out_split=True)
    out["meanstd.split"] = mss
    out["meanstd.unpacked"] = ops.split_unpack(mss)
    if with_znorm:
        G = out["mean"].shape[0]
        a = arena.fenced(rnd(G, 40, seed=15).cuda(), "a")
        out["znorm_cat_pooled"] = ops.znorm_cat_pooled(a, p)
        out["znorm_cat"] = ops.znorm_cat(a, out["mean"])
    return p, out


def _check_pool(got, D, geom, group, lens, route):
    K = geom[4]
    rows = D["ref"].reshape(-1, K)
    G = -(-rows.shape[0] // group)
    mean, std = _pool_refs(rows, G, group, lens)
    assert rel_err(got["mean"].numpy(), mean.numpy()) < TOL, route
    assert rel_err(got["meanstd"][:, :K].numpy(), mean.numpy()) < TOL and rel_err(got["meanstd"][:, K:].numpy(), std.numpy()) < TOL, route
    un = got["meanstd.unpacked"]
    assert un.shape[1] == (2 * K + 31) // 32 * 32 and rel_err(un[:, :2 * K].numpy(), torch.cat([mean, std], 1).numpy()) < TOL, route
    if un.shape[1] > 2 * K:       # the channel padding of the last 32-block is zeroed (what is behind it: the arena's fence)
        assert float(un[:, 2 * K:].abs().max()) == 0.0, route
    if "znorm_cat" in got:
        assert torch.equal(_bits(got["znorm_cat_pooled"]), _bits(got["znorm_cat"])), route


@pytest.mark.parametrize("mi", [3, 4, 5])
def test_rows_kernel_pooled_epilogue(ops, dbg, monkeypatch, mi):
    """The smallest POOL_CASES row with H == 1 (group == 128 rows), forced onto the rows kernel."""
    from deeplip_amd import _lib
    dbg(_lib.DBG_ROWS, mi)
    geom, group = (2, 1, 300, 64, 96, 1, 1, 1, 0, 1), 128
    route = f"rows kernel, MI {mi}, pooled epilogue"
    D = conv_data(geom, True, False, False)

    def body(a):
        p, out = _pool_body(ops, a, D, group, None, False)
        assert p.tile_rows == 16 * mi, route
        return out
    _check_pool(both_fills(ops, monkeypatch, route, body), D, geom, group, None, route)


# ---- f. the two-source launch ----
@pytest.mark.parametrize("out_split", [False, True])
def test_two_source_launch(ops, dbg, monkeypatch, out_split):
    """conv2_nhwc at the smallest SHORTCUT_CASES row (1, 4, 32, 64 on the 64 x 64 tile).  The wrapper takes no pitches: x, x2 keep
    their row fences, the output comes from the arena."""
    from deeplip_amd import _lib, packing
    from deeplip_amd._lib import ConvDesc
    N, Hin, C2, K, tile = 1, 4, 32, 64, 3
    Ho = (Hin - 1) // 2 + 1
    x = _split_value(rnd(N, Hin, Hin, C2, seed=51) * 2.0)
    h = _split_value(rnd(N, Ho, Ho, K, seed=52) * 2.0)
    w2 = rnd(K, K, 3, 3, seed=53, scale=1.0 / np.sqrt(9 * K))
    wd = rnd(K, C2, 1, 1, seed=54, scale=1.0 / np.sqrt(C2))
    b = rnd(K, seed=55, scale=0.1)
    slope = torch.rand(K, generator=torch.Generator().manual_seed(5)) * 0.3
    ref = F.conv2d(h.permute(0, 3, 1, 2).double(), w2.double(), None, padding=1) + \
        F.conv2d(x.permute(0, 3, 1, 2).double(), wd.double(), None, stride=2) + b.double().view(1, K, 1, 1)
    ref = torch.where(ref >= 0, ref, ref * slope.double().view(1, K, 1, 1)).permute(0, 2, 3, 1).contiguous()
    ws, sc = packing.split_weights(torch.cat([w2.double().permute(0, 2, 3, 1).reshape(K, -1), wd.double().reshape(K, C2)], dim=1))
    _ring_off_others(dbg)       # (a two-source launch goes to the ring kernel whatever they say; the query below looks at d alone)
    dbg(_lib.DBG_DMA_TILE, tile)
    route = f"ring kernel, two sources, tile {tile} = {DMA_CFG[tile]}, {'split' if out_split else 'fp32'} output"
    d = ConvDesc(N, Ho, Ho, K, K, 3, 3, 1, 1, 1, 1, 1, 1, Ho, Ho, K, K, 0)
    assert kind(d) == 0 and plan(d, 3) == DMA_CFG[tile], route

    def body(a):
        y = ops.conv2_nhwc(a.fenced(_split_encode(h).cuda(), "x"), a.fenced(_split_encode(x).cuda(), "x2"), a.vector(ws.cuda(), "w_split"),
                           a.vector(b.cuda(), "bias"), a.vector(sc.cuda(), "w_scale"), pad=(1, 1), stride2=(2, 2),
                           slope=a.vector(slope.cuda(), "slope"), out_split=out_split)
        return {"y.raw": y, "y": ops.split_unpack(y) if out_split else y}
    got = both_fills(ops, monkeypatch, route, body)
    assert_v(got, {"ref": ref}, route)


# ---- g. the pooled epilogue of the ring kernel and its finishers ----
POOLED = [  # rows of POOL_CASES as (geometry, group rows, post affine, lengths)
    ((3, 1, 150, 512, 192, 1, 3, 1, 0, 2), 146, True, None),                          # the smallest whose groups straddle a 128-row tile
    ((5, 1, 278, 512, 1500, 1, 1, 1, 0, 1), 278, False, [278, 100, 2, 200, 277]),    # ragged; 2 K = 3000: 8 padding channels when split
]


@pytest.mark.parametrize("geom,group,post,lens", POOLED, ids=["146-row-groups", "lengths-K1500"])
def test_pooled_epilogue_and_finishers(ops, monkeypatch, geom, group, post, lens):
    """conv_pool -> pool_finish in both modes (and split) -> znorm_cat_pooled: W and R on the arena's partial block and on every
    finished tensor, V on the finished rows."""
    route = "ring kernel, pooled epilogue" + (" with lengths" if lens else "")
    D = conv_data(geom, True, False, post)

    def body(a):
        p, out = _pool_body(ops, a, D, group, lens, True)
        assert p.tile_rows == 128 and group % p.tile_rows != 0, route
        return out
    _check_pool(both_fills(ops, monkeypatch, route, body), D, geom, group, lens, route)


# ---- h. the weight gradient run as a convolution, reference layout ----
@pytest.mark.parametrize("sk", [-1, 4], ids=["reduce-launch", "in-kernel-finisher"])
@pytest.mark.parametrize("N,H,Cc,K,stride", [(225, 12, 64, 128, 2), (225, 6, 96, 128, 1)])
def test_wgrad_reference_layout_scatter(ops, dbg, monkeypatch, N, H, Cc, K, stride, sk):
    """dlip_wgrad_conv_f16x3 with R, S given stores dW[k][c][r][s] for r < R, s < S "and nowhere otherwise" (stride 2 computes a
    remainder row and column beside them): out is a fenced [K, C, 3, 3]; bit for bit wgrad_as_conv on plain tensors.

    The two stores behind it -- slab_reduce_kernel's scatter through a plain pointer, and the in-kernel finisher's band store
    (dlip_debug_set(3, 4)) -- exist only where the launch cuts few tiles many ways: a reduction of nk = Ho Wo N32 / 32 >= 256 slices,
    at most 64 tiles, at least 4 parts per tile.  These are the smallest shapes that get there with 6 x 6 gradient maps: 36 taps x 8
    slices of 32 images (N = 225 is the fewest for eight) = 288 slices, 4 tiles of 256 x 128 cut into 18 parts each (at least 16
    slices per workgroup).  (33 x 6 x 6 stride 2 and 5 x 6 x 6 are 18 and 36 slices: one plain launch whatever the key says.)
    Which of the two finished a launch cannot be queried; the slabs tell: the reduce launch has EVERY part published to its own slab,
    the finisher's launch has written slabs as well -- and the ticket words are back at zero."""
    from deeplip_amd import _lib, autograd_video as av
    dbg(_lib.DBG_STREAMK, sk)
    Ho = (H + 2 - 3) // stride + 1
    # the launch arithmetic restated (conv_igemm_f16x3_dma.hip, launch_one): the "convolution" has M = C R' S' rows
    Rp = (H + 2 - stride * (Ho - 1) - 1) + 1
    nk, tiles = Ho * Ho * ((N + 31) // 32), -(-Cc * Rp * Rp // 256) * (K // 128)
    G = tiles * nk // 16 // tiles * tiles
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert nk >= 256 and tiles <= 64 and G // tiles >= 4 and tiles * nk < 16 * cus and Rp == (4 if stride == 2 else 3), (nk, tiles, G, Rp)
    slab = 256 * 128 * 4
    x = rnd(N, H, H, Cc, seed=61).cuda()
    dy = (rnd(N, Ho, Ho, K, seed=62) * 1e-3).cuda()
    want = av.wgrad_as_conv(x, dy, 3, 3, (stride, stride), (1, 1), (1, 1)).clone()
    xT, _ = av.wgrad_image(x)
    scale2 = av.pow2_lift(dy)
    gT, _ = av.wgrad_image(dy, scale2)
    inv = av.lift_inv(scale2, K).clone()
    torch.cuda.synchronize()
    N32 = xT.shape[3]
    route = f"ring kernel, weight gradient [K, C, R, S], DBG_STREAMK {sk}"
    assert tuple(want.shape) == (K, Cc, 3, 3) and 2 * G * slab <= SLAB_MARK, route

    def body(a):
        out = a.filled((K, Cc, 3, 3), "cuda", torch.float32, "dw")
        mark_slabs()
        _lib.call("dlip_wgrad_conv_f16x3", a.fenced(xT, "x_img"), a.fenced(gT, "g_img"), a.vector(inv, "post_scale"),
                  a.vector(torch.zeros(K, device="cuda"), "post_shift"), a.vector(torch.ones(K, device="cuda"), "unit_scale"), out,
                  Cc, H, H, K, Ho, Ho, N32, stride, stride, 1, 1, 1, 1, 3, 3)
        torch.cuda.synchronize()
        written = slabs_written(slab, 2 * G)        # part g publishes to slab 2 g (a part that starts mid-tile: 2 g + 1 -- none here)
        if sk == -1:
            assert written == [g % 2 == 0 for g in range(2 * G)], f"{route}: not every one of the {G} parts was published: {written}"
        else:
            assert any(written) and not any(written[1::2]), f"{route}: the launch cut no tile: {written}"
        assert int(_workspace()[0].abs().max()) == 0, f"{route}: ticket words not back at zero"
        return {"dw": out}
    got = both_fills(ops, monkeypatch, route, body)
    assert torch.equal(_bits(got["dw"]), _bits(want.cpu())), route


# ---- i. the stems ----
@functools.lru_cache(maxsize=None)
def _stem_params():
    from deeplip_amd import packing
    w = rnd(64, 1, 5, 7, 7, seed=12, scale=1.0 / np.sqrt(245))
    wp = torch.zeros(248, 64)
    wp[:245] = w.reshape(64, 245).t()
    img, sc = packing.split_stem_weights(w.double())
    slope = torch.rand(64, generator=torch.Generator().manual_seed(14)) * 0.3
    return w, wp, img, sc, rnd(64, seed=13, scale=0.1), slope


@pytest.mark.parametrize("which", ["stem3d", "stem3d-split-weights", "stem3d_pool", "stem3d_pool-lengths", "stem3d_pool_u8"])
@pytest.mark.parametrize("B,T,H,W", [(1, 2, 20, 30), (1, 3, 24, 24)])
def test_stems(ops, monkeypatch, B, T, H, W, which):
    """The input fenced, the outputs (and the fused kernels' workspace) from the arena: W and R; V for the two plain stems.  With
    ``lengths`` the padded frames are poisoned / zeroed as well: they are read as zeros "whatever x holds there"."""
    w, wp, img, sc, b, slope = _stem_params()
    x = rnd(B, T, H, W, seed=11) * 2.0
    crop = min(H, W)
    frames = torch.randint(0, 256, (B, T, H, W), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    route = f"stem: {which}"
    L = T - 1

    def body(a):
        v = lambda t, n: a.vector(t.cuda(), n)      # noqa: E731
        if which == "stem3d":
            y = ops.stem3d(a.fenced(x.cuda(), "x"), v(wp, "w"), v(b, "bias"), v(slope, "slope"))
        elif which == "stem3d-split-weights":
            y = ops.stem3d(a.fenced(x.cuda(), "x"), v(img, "w_img"), v(b, "bias"), v(slope, "slope"), w_scale=v(sc, "w_scale"))
        elif which == "stem3d_pool":
            y = ops.stem3d_pool(a.fenced(x.cuda(), "x"), v(img, "w_img"), v(b, "bias"), v(slope, "slope"), v(sc, "w_scale"))
        elif which == "stem3d_pool-lengths":
            xd = a.fenced(x.cuda(), "x")
            xd[:, L:].view(-1).view(torch.int32)[:] = 0x7FC07FC0 if a.fill == POISON else 0     # the padded frames
            ln = a.fenced(torch.tensor([L] * B, dtype=torch.int32).cuda(), "lengths")
            y = ops.stem3d_pool(xd, v(img, "w_img"), v(b, "bias"), v(slope, "slope"), v(sc, "w_scale"), lengths=ln)
        else:
            y = ops.stem3d_pool_u8(a.fenced(frames.cuda(), "frames"), v(img, "w_img"), v(b, "bias"), v(slope, "slope"), v(sc, "w_scale"), crop=crop)
        return {"y": y}
    got = both_fills(ops, monkeypatch, route, body)
    if which.startswith("stem3d") and "pool" not in which:
        ref = F.prelu(F.conv3d(x[:, None].double(), w.double(), b.double(), stride=(1, 2, 2), padding=(2, 3, 3)), slope.double())
        y = got["y"].view(B, T, H // 2, W // 2, 64).permute(0, 4, 1, 2, 3)
        assert rel_err(y.numpy(), ref.numpy()) < TOL, route


# ---- j. the split workspace ----
def test_split_workspace_is_respected(ops, dbg, monkeypatch):
    """A side stream's workspace of exactly dlip_conv_workspace_bytes() carved from a Fenced; case c's forced-split launches run
    there: the slabs are used, both fences stay intact, the ticket words are back at zero."""
    from deeplip_amd import _lib
    need = int(_lib.lib().dlip_conv_workspace_bytes())
    assert need > (1 << 18)
    _ring_off_others(dbg)
    dbg(_lib.DBG_STREAMK, 2)
    ws = Fenced(need, "cuda", POISON, name="split workspace")
    block = ws.payload
    side = torch.cuda.Stream()
    key = (torch.cuda.current_device(), side.cuda_stream)
    torch.cuda.synchronize()
    try:
        with torch.cuda.stream(side):
            _lib.call("dlip_conv_set_workspace", block.data_ptr(), need, stream=side.cuda_stream)
            _lib._workspaces[key] = block
            for geom, use_res in RING_SHAPES:
                D = conv_data(geom, True, use_res, True)
                for tile in range(6):
                    dbg(_lib.DBG_DMA_TILE, tile)
                    for out_split in (False, True):
                        route = (f"ring kernel on a fenced workspace, tile {tile} = {DMA_CFG[tile]}, {'split' if out_split else 'fp32'} "
                                 "output, balanced split forced")

                        def chk(d):
                            assert kind(d) == 0 and plan(d, 3) == DMA_CFG[tile], route

                        def body(a):
                            mark_slabs()                    # (of the current stream's workspace: the fenced block)
                            out = launch_conv(ops, a, D, geom, "split", out_split=out_split, route=chk)
                            torch.cuda.synchronize()
                            assert slabs_used(), f"{route}: the launch did not use the registered workspace's slabs"
                            return out
                        got = both_fills(ops, monkeypatch, route, body)
                        assert_v(got, D, route)
                        ws.check()
                        assert int(block[: 4 << 16].view(torch.int32).abs().max()) == 0, f"{route}: ticket words not back at zero"
        torch.cuda.synchronize()
        ws.check()
    finally:
        torch.cuda.synchronize()
        _lib.call("dlip_conv_set_workspace", None, 0, stream=side.cuda_stream)          # unregister
        _lib._workspaces.pop(key, None)
