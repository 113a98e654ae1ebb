"""One route per convolution launch: what dlip_conv_route reports for a launch, the label ops.* hands to its launch hook and the
route the launch itself recorded (dlip_conv_last_route_query) are one answer, on every kernel and under the debug keys that
pick an instance."""
import ctypes as C

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5        # the bound tests/test_conv_footprint_gpu.py holds every forced tile of a kernel to (there against fp64)
RING, WIN, ROWS, STAGED, F32 = "conv_igemm_f16x3_dma_kernel", "conv_win_f16x3_kernel", "conv_rows_f16x3_kernel", "conv_igemm_f16x3_kernel", "conv_igemm_f32_kernel"
KINDS = (RING, WIN, ROWS, STAGED, F32)


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
    try:
        yield set_
    finally:
        for k in touched:
            _lib.debug_set(k, -1)


def pick_tile(M, K, eff):
    """conv_common.h's picker of the register kernels' tile, restated: fewest rounds of one tile per CU, weighted."""
    best, best_cost = None, 1e300
    for (bm, bn), e in zip([(128, 128), (128, 64), (64, 64), (64, 128), (96, 128)], eff):
        tiles = ((M + bm - 1) // bm) * ((K + bn - 1) // bn)
        cost = ((tiles + 255) // 256) * bm * bn / e
        if cost < best_cost * 0.999:
            best, best_cost = (bm, bn), cost
    return best


EFF_F32, EFF_F16X3 = (0.90, 0.97, 0.93, 1.00, 0.97), (0.95, 0.93, 0.80, 1.00, 0.90)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * scale


def route_of(d, mode, epilogue, C2=0, unaligned=0):
    from deeplip_amd import _lib
    kind, bm, bn = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.call("dlip_conv_route", C.byref(d), mode, epilogue, C2, unaligned, C.byref(kind), C.byref(bm), C.byref(bn))
    return kind.value, bm.value, bn.value


def last_route():
    """(kind, bm, bn) of this thread's most recent convolution launch, and how many it has made."""
    from deeplip_amd import _lib
    out = (C.c_int64 * 4)()
    fn = _lib.lib().dlip_conv_last_route_query
    fn.argtypes, fn.restype = [C.POINTER(C.c_int64)], C.c_int
    _lib.check(fn(out), "dlip_conv_last_route_query")
    return (int(out[0]), int(out[1]), int(out[2])), int(out[3])


def check_launch(ops, d, mode, epilogue, want_label, launch, C2=0):
    """The three assertions of this file around ONE launch; returns what ``launch()`` returns."""
    from deeplip_amd import plan
    before = route_of(d, mode, epilogue, C2)
    n0 = last_route()[1]
    hook, prev = plan._NameHook(), ops.LAUNCH_HOOK
    ops.LAUNCH_HOOK = hook
    try:
        out = launch()
    finally:
        ops.LAUNCH_HOOK = prev
    torch.cuda.synchronize()
    ran, n1 = last_route()
    tag = ",dual" if C2 else ",pool" if epilogue == 2 else ""
    assert [h[0] for h in hook.seen] == [want_label], (hook.seen, want_label)
    assert want_label == f"{KINDS[before[0]]}<{before[1]},{before[2]}{tag}>"
    assert ran == before, (ran, before)
    assert n1 == n0 + 1
    return out


def conv_case(ops, N, H, W, Cin, K, R, S, stride, pad, *, mode, out_split=False):
    """(descriptor, launch) of a plain convolution through ops.conv_nhwc; mode as dlip_conv_route's."""
    from deeplip_amd import packing
    from deeplip_amd.ops import _conv_desc
    x = rnd(N, H, W, Cin, seed=1).cuda()
    w = rnd(K, R, S, Cin, seed=2, scale=(Cin * R * S) ** -0.5)
    b = rnd(K, seed=3, scale=0.1).cuda()
    d = _conv_desc(N, H, W, Cin, K, R, S, stride, pad, (1, 1))
    if mode == 0:
        return d, lambda: ops.conv_nhwc(x, w.cuda(), b, stride=stride, pad=pad)
    ws, sc = packing.split_weights(w.double())
    xs = ops.split_pack(x) if mode == 3 else x
    return d, lambda: ops.conv_nhwc(xs, ws.cuda(), b, stride=stride, pad=pad, w_scale=sc.cuda(), x_split=mode == 3, out_split=out_split)


def test_register_kernels(ops):
    d, launch = conv_case(ops, 1, 3, 3, 4, 4, 1, 1, (1, 1), (0, 0), mode=0)
    check_launch(ops, d, 0, 0, "%s<%d,%d>" % ((F32,) + pick_tile(9, 4, EFF_F32)), launch)
    d, launch = conv_case(ops, 1, 3, 3, 8, 8, 1, 1, (1, 1), (0, 0), mode=1)
    check_launch(ops, d, 1, 0, "%s<%d,%d>" % ((STAGED,) + pick_tile(9, 8, EFF_F16X3)), launch)


def test_ring_kernel(ops):
    d, launch = conv_case(ops, 1, 6, 6, 32, 32, 3, 3, (2, 2), (1, 1), mode=3)       # M = 9
    check_launch(ops, d, 3, 0, f"{RING}<64,64>", launch)


@pytest.mark.parametrize("win,Cin,K,label", [(-1, 64, 64, f"{WIN}<128,64>"), (-1, 32, 128, f"{WIN}<128,128>"), (4, 64, 64, f"{WIN}<256,64>"),
                                            (6, 32, 128, f"{WIN}<256,128>"), (0, 64, 64, f"{RING}<64,64>")])
def test_window_kernel_and_its_geometry_keys(ops, dbg, win, Cin, K, label):
    from deeplip_amd import _lib
    dbg(_lib.DBG_WIN, win)
    for out_split in (False, True):
        d, launch = conv_case(ops, 1, 3, 3, Cin, K, 3, 3, (1, 1), (1, 1), mode=3, out_split=out_split)
        check_launch(ops, d, 3, int(out_split), label, launch)


@pytest.mark.parametrize("rows,label", [(3, f"{ROWS}<96,256>"), (4, f"{ROWS}<128,256>"), (5, f"{ROWS}<160,256>"), (0, f"{RING}<64,64>")])
def test_rows_kernel_forced_heights(ops, dbg, rows, label):
    from deeplip_amd import _lib
    dbg(_lib.DBG_ROWS, rows)
    d, launch = conv_case(ops, 1, 1, 40, 32, 32, 1, 3, (1, 1), (0, 0), mode=3)      # M = 38
    check_launch(ops, d, 3, 0, label, launch)


@pytest.mark.parametrize("rows,label,tile_rows", [(-1, f"{RING}<128,128,pool>", 128), (3, f"{ROWS}<96,256,pool>", 48)])
def test_pooled_launch(ops, dbg, rows, label, tile_rows):
    from deeplip_amd import _lib, packing
    from deeplip_amd.ops import _conv_desc
    dbg(_lib.DBG_ROWS, rows)
    xs = ops.split_pack(rnd(2, 1, 128, 32, seed=1).cuda())
    ws, sc = packing.split_weights(rnd(32, 1, 1, 32, seed=2, scale=32 ** -0.5).double())
    ws, sc, b = ws.cuda(), sc.cuda(), rnd(32, seed=3, scale=0.1).cuda()
    d = _conv_desc(2, 1, 128, 32, 32, 1, 1, (1, 1), (0, 0), (1, 1))
    assert ops.conv_pool_tile_rows(xs, ws) == tile_rows
    p = check_launch(ops, d, 3, 2, label, lambda: ops.conv_pool(xs, ws, b, sc, 128))
    assert p.tile_rows == tile_rows


def _two_sources(ops, N, H, Cx, C2, K, stride, stride2):
    """(descriptor, launch) of ops.conv2_nhwc: 3x3 pad 1 over x [N,H,H,Cx] + the 1x1 shortcut over x2 [N,H,H,C2]."""
    from deeplip_amd import packing
    from deeplip_amd.ops import _conv_desc
    xs = ops.split_pack(rnd(N, H, H, Cx, seed=1).cuda())
    x2 = ops.split_pack(rnd(N, H, H, C2, seed=2).cuda())
    w = torch.cat([rnd(K, 9 * Cx, seed=3, scale=(9 * Cx) ** -0.5), rnd(K, C2, seed=4, scale=C2 ** -0.5)], dim=1)
    ws, sc = packing.split_weights(w.double())
    ws, sc, b = ws.cuda(), sc.cuda(), rnd(K, seed=5, scale=0.1).cuda()
    d = _conv_desc(N, H, H, Cx, K, 3, 3, stride, (1, 1), (1, 1))
    return d, lambda: ops.conv2_nhwc(xs, x2, ws, b, sc, stride=stride, pad=(1, 1), stride2=stride2, out_split=False)


def test_two_sources(ops):
    d, launch = _two_sources(ops, 1, 8, 32, 32, 32, (2, 2), (2, 2))                 # M = 16
    check_launch(ops, d, 3, 0, f"{RING}<64,64,dual>", launch, C2=32)


def test_two_sources_tile_counts_both_sources_slices(ops, dbg):
    """M = 8192, 27 slices of x + 5 of x2 = 32: the 256 x 128 tile's threshold is met by the SUM, which is what the launch always
    picked with (the label used to be picked with the 27).  Same values as on the 128 x 128 tile, to the bound this suite holds
    every forced tile of the ring kernel to."""
    from deeplip_amd import _lib
    d, launch = _two_sources(ops, 8, 32, 96, 160, 128, (1, 1), (1, 1))
    y = check_launch(ops, d, 3, 0, f"{RING}<256,128,dual>", launch, C2=160).clone()
    dbg(_lib.DBG_DMA_TILE, 0)
    y0 = check_launch(ops, d, 3, 0, f"{RING}<128,128,dual>", launch, C2=160)
    err = rel_err(y.cpu().double().numpy(), y0.cpu().double().numpy())
    print(f"256x128 against 128x128: rel_err {err:.3e}")
    assert err < TOL


def test_unaligned_query(ops):
    """Query only: a split-input launch whose y or residual is off 16 bytes runs the register-staged kernel on pick_tile's tile."""
    from deeplip_amd.ops import _conv_desc
    d = _conv_desc(1, 6, 6, 32, 32, 3, 3, (2, 2), (1, 1), (1, 1))
    assert route_of(d, 3, 0) == (0, 64, 64)
    assert route_of(d, 3, 0, unaligned=1) == (3,) + pick_tile(9, 32, EFF_F16X3)
