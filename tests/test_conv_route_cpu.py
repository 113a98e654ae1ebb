"""The convolution route reporters without a GPU: dlip_conv_plan, dlip_conv_kernel_kind, dlip_conv_stats_chunks and
dlip_conv_pool_partial_bytes are thin callers of the function dlip_conv_route reports, so on a grid of descriptors they must agree
with it -- and with what they answered before they were (tests/golden/conv_route_table.json, recorded from the library before the
change with this module's own loop: `python tests/test_conv_route_cpu.py > tests/golden/conv_route_table.json`).

Without a device the window kernel's probe answers no and the rows kernel assumes 256 CUs."""
import contextlib
import ctypes as C
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_route_table.json")

# 1-D valid convolutions: (N, W, C, K, S, dilation); M = N * (W - dil (S - 1)) on both sides of 4096, K on both sides of 192,
# C off a multiple of 32 (no split-format launch exists: the reporters answer for the ring kernel all the same), K off a multiple of 4
SHAPES = [(64, 296, 512, 512, 1, 1), (64, 300, 512, 512, 3, 2), (256, 278, 512, 1500, 1, 1), (64, 1, 3008, 512, 1, 1),
          (13, 315, 64, 192, 1, 1), (13, 316, 64, 192, 1, 1), (13, 316, 64, 188, 1, 1), (13, 316, 64, 196, 1, 1), (16, 257, 96, 256, 2, 1),
          (64, 296, 48, 512, 1, 1), (64, 296, 64, 198, 1, 1), (2, 128, 32, 32, 1, 1), (40, 300, 128, 512, 3, 1), (100, 300, 64, 512, 1, 1),
          (1, 40, 32, 32, 3, 1), (64, 296, 512, 64, 1, 1)]
KEYS = [("ROWS", -1), ("ROWS", 0), ("ROWS", 1), ("ROWS", 3), ("DMA_ENABLE", 0)]


def _desc(shape, ldr):
    from deeplip_amd._lib import ConvDesc
    N, W, Cin, K, S, dil = shape
    return ConvDesc(N, 1, W, Cin, K, 1, S, 1, 1, 0, 0, 1, dil, 1, W - dil * (S - 1), Cin, K, K if ldr else 0)


def _wrappers(d):
    """What the four older reporters answer for `d`."""
    from deeplip_amd import _lib
    lib = _lib.lib()
    out = {"kind": int(lib.dlip_conv_kernel_kind(C.byref(d)))}
    for mode in (0, 1, 3):
        bm, bn = C.c_int32(), C.c_int32()
        _lib.check(lib.dlip_conv_plan(C.byref(d), mode, C.byref(bm), C.byref(bn)), "dlip_conv_plan")
        out[f"plan{mode}"] = [bm.value, bn.value]
    out["stats_chunks"] = int(lib.dlip_conv_stats_chunks(C.byref(d)))
    rows = C.c_int32()
    out["pool_bytes"] = int(lib.dlip_conv_pool_partial_bytes(C.byref(d), C.byref(rows)))
    out["pool_tile_rows"] = rows.value
    return out


@contextlib.contextmanager
def _debug_key(key, value):
    """The debug key set for the block; back at its built-in value when the block is left, by an assertion too."""
    from deeplip_amd import _lib
    _lib.debug_set(getattr(_lib, "DBG_" + key), value)
    try:
        yield
    finally:
        _lib.debug_set(getattr(_lib, "DBG_" + key), -1)


def _grid(key, value):
    """(name, descriptor) of every grid point under one debug key."""
    return [(f"{key}={value} {shape} ldr={ldr}", _desc(shape, ldr)) for shape in SHAPES for ldr in (0, 1)]


def _route(d, mode, epilogue):
    from deeplip_amd import _lib
    kind, bm, bn = C.c_int32(), C.c_int32(), C.c_int32()
    rc = _lib.lib().dlip_conv_route(C.byref(d), mode, epilogue, 0, 0, C.byref(kind), C.byref(bm), C.byref(bn))
    return (rc, kind.value, bm.value, bn.value)


def _check_point(name, d, want):
    """One grid point: `want` is its row of the recorded table.  Returns 1 (a point checked)."""
    got = _wrappers(d)
    # -- with dlip_conv_route --
    for mode in (0, 1, 3):
        rc, kind, bm, bn = _route(d, mode, 0)
        assert rc == 0 and got[f"plan{mode}"] == [bm, bn], (name, mode)
        if mode != 3:
            assert kind == (4, 3)[mode], (name, mode)
    kind3 = _route(d, 3, 0)[1]
    assert got["kind"] == (kind3 if kind3 in (1, 2) else 0), name
    rc, kind, bm, bn = _route(d, 3, 3)                               # statistics: the rows kernel or nothing
    assert (got["stats_chunks"] > 0) == (rc == 0) and (rc != 0 or kind == 2), name
    rc, kind, bm, bn = _route(d, 3, 2)                               # pooled: a rows launch reports HALF its tile as a partial band
    assert rc == 0 and kind in (0, 2) and got["pool_tile_rows"] == (bm // 2 if kind == 2 else bm), name
    bands = (d.N * d.Wo + got["pool_tile_rows"] - 1) // got["pool_tile_rows"]
    assert got["pool_bytes"] == bands * 4 * ((d.K + 127) // 128 * 128) * 8, name
    # -- with the answers from before the reporters shared the launch's route.  One kind of entry was wrong then and is
    # excepted: an fp32 y with K off a multiple of 4 cannot leave the ring or rows kernel in 16-byte chunks, the launch runs the
    # register-staged kernel (dlip_conv_nhwc_f16x3), and dlip_conv_plan(d, 3) / dlip_conv_kernel_kind named the ring or rows kernel.
    if d.K % 4 != 0:
        assert kind3 == 3 and got["kind"] == 0 and got["plan3"] == got["plan1"], name
        want["kind"], want["plan3"] = got["kind"], got["plan3"]
    assert got == want, name
    return 1


def test_reporters_agree_with_the_route_and_with_their_earlier_answers():
    with open(GOLDEN) as f:
        golden = json.load(f)
    seen = 0
    for key, value in KEYS:
        with _debug_key(key, value):
            for name, d in _grid(key, value):
                seen += _check_point(name, d, dict(golden[name]))
    assert seen == len(golden) == len(KEYS) * len(SHAPES) * 2


if __name__ == "__main__":      # records the table (run from the tree whose library is to answer)
    rows = []
    for key_, value_ in KEYS:
        with _debug_key(key_, value_):
            rows += [f"{json.dumps(name)}: {json.dumps(_wrappers(d))}" for name, d in _grid(key_, value_)]
    print("{\n" + ",\n".join(rows) + "\n}")
