"""Lip-clip augmentation (deeplip_amd/clip_augment.py), host side (-m "not gpu"): the numpy definition
(tests/clip_augment_ref.py) against the oracle's pipelines with every stage off, the invariants of the masks at extreme draws, the
length-free draws, the header's constants, the C ABI (declared, exported, no host pointers, the refusals in front of any launch),
and every host-side refusal of ``ClipAugment`` and of ``train_video.load_args`` in front of the GPU requirement."""
import ctypes
import random

import numpy as np
import pytest
import torch

import clip_augment_ref as ref

NAMES = ("dlip_clip_augment_u8", "dlip_clip_augment_f32", "dlip_clip_augment_workspace_bytes")


def _ca(**kw):
    from deeplip_amd.clip_augment import ClipAugment
    return ClipAugment(**kw)


def _frames(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.int64).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- the definition
@pytest.mark.parametrize("rgb", [False, True])
def test_ref_with_every_stage_off_is_the_oracles_pipelines(rgb):
    from oracle import deeplip_oracle as O
    fr = _frames((3, 4) + ((3,) if rgb else ()) + (21, 26), 1)
    draws = np.full((3, ref.DRAWS), ref.TOP, dtype=np.int32)
    val = ref.clip_augment(fr, None, draws, crop=16)
    assert val["y"].shape == (3, 1, 4, 16, 16) and not val["mask"].any()
    for b in range(3):
        assert np.array_equal(val["y"][b, 0].view(np.uint32), O.video_preprocess_u8(fr[b], 16).view(np.uint32))
    rng = random.Random(3)
    want, cps = zip(*(O.video_preprocess_train_u8(fr[b], rng, crop=16) for b in range(3)))
    assert any(c[2] for c in cps) and not all(c[2] for c in cps)                  # a flipped clip and an unflipped one
    train = ref.clip_augment(fr, [4, 2, 1], draws, crop=16, clip_params=np.array([list(c) + [0] for c in cps], dtype=np.int32))
    for b, n in enumerate([4, 2, 1]):
        assert np.array_equal(train["y"][b, 0, :n].view(np.uint32), want[b][:n].view(np.uint32)) and (train["y"][b, 0, n:] == 0).all()


@pytest.mark.parametrize("r", [0, ref.TOP, -7, 2 ** 30, 123456789])
def test_masks_lie_inside_the_clip_and_the_crop(r):
    row = [r] * ref.DRAWS
    for n in range(1, 12):
        for width, ratio in ((0, 1.0), (3, 1.0), (100, 1.0), (100, 0.5), (5, 0.3), (4, 0.0)):
            cap = ref.time_cap(n, width, ratio)
            assert cap == min(width, int(np.floor(ratio * n))) <= n
            for t0, w in ref.time_masks(n, row, ref.MAX_MASKS, width, ratio):
                assert 0 <= w <= cap and 0 <= t0 and t0 + w <= n
            if r == ref.TOP:
                assert all(w == cap for _, w in ref.time_masks(n, row, 2, width, ratio))       # the widest draw: the cap itself
    for OH, OW in ((8, 8), (88, 88), (5, 12)):
        for size in (0, 1, 3, 8, 88, 1000, 2 ** 30):
            for y0, x0, h, w in ref.cutouts(OH, OW, row, ref.MAX_MASKS, size):
                assert 0 <= h <= min(size, OH) and 0 <= w <= min(size, OW)
                assert 0 <= y0 and y0 + h <= OH and 0 <= x0 and x0 + w <= OW
            if r == ref.TOP and size >= max(OH, OW):
                assert ref.cutouts(OH, OW, row, 1, size) == [(0, 0, OH, OW)]                   # cut_size >= crop is clamped: the whole crop


def test_masked_fill_and_mixup_of_the_ref():
    A = np.random.default_rng(5).standard_normal((5, 8, 8)).astype(np.float32) + np.float32(0.5)
    row = np.zeros(ref.DRAWS, dtype=np.int32)
    row[0], row[1] = ref.TOP, ref.TOP                 # the widest mask, as late as it fits: ends on the last valid frame
    out, m, mean = ref.masked(A, 3, row, n_time=1, time_width=2, fill=1)
    assert m[1:3].all() and not m[0].any() and not m[3:].any() and (out[3:] == 0).all()
    assert (out[1:3] == np.float32(mean)).all() and abs(mean - A[:3].astype(np.float64).mean()) < 1e-12
    x = A[None, None].repeat(2, 0).copy()
    x[1] *= 2
    draws = np.zeros((2, ref.DRAWS), dtype=np.int32)
    y = ref.clip_augment(x, [5, 2], draws, perm=[1, 0], lam=0.25)["y"]
    l, mu = np.float32(0.25), np.float32(0.75)
    assert np.array_equal(y[0, 0, :2], l * x[0, 0, :2] + mu * x[1, 0, :2]) and np.array_equal(y[0, 0, 2:], l * x[0, 0, 2:])
    assert np.array_equal(y[1, 0, :2], l * x[1, 0, :2] + mu * x[0, 0, :2]) and (y[1, 0, 2:] == 0).all()
    same = ref.clip_augment(x, [5, 2], draws, perm=[0, 1], lam=0.25)["y"]             # fixed points: unblended
    assert np.array_equal(same[0, 0], x[0, 0]) and np.array_equal(same[1, 0, :2], x[1, 0, :2])


# ------------------------------------------------------------------------------------------------------------------ the draws
def test_draw_shapes_dtypes_and_ranges():
    from deeplip_amd import _lib, clip_augment as ca
    assert ca.MAX_MASKS == _lib.HEADER["DLIP_CLIPAUG_MAX_MASKS"] == ref.MAX_MASKS
    assert ca.DRAWS == _lib.HEADER["DLIP_CLIPAUG_DRAWS"] == ref.DRAWS == 6 * ca.MAX_MASKS
    assert _lib.HEADER["DLIP_CLIPAUG_MEAN_FRAMES"] >= 1
    d = _ca(time_masks=2, time_width=3).draw(7, np.random.default_rng(0))
    assert sorted(d) == ["draws"] and d["draws"].dtype == np.int32 and d["draws"].shape == (7, ca.DRAWS)
    assert d["draws"].min() >= 0 and d["draws"].max() > 2 ** 30
    seen = set()
    g = np.random.default_rng(1)
    for _ in range(20):
        d = _ca(mixup_alpha=0.4).draw(5, g)
        assert sorted(d) == ["draws", "lam", "perm"]
        assert d["perm"].dtype == np.int32 and sorted(d["perm"].tolist()) == list(range(5))
        assert d["lam"].dtype == np.float32 and d["lam"].shape == (1,) and 0.0 <= float(d["lam"][0]) <= 1.0
        seen.add(tuple(d["perm"].tolist()))
    assert len(seen) > 1
    a, b = (_ca(cutouts=1, cut_size=4, mixup_alpha=1.0).draw(4, np.random.default_rng(9)) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)                                 # the generator alone decides


# -------------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_exported_and_take_no_host_pointer():
    from deeplip_amd import _lib
    VP, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert _lib.PROTOTYPES["dlip_clip_augment_workspace_bytes"] == (I64, [I32, I32])
    assert _lib.PROTOTYPES["dlip_clip_augment_u8"] == (ctypes.c_int, [VP] * 8 + [I64] + [I32] * 8 + [F64, I32, I32, I32, VP])
    assert _lib.PROTOTYPES["dlip_clip_augment_f32"] == (ctypes.c_int, [VP] * 7 + [I64] + [I32] * 6 + [F64, I32, I32, I32, VP])
    l = _lib.lib()
    for n in NAMES:
        assert hasattr(l, n)
    assert "dlip_clip_augment_u8" in _lib.STREAM_LAST and "dlip_clip_augment_f32" in _lib.STREAM_LAST
    F = _lib.HEADER["DLIP_CLIPAUG_MEAN_FRAMES"]                       # one fp64 partial per clip and chunk of F frames
    assert l.dlip_clip_augment_workspace_bytes(3, 5) == 3 * -(-5 // F) * 8 and l.dlip_clip_augment_workspace_bytes(64, 29) == 64 * -(-29 // F) * 8
    assert l.dlip_clip_augment_workspace_bytes(0, 5) < 0 and l.dlip_clip_augment_workspace_bytes(3, 70000) < 0


def test_library_refuses_bad_arguments_before_any_launch():
    """DLIP_EINVAL is returned by host code in front of the launch: made-up addresses are never dereferenced, no device is needed."""
    from deeplip_amd import _lib
    l = _lib.lib()
    P = 4096                                            # a made-up, aligned address
    good = dict(frames=P, cp=None, lens=None, draws=P * 2, perm=None, lam=None, y=P * 3, ws=P * 4, wsb=1 << 20, B=2, T=3, ch=1, Hs=12,
                Ws=12, crop=8, nt=1, tw=2, tr=1.0, nc=1, cs=3, fill=0)
    for bad in (dict(crop=6), dict(crop=16), dict(ch=2), dict(nt=ref.MAX_MASKS + 1), dict(nc=-1), dict(tw=-1), dict(cs=-1), dict(tr=1.5),
                dict(tr=float("nan")), dict(fill=2), dict(perm=P * 5), dict(lam=P * 5), dict(y=P), dict(y=P * 3 + 4), dict(draws=None),
                dict(ws=None), dict(wsb=8), dict(B=0), dict(T=0), dict(ws=P * 4 + 4)):
        a = dict(good, **bad)
        rc = l.dlip_clip_augment_u8(a["frames"], a["cp"], a["lens"], a["draws"], a["perm"], a["lam"], a["y"], a["ws"], a["wsb"], a["B"], a["T"],
                                    a["ch"], a["Hs"], a["Ws"], a["crop"], a["nt"], a["tw"], a["tr"], a["nc"], a["cs"], a["fill"], None)
        assert rc == _lib.HEADER["DLIP_EINVAL"], bad
    assert l.dlip_clip_augment_f32(P, None, P * 2, None, None, P * 3, P * 4, 1 << 20, 2, 3, 8, 6, 1, 2, 1.0, 0, 0, 0, None) == -1      # W % 4
    assert l.dlip_clip_augment_f32(P, None, P * 2, None, None, P, P * 4, 1 << 20, 2, 3, 8, 8, 1, 2, 1.0, 0, 0, 0, None) == -1          # y == x


# -------------------------------------------------------------------------------------------------------------- the refusals
@pytest.mark.parametrize("bad", [
    dict(),                                                       # configurations that would do nothing
    dict(time_masks=2), dict(time_width=5), dict(time_masks=2, time_width=5, time_ratio=0.0), dict(cutouts=2), dict(cut_size=9),
    dict(time_masks=ref.MAX_MASKS + 1, time_width=3), dict(cutouts=ref.MAX_MASKS + 1, cut_size=3),          # counts outside [0, MAX]
    dict(time_masks=-1, time_width=3), dict(time_masks=1.5, time_width=3), dict(time_masks=True, time_width=3),
    dict(time_masks=1, time_width=-3), dict(cutouts=1, cut_size=-1), dict(cutouts=1, cut_size=2 ** 31),
    dict(time_masks=1, time_width=3, time_ratio=1.5), dict(time_masks=1, time_width=3, time_ratio=float("nan")),
    dict(time_masks=1, time_width=3, time_ratio="half"),
    dict(time_masks=1, time_width=3, fill="noise"), dict(time_masks=1, time_width=3, fill=0),
    dict(mixup_alpha=-0.5), dict(mixup_alpha=float("inf")), dict(mixup_alpha=float("nan")), dict(mixup_alpha="1"),
    dict(time_masks=1, time_width=3, crop=0), dict(time_masks=1, time_width=3, crop=90), dict(time_masks=1, time_width=3, crop=-8),
])
def test_constructor_refusals(bad):
    with pytest.raises(ValueError):
        _ca(**bad)


def test_call_refuses_bad_host_values_before_it_asks_for_a_gpu():
    from deeplip_amd._lib import DeepLipHipError
    ca = _ca(time_masks=1, time_width=2, mixup_alpha=0.5, crop=8)
    fr = torch.zeros(3, 5, 12, 12, dtype=torch.uint8)
    good = ca.draw(3, np.random.default_rng(0))
    with pytest.raises(ValueError, match="crop"):
        ca(torch.zeros(3, 5, 12, 6, dtype=torch.uint8), params=good)                              # crop > Ws
    with pytest.raises(ValueError, match="crop"):
        ca(torch.zeros(3, 5, 3, 7, 12, dtype=torch.uint8), params=good)                           # crop > Hs
    with pytest.raises(ValueError):
        ca(torch.zeros(3, 5, 2, 12, 12, dtype=torch.uint8), params=good)                          # two colour planes
    with pytest.raises(ValueError, match="multiple of 4"):
        ca(torch.zeros(3, 1, 5, 8, 6), params=good)                                               # a float clip of width 6
    with pytest.raises(TypeError):
        ca(torch.zeros(3, 5, 12, 12), params=good)                                                # neither source
    with pytest.raises(TypeError):
        ca(np.zeros((3, 5, 12, 12), dtype=np.uint8), params=good)
    with pytest.raises(ValueError, match="permutation"):
        ca(fr, params=dict(good, perm=np.array([0, 0, 1], dtype=np.int32)))
    with pytest.raises(ValueError, match="permutation"):
        ca(fr, params=dict(good, perm=np.array([0, 1, 3], dtype=np.int32)))
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lam"):
            ca(fr, params=dict(good, lam=np.array([lam], dtype=np.float32)))
    with pytest.raises(ValueError, match="exactly"):
        ca(fr, params={"draws": good["draws"]})                                                   # mixup is on: perm and lam are due
    with pytest.raises(ValueError, match="exactly"):
        _ca(time_masks=1, time_width=2, crop=8)(fr, params=good)                                  # mixup is off: they are not
    with pytest.raises(TypeError):
        ca(fr, params=dict(good, draws=good["draws"].astype(np.int64)))
    with pytest.raises(TypeError):
        ca(fr, params=dict(good, draws=good["draws"][:2]))
    with pytest.raises(TypeError):
        ca(fr, params=dict(good, lam=np.array([0.5])))                                            # float64
    with pytest.raises(ValueError, match="lengths"):
        ca(fr, lengths=[5, 0, 1], params=good)
    with pytest.raises(ValueError, match="lengths"):
        ca(fr, lengths=[5, 6, 1], params=good)
    with pytest.raises(ValueError, match="lengths"):
        ca(fr, lengths=[5, 1], params=good)
    with pytest.raises(ValueError, match="clip_params"):
        ca(fr, clip_params=torch.zeros(2, 4, dtype=torch.int32), params=good)
    with pytest.raises(ValueError, match="clip_params"):
        ca(torch.zeros(3, 1, 5, 8, 8), clip_params=torch.zeros(3, 4, dtype=torch.int32), params=good)
    with pytest.raises(ValueError, match="mixup is off"):
        _ca(time_masks=1, time_width=2).mix_targets(torch.zeros(3, dtype=torch.long), good)
    # everything host-side in order: CPU tensors are refused like everywhere else
    with pytest.raises(DeepLipHipError, match="no CPU path"):
        ca(fr, lengths=[5, 3, 1], params=good)
    with pytest.raises(DeepLipHipError, match="no CPU path"):
        ca(torch.zeros(3, 1, 5, 8, 8), params=good)
    with pytest.raises(DeepLipHipError, match="no CPU path"):
        ca.mix_targets(torch.zeros(3, dtype=torch.long), good)


def test_load_args_flags_and_refusals():
    import train_video
    a = train_video.load_args([])
    assert a.clip_augment is None and (a.time_masks, a.time_mask_width, a.cutouts, a.cutout_size, a.mixup_alpha) == (0, 0, 0, 0, 0.0)
    assert (a.time_mask_ratio, a.mask_fill) == (1.0, "mean")
    off = ["--time-masks", "0", "--time-mask-width", "0", "--time-mask-ratio", "1.0", "--cutouts", "0", "--cutout-size", "0",
           "--mask-fill", "mean", "--mixup-alpha", "0"]
    assert train_video.load_args(off).clip_augment is None
    assert train_video.load_args(off + ["--head-only"]).clip_augment is None            # nothing is on: nothing to refuse
    a = train_video.load_args(["--time-masks", "2", "--time-mask-width", "4", "--time-mask-ratio", "0.4", "--cutouts", "1", "--cutout-size",
                               "20", "--mask-fill", "zero", "--mixup-alpha", "0.4"])
    assert a.clip_augment == dict(time_masks=2, time_width=4, time_ratio=0.4, cutouts=1, cut_size=20, fill="zero", mixup_alpha=0.4, crop=88)
    assert train_video.load_args(["--mixup-alpha", "1"]).clip_augment["mixup_alpha"] == 1.0
    for bad in (["--time-masks", "2"], ["--time-mask-width", "4"], ["--cutouts", "1"], ["--cutout-size", "8"],     # would do nothing
                ["--time-masks", "9", "--time-mask-width", "4"], ["--time-masks", "-1", "--time-mask-width", "4"],
                ["--time-masks", "1", "--time-mask-width", "4", "--time-mask-ratio", "2"], ["--mixup-alpha", "-1"],
                ["--mixup-alpha", "0.4", "--head-only"], ["--time-masks", "1", "--time-mask-width", "4", "--head-only"]):
        with pytest.raises(ValueError):
            train_video.load_args(bad)
    with pytest.raises(SystemExit):
        train_video.load_args(["--mask-fill", "noise"])
