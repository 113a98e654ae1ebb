"""Lip-clip augmentation on the device (-m gpu; deeplip_amd/clip_augment.py): the kernels against the definition
in numpy (tests/clip_augment_ref.py) -- bit for bit with ``fill: zero`` and on every unfilled pixel, the mean fill within its rounding
bound --, a row's bits alone and in a batch, mixup with longer / shorter partners and a fixed point, the footprint of both launches,
device lengths (clamped), a recorded plan, the mixed criterion, and train_video.main with the augmentation flags.

Geometry: the smallest at which the kernel can still go wrong -- gray 12 x 12 frames cropped to 8 x 8 (two quads per row, 16 quads per
frame: one partly filled workgroup), B = 3 clips of T = 5 frames holding 5, 3 and 1 (the mean pass adds up to five partials per clip);
13 x 15 frames for the byte-wise reads; the shipped 96 x 96 -> 88 RGB geometry with an odd ox and a flip (eight workgroups per frame,
the last one partly filled, re-aligned word reads); a float clip [3, 1, 5, 8, 8] with NaN behind the lengths."""
import functools

import numpy as np
import pytest
import torch

import clip_augment_ref as ref
from footprint import POISON, ZEROS, FenceArena

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T, LENS = 3, 5, (5, 3, 1)
FILL_BAR = 1e-6      # a filled pixel: the fp64 sum is exact far beyond fp32, so the single rounding differs by at most one fp32 ulp and a
#                      blend can double it; |pixel| <= 3.6, one ulp there is 2.4e-7, two are 4.8e-7
TOP = ref.TOP


def _ca(**kw):
    from deeplip_amd.clip_augment import ClipAugment
    return ClipAugment(**kw)


@functools.lru_cache(maxsize=None)
def _gray(Hs=12, Ws=12):
    x = np.random.default_rng(100 + Hs).integers(0, 256, size=(B, T, Hs, Ws), dtype=np.int64).astype(np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _float_clip():
    x = np.full((B, 1, T, 8, 8), np.nan, dtype=np.float32)
    for b, n in enumerate(LENS):
        x[b, 0, :n] = np.random.default_rng(200 + b).standard_normal((n, 8, 8)).astype(np.float32) + np.float32(0.5)
    x.setflags(write=False)
    return x


def _draws(seed, rows=B):
    return np.random.default_rng(seed).integers(0, 2 ** 31, size=(rows, ref.DRAWS), dtype=np.int64).astype(np.int32)


def _edge_draws():
    """Row 0 (5 frames): time mask 0 as wide as the cap and as late as it fits (it ends on the last valid frame), time mask 1 of width 0;
    cutout 0 of the largest size in the top left corner, cutout 1 in the bottom right one.  Row 1: cutouts on the top right / bottom
    left.  Row 2 (one frame): a mask over the only frame."""
    d = _draws(7)
    d[0, 0:4] = (TOP, TOP, 0, 0)
    c = 2 * ref.MAX_MASKS
    d[0, c:c + 8] = (TOP, TOP, 0, 0, TOP, TOP, TOP, TOP)
    d[1, c:c + 8] = (TOP, TOP, 0, TOP, TOP, TOP, TOP, 0)
    d[2, 0:2] = (TOP, 0)
    return d


def _kw(ca):
    return dict(n_time=ca.time_masks, time_width=ca.time_width, time_ratio=ca.time_ratio, n_cut=ca.cutouts, cut_size=ca.cut_size,
                fill=("zero", "mean").index(ca.fill))


def _run(ca, src, lens, params, cp=None):
    cpt = None if cp is None else torch.from_numpy(np.asarray(cp, dtype=np.int32)).to(DEV)
    y = ca(torch.from_numpy(np.array(src)).to(DEV), clip_params=cpt, lengths=lens, params=params)
    return y.cpu().numpy()


def _ref(ca, src, lens, params, cp=None):
    lam = None if "lam" not in params else float(params["lam"][0])
    return ref.clip_augment(src, lens, params["draws"], crop=ca.crop, clip_params=cp, perm=params.get("perm"), lam=lam, **_kw(ca))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(ca, src, lens, params, cp=None, what=""):
    got, want = _run(ca, src, lens, params, cp), _ref(ca, src, lens, params, cp)
    assert got.shape == want["y"].shape and not np.isnan(got).any(), what
    m = want["mask"]
    if ca.fill == "zero":
        assert np.array_equal(_bits(got), _bits(want["y"])), what                  # every pixel, the zeros behind the lengths included
    else:
        assert np.array_equal(_bits(got[~m]), _bits(want["y"][~m])), what          # unfilled pixels and the zero tails: exact
        err = np.abs(got[m].astype(np.float64) - want["y"][m].astype(np.float64))
        print(f"{what}: {int(m.sum())} filled pixels, largest |got - ref| {float(err.max()) if err.size else 0.0:.3e} (bar {FILL_BAR:.0e})")
        assert (err <= FILL_BAR).all(), what
    return got, want


# ------------------------------------------------------------------------------------------------- 1. gray uint8, 12 x 12 -> 8
STAGES = {
    "time": dict(time_masks=2, time_width=2),
    "time ratio": dict(time_masks=ref.MAX_MASKS, time_width=4, time_ratio=0.5),
    "cutout": dict(cutouts=2, cut_size=3),
    "cutout whole": dict(cutouts=1, cut_size=100),
    "all": dict(time_masks=2, time_width=2, cutouts=2, cut_size=3),
}


@pytest.mark.parametrize("fill", ["zero", "mean"])
@pytest.mark.parametrize("stage", list(STAGES))
def test_gray_frames_against_the_definition(stage, fill):
    ca = _ca(crop=8, fill=fill, **STAGES[stage])
    edge = _edge_draws()
    if ca.time_masks and ca.time_ratio == 1.0:                      # the draws hit what they are meant to hit
        assert ref.time_masks(5, edge[0], 2, ca.time_width, 1.0) == [(5 - ca.time_width, ca.time_width), (0, 0)]
        assert ref.time_masks(1, edge[2], 1, ca.time_width, 1.0) == [(0, 1)]
    if ca.cutouts == 2:
        assert ref.cutouts(8, 8, edge[0], 2, 3) == [(0, 0, 3, 3), (5, 5, 3, 3)] and ref.cutouts(8, 8, edge[1], 2, 3) == [(0, 5, 3, 3), (5, 0, 3, 3)]
    for name, d in (("edge", edge), ("seed 1", _draws(1)), ("seed 2", _draws(2))):
        got, want = _check(ca, _gray(), list(LENS), {"draws": d}, what=f"{stage}/{fill}/{name}")
        if name == "edge":
            assert want["mask"][0].any()
    if stage == "cutout whole":                                     # cut_size >= crop with the widest draws: the whole clip is the fill
        d = np.full((B, ref.DRAWS), TOP, dtype=np.int32)
        d[:, 2 * ref.MAX_MASKS + 2:2 * ref.MAX_MASKS + 4] = 0
        got, want = _check(ca, _gray(), list(LENS), {"draws": d}, what="whole")
        assert all(want["mask"][b, 0, :n].all() for b, n in enumerate(LENS))


def test_centre_crop_clip_params_and_bytewise_reads():
    """clip_params None = the centre crop; odd origins, flips and out-of-frame origins (clamped); 13 x 15 frames: a buffer that is not
    whole words, read byte by byte."""
    ca = _ca(crop=8, fill="mean", time_masks=1, time_width=2, cutouts=2, cut_size=5)
    for Hs, Ws in ((12, 12), (13, 15)):
        for cp in (None, [[1, 3, 1, 0], [4, 1, 0, 0], [0, 0, 1, 0]], [[-3, 99, 1, 0], [99, -3, 0, 0], [2, 2, 0, 0]]):
            _check(ca, _gray(Hs, Ws), list(LENS), {"draws": _draws(3)}, cp=cp, what=f"{Hs}x{Ws} {cp}")
    plain = _run(_ca(crop=8, cutouts=1, cut_size=1), _gray(), None, {"draws": np.zeros((B, ref.DRAWS), dtype=np.int32)})      # h = w = 0
    from deeplip_amd.frontend import VideoFrontend
    vf = VideoFrontend(8)(torch.from_numpy(np.array(_gray())).to(DEV)).cpu().numpy()
    assert np.array_equal(_bits(plain), _bits(vf.reshape(plain.shape)))                 # an un-augmented pixel has the bits of today's ingest


# --------------------------------------------------------------------------------------------------- 2. RGB 96 x 96 -> 88
@pytest.mark.parametrize("fill", ["zero", "mean"])
def test_rgb_shipped_geometry_everything_on(fill):
    fr = np.random.default_rng(11).integers(0, 256, size=(2, 3, 3, 96, 96), dtype=np.int64).astype(np.uint8)
    ca = _ca(time_masks=2, time_width=2, time_ratio=0.7, cutouts=2, cut_size=30, fill=fill, mixup_alpha=0.4)
    params = {"draws": _draws(12, 2), "perm": np.array([1, 0], dtype=np.int32), "lam": np.array([0.3], dtype=np.float32)}
    cp = [[5, 3, 1, 0], [2, 7, 0, 0]]                                # odd ox on both rows, a flip on the first
    got, want = _check(ca, fr, [3, 2], params, cp=cp, what=f"rgb/{fill}")
    assert want["mask"].any() and not want["mask"].all() and (got[1, 0, 2] == 0).all()


# ---------------------------------------------------------------------------------------------------------- 3. float source
@pytest.mark.parametrize("fill", ["zero", "mean"])
def test_float_clip_masks_and_mixup(fill):
    ca = _ca(time_masks=2, time_width=2, cutouts=2, cut_size=3, fill=fill, mixup_alpha=1.0)
    params = {"draws": _edge_draws(), "perm": np.array([1, 2, 0], dtype=np.int32), "lam": np.array([0.625], dtype=np.float32)}
    _check(ca, _float_clip(), list(LENS), params, what=f"float/{fill}")
    _check(_ca(time_masks=1, time_width=3, fill=fill), _float_clip(), list(LENS), {"draws": _draws(4)}, what=f"float masks/{fill}")


# ------------------------------------------------------------------------------------------------------------ 4. rows alone
def test_a_row_has_the_same_bits_alone():
    ca = _ca(crop=8, fill="mean", time_masks=2, time_width=2, cutouts=2, cut_size=4)
    d = _draws(21)
    cp = [[1, 3, 1, 0], [4, 1, 0, 0], [0, 2, 1, 0]]
    batch = _run(ca, _gray(), list(LENS), {"draws": d}, cp)
    for b, n in enumerate(LENS):
        alone = _run(ca, _gray()[b:b + 1], [n], {"draws": d[b:b + 1]}, cp[b:b + 1])
        assert np.array_equal(_bits(alone[0]), _bits(batch[b])), b
        short = _run(ca, _gray()[b:b + 1, :n], None, {"draws": d[b:b + 1]}, cp[b:b + 1])          # ... and at T = n without lengths
        assert np.array_equal(_bits(short[0, 0]), _bits(batch[b, 0, :n])), b
    fbatch = _run(ca, _float_clip(), list(LENS), {"draws": d})
    for b, n in enumerate(LENS):
        assert np.array_equal(_bits(_run(ca, _float_clip()[b:b + 1], [n], {"draws": d[b:b + 1]})[0]), _bits(fbatch[b])), b


# ----------------------------------------------------------------------------------------------------------------- 5. mixup
@pytest.mark.parametrize("lam", [0.25, 0.3])
def test_mixup_partners_longer_shorter_and_a_fixed_point(lam):
    masks = dict(crop=8, fill="zero", time_masks=1, time_width=2, cutouts=1, cut_size=4)
    ca = _ca(mixup_alpha=0.4, **masks)
    d = _draws(31)
    perm = np.array([1, 0, 2], dtype=np.int32)                       # row 0 (5 frames) <-> row 1 (3 frames); row 2 is a fixed point
    got, want = _check(ca, _gray(), list(LENS), {"draws": d, "perm": perm, "lam": np.array([lam], dtype=np.float32)}, what=f"mixup {lam}")
    plain = _run(_ca(**masks), _gray(), list(LENS), {"draws": d})
    assert np.array_equal(_bits(got[2]), _bits(plain[2]))                                          # the fixed point is stored unblended
    assert not np.array_equal(got[0, 0, :3], plain[0, 0, :3]) and (got[1, 0, 3:] == 0).all()
    l32 = np.float32(lam)
    assert np.array_equal(_bits(got[0, 0, 3:]), _bits(l32 * plain[0, 0, 3:] + (np.float32(1) - l32) * np.float32(0)))   # the partner has ended
    one = _run(ca, _gray(), list(LENS), {"draws": d, "perm": perm, "lam": np.array([1.0], dtype=np.float32)})
    assert np.array_equal(_bits(one), _bits(plain))                                                # lam = 1: the un-mixed result


# ------------------------------------------------------------------------------------------------------------- 6. footprint
def test_footprint_and_clamped_device_lengths(monkeypatch):
    from deeplip_amd import ops
    ca = _ca(crop=8, fill="mean", time_masks=2, time_width=2, cutouts=2, cut_size=3, mixup_alpha=0.4)
    host = {"draws": _edge_draws(), "perm": np.array([1, 0, 2], dtype=np.int32), "lam": np.array([0.3], dtype=np.float32)}
    wild = torch.tensor([0, T + 5, 3], dtype=torch.int32)            # clamped to 1, T, 3
    outs = []
    for fill in (POISON, ZEROS):
        arena = FenceArena(fill)
        fr = arena.fenced(torch.from_numpy(np.array(_gray())).to(DEV), "frames")
        cp = arena.fenced(torch.tensor([[1, 3, 1, 0], [4, 1, 0, 0], [0, 2, 1, 0]], dtype=torch.int32, device=DEV), "clip_params")
        ln = arena.fenced(wild.to(DEV), "lengths")
        p = {k: arena.fenced(torch.from_numpy(v).to(DEV), k) for k, v in host.items()}
        monkeypatch.setattr(ops, "ARENA", arena)
        try:
            y = ca(fr, clip_params=cp, lengths=ln, params=p)
            torch.cuda.synchronize()
        finally:
            monkeypatch.setattr(ops, "ARENA", None)
        arena.check_all(f"clip_augment, fill {fill:#x}")
        assert len(arena.taken) == 2 and not arena.unwritten(y)      # the workspace and the output; the output is written whole
        outs.append(y.cpu().numpy())
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    want = _ref(ca, _gray(), [1, T, 3], host, cp=[[1, 3, 1, 0], [4, 1, 0, 0], [0, 2, 1, 0]])
    m = want["mask"]
    assert np.array_equal(_bits(outs[0][~m]), _bits(want["y"][~m])) and (np.abs(outs[0][m] - want["y"][m]) <= FILL_BAR).all()


# ------------------------------------------------------------------------------------------------- 7. determinism, the plan
def test_two_calls_agree_and_a_recorded_plan_follows_new_draws_and_lengths():
    from deeplip_amd.plan import StepPlan
    ca = _ca(crop=8, fill="mean", time_masks=2, time_width=2, cutouts=2, cut_size=3, mixup_alpha=0.4)
    cf = _ca(fill="mean", time_masks=1, time_width=3)

    def dev(seed, lens, perm, lam):
        return (torch.from_numpy(np.array(_gray())).to(DEV), torch.from_numpy(np.nan_to_num(_float_clip()) + np.float32(seed)).to(DEV),
                torch.tensor(lens, dtype=torch.int32, device=DEV), torch.from_numpy(_draws(seed)).to(DEV),
                torch.tensor(perm, dtype=torch.int32, device=DEV), torch.tensor([lam], dtype=torch.float32, device=DEV))

    def step(fr, xf, lens, draws, perm, lam):
        return ca(fr, lengths=lens, params={"draws": draws, "perm": perm, "lam": lam}), cf(xf, lengths=lens, params={"draws": draws})

    ins0 = dev(41, [5, 3, 1], [1, 0, 2], 0.3)
    a, b = step(*ins0), step(*ins0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))              # two calls, the same bits
    plan = StepPlan(step, *ins0)
    first = [t.clone() for t in plan.run()]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(first, a))
    ins1 = dev(42, [2, 5, 4], [2, 0, 1], 0.7)
    got = [t.clone() for t in plan(*ins1)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(got, step(*ins1))) and not torch.equal(got[0], first[0])
    print(f"launches in the plan: {plan.launches}")
    assert plan.launches >= 4                                        # a mean pass and a write pass per stage
    plan.close()


# --------------------------------------------------------------------------------------------------------- 8. the mixed loss
def test_mixed_loss_against_torch_and_a_replayed_step_follows_lam():
    import train_video
    from deeplip_amd.train_plan import TrainStepGraph
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(6, 54, generator=g).to(DEV)
    la, lb = torch.randint(0, 54, (6,), generator=g).to(DEV), torch.randint(0, 54, (6,), generator=g).to(DEV)
    lam = torch.tensor([0.3], dtype=torch.float32, device=DEV)

    def want(l):
        x = logits.double().cpu()
        ce = torch.nn.functional.cross_entropy
        return float(l * ce(x, la.cpu()) + (1.0 - l) * ce(x, lb.cpu()))

    def step(lg, a, b, l):
        lg = lg.clone().requires_grad_()
        loss = train_video.mixed_ce_loss(lg, a, b, l)
        loss.backward()
        return loss, lg.grad

    plan = TrainStepGraph(step, eager_steps=1)
    seen = []
    for l in (0.3, 0.3, 0.9, 0.0):                                   # eager, recorded, replayed twice with a new lam in the same tensor
        lam.fill_(l)
        loss, grad = plan.step(logits, la, lb, lam)
        plan.finish()
        loss = loss.detach()
        seen.append((float(loss), plan.recorded))
        print(f"lam {l}: loss {float(loss):.7f},torch fp64 {want(float(np.float32(l))):.7f}")
        assert abs(float(loss) - want(float(np.float32(l)))) <= 2e-5 * max(1.0, abs(want(float(np.float32(l)))))
        x = logits.double().cpu().requires_grad_()
        ce = torch.nn.functional.cross_entropy
        (float(np.float32(l)) * ce(x, la.cpu()) + (1.0 - float(np.float32(l))) * ce(x, lb.cpu())).backward()
        assert float((grad.double().cpu() - x.grad).abs().max()) <= 2e-5 * float(x.grad.abs().max())
    assert [r for _, r in seen] == [False, True, True, True] and seen[0][0] == seen[1][0] and seen[2][0] != seen[1][0]


# ------------------------------------------------------------------------------------------------------------ 9. the trainer
AUG = ["--time-masks", "2", "--time-mask-width", "3", "--time-mask-ratio", "0.5", "--cutouts", "2", "--cutout-size", "30", "--mask-fill", "mean",
       "--mixup-alpha", "0.4"]
OFF = ["--time-masks", "0", "--time-mask-width", "0", "--time-mask-ratio", "1.0", "--cutouts", "0", "--cutout-size", "0", "--mask-fill", "mean",
       "--mixup-alpha", "0"]


@pytest.mark.parametrize("rgb", [False, True])
def test_train_video_main_with_every_augmentation_flag(tmp_path, capsys, rgb):
    import train_video
    argv = ["--save-path", str(tmp_path / "ck"), "--steps", "2", "--frames", "9"] + (["--rgb"] if rgb else [])
    loss, shape = train_video.main(argv + AUG)
    assert np.isfinite(loss) and shape == (4, 54)                    # the logits' shape is unchanged
    out = capsys.readouterr().out
    assert out.count("(replayed)") == 1 and train_video.train.last_plan.summary() == {"shapes": 1, "recorded": 1, "eager_only": []}


def test_train_video_main_with_every_flag_off_is_the_run_without_flags(tmp_path):
    import train_video
    argv = ["--steps", "1", "--frames", "9", "--rgb"]
    plain = train_video.main(["--save-path", str(tmp_path / "a")] + argv)
    off = train_video.main(["--save-path", str(tmp_path / "b")] + argv + OFF)
    assert plain == off and np.isfinite(plain[0])                    # the first step's loss, bit for bit
    on = train_video.main(["--save-path", str(tmp_path / "c")] + argv + AUG[:-2])          # masks and cutout, no mixup: today's criterion
    assert np.isfinite(on[0]) and on[0] != plain[0] and on[1] == (4, 54)
    with pytest.raises(ValueError):
        train_video.main(["--save-path", str(tmp_path / "d")] + argv + AUG + ["--head-only"])
