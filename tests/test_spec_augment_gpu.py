"""SpecAugment on the device (-m gpu; deeplip_amd/spec_augment.py): the kernel against the definition in numpy
(tests/spec_augment_ref.py) -- the masks bit for bit, the warp within its derived rounding bound, the mean fill, a row's bits whatever
the batch, the width, the alignment and the rank of the tensor are, device lengths (clamped), a recorded plan, and train_audio's
``data.spec_augment`` on both of its paths.

Geometry: B = 6 rows of C = 5 (also 1 and 24) features padded to NF = 1031 frames -- odd, so no row is 16-byte aligned, and past the
edge of the kernel's tiles (256 frames at 4-byte accesses, 1024 at 16-byte ones) -- holding 1031, 1, 2, 4, 5 (the first length that
warps) and 1025 frames; the padding is NaN, which the kernel must never load.  The 16-byte path runs where NF % 4 == 0: the same batch
padded to 1032 frames, and the rows alone at NF = n = 4."""
import functools

import numpy as np
import pytest
import torch

import spec_augment_ref as ref
from test_models_gpu import DEV, tdnn_opts

pytestmark = pytest.mark.gpu

B, NF = 6, 1031
LENS = (1031, 1, 2, 4, 5, 1025)
EPS = 2.0 ** -24
MID = 2 ** 30                        # the draw that gives d = 0: pick(2^30, 2 We + 1) = We


def _sa(**kw):
    from deeplip_amd.spec_augment import SpecAugment
    return SpecAugment(**kw)


@functools.lru_cache(maxsize=None)
def _x(C, offset=0.0):
    """The batch on the host: N(offset, 1) in the rows, NaN behind them.  Read-only, shared."""
    g = np.random.default_rng(1000 + C)
    x = np.full((B, C, NF), np.nan, dtype=np.float32)
    for b, n in enumerate(LENS):
        x[b, :, :n] = (g.standard_normal((C, n)) + offset).astype(np.float32)
    x.setflags(write=False)
    return x


def _draws(seed):
    return np.random.default_rng(seed).integers(0, 2 ** 31, size=(B, ref.DRAWS), dtype=np.int64).astype(np.int32)


def _run(sa, x, lens, draws):
    y = sa(torch.from_numpy(np.array(x, dtype=np.float32)).to(DEV), lens, params={"draws": np.ascontiguousarray(draws)})
    return y.cpu().numpy()


def _ref(sa, x, lens, draws):
    return ref.spec_augment(x, lens, draws, warp=sa.time_warp, n_freq=sa.freq_masks, freq_width=sa.freq_width, n_time=sa.time_masks,
                            time_width=sa.time_width, time_ratio=sa.time_ratio, fill=("zero", "mean").index(sa.fill))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


# --------------------------------------------------------------------------------------------------------------- 1. masks only
MASK_CASES = {
    "2+2, C=5": (5, dict(freq_masks=2, freq_width=2, time_masks=2, time_width=40)),
    "8+8, C=24, ratio 0.2": (24, dict(freq_masks=8, freq_width=3, time_masks=8, time_width=30, time_ratio=0.2)),
    "C=1": (1, dict(freq_masks=1, freq_width=1, time_masks=3, time_width=100)),
    "wide caps": (5, dict(freq_masks=3, freq_width=1000, time_masks=2, time_width=5000)),
    "time only": (5, dict(freq_masks=0, time_masks=4, time_width=64, time_ratio=0.5)),
}


@pytest.mark.parametrize("name", list(MASK_CASES))
def test_masks_are_the_definitions_bit_for_bit(name):
    C, kw = MASK_CASES[name]
    sa = _sa(**kw)
    x = _x(C)
    for seed, edit in ((1, None), (2, "zero widths"), (3, "whole row"), (4, "negative")):
        d = _draws(seed)
        if edit == "zero widths":           # a width draw of 0 is a mask of no entries
            d[:, 2:2 + 4 * ref.MAX_MASKS:2] = np.where(np.arange(2 * ref.MAX_MASKS) % 2 == 0, 0, d[:, 2:2 + 4 * ref.MAX_MASKS:2])
        if edit == "whole row":             # the widest draw: a time mask as wide as its cap (the whole row at ratio 1 and a wide cap)
            d[:, 2 + 2 * ref.MAX_MASKS] = ref.TOP
        if edit == "negative":              # negative draws count as 0
            d[0::2, 3::4] = -5
            d[1::2, 2::4] = np.iinfo(np.int32).min
        got, want = _run(sa, x, list(LENS), d), _ref(sa, x, LENS, d)
        assert _same_bits(got, want["y"]), (name, edit)                  # every element, the zeros of the padding included
        assert not np.isnan(got).any() and (got[~want["mask"] & np.isfinite(x)] == x[~want["mask"] & np.isfinite(x)]).all()
        if edit == "whole row" and sa.time_ratio == 1.0 and sa.time_width >= NF:
            assert want["mask"][0].all() and (got == 0).all()            # (every row is masked from end to end)
        if edit is None:
            assert want["mask"][0].any()


def test_masks_on_the_16_byte_path():
    """NF % 4 == 0: 16-byte accesses, 1028 = one access past a 1024-frame tile.  Same definition, same bits."""
    sa = _sa(freq_masks=2, freq_width=2, time_masks=2, time_width=40)
    x = np.ascontiguousarray(_x(5)[:, :, :1028])
    lens = [min(n, 1028) for n in LENS]
    d = _draws(5)
    assert _same_bits(_run(sa, x, lens, d), _ref(sa, x, lens, d)["y"])


# --------------------------------------------------------------------------------------------------------------------- 2. the warp
@pytest.mark.parametrize("W,C,masks", [(5, 5, False), (80, 5, False), (1000, 1, False), (5, 24, True)])
def test_warp_within_the_rounding_bound(W, C, masks):
    """|y - y64| <= 4 * 2^-24 * max(|x[f, i]|, |x[f, i + 1]|) per interpolated entry: one fp32 rounding of the difference (2 * 2^-24 of
    the larger sample at most), a <= 1, one rounding of the fma.  Every other entry holds its source's bits.  (The rounding of a itself
    to fp32 is not counted in the 4; with it the worst case is 5.  Largest fractions of the bound measured on an MI355X: 0.656, 0.802,
    0.717, 0.771 for the four cases.)"""
    sa = _sa(time_warp=W, **(dict(freq_masks=2, freq_width=3, time_masks=2, time_width=50) if masks else dict(freq_masks=0, time_masks=0)))
    x = _x(C)
    worst = 0.0
    for seed, still in ((11, ()), (12, (0,)), (13, (0, 4, 5))):
        d = _draws(seed)
        for b in range(B):                                               # d == 0: the row is left as it is; else d = -We or +We
            d[b, 1] = MID if b in still else (0, ref.TOP)[(seed + b) % 2]
        got, want = _run(sa, x, list(LENS), d), _ref(sa, x, LENS, d)
        it = want["interp"]
        assert _same_bits(got[~it], want["y"][~it]), (W, seed)           # copies, masked entries, the padding: exact
        err = np.abs(got[it].astype(np.float64) - want["y"][it])
        bound = 4 * EPS * want["scale"][it]
        assert (err <= bound).all(), (W, seed, float((err / bound).max()))
        if it.any():
            worst = max(worst, float((err / bound).max()))
        for b, n in enumerate(LENS):
            wp = ref.warp_params(n, W, d[b, 0], d[b, 1])
            moved = wp is not None and wp[0] != wp[1]
            assert moved == (n >= 5 and b not in still), (b, n)
            if masks:
                continue
            assert _same_bits(got[b, :, [0, n - 1]], x[b, :, [0, n - 1]])                # frames 0 and n - 1 stay in place
            if moved:
                assert it[b].any() and _same_bits(got[b, :, wp[1]], x[b, :, wp[0]])        # s(c') = c
                assert n < 100 or not _same_bits(got[b, :, :n], x[b, :, :n])
            else:
                assert _same_bits(got[b, :, :n], x[b, :, :n])            # rows with d == 0 and rows of n < 5: bit for bit
        assert (got[:, :, 1:][np.isnan(x[:, :, 1:])] == 0).all()
    print(f"warp W = {W}, C = {C}: largest fraction of the bound {worst:.3f}")
    assert worst > 0


# ---------------------------------------------------------------------------------------------------------------- 3. fill: mean
@pytest.mark.parametrize("C", [5, 24])
def test_fill_mean(C):
    sa = _sa(freq_masks=2, freq_width=2, time_masks=2, time_width=60, fill="mean")
    x = _x(C, offset=0.75)
    d = _draws(21)
    d[1, 2 + 2 * ref.MAX_MASKS] = ref.TOP                                # the one-frame row is masked whole: its fill is its own mean
    got, want = _run(sa, x, list(LENS), d), _ref(sa, x, LENS, d)
    m = want["mask"]
    assert _same_bits(got[~m], want["y"][~m])                            # unmasked entries and the padding: as with fill zero
    for b, n in enumerate(LENS):
        vals = got[b][m[b]]
        if b in (0, 1, 5):
            assert vals.size > 0
        if vals.size == 0:
            continue
        assert (vals.view(np.uint32) == vals.view(np.uint32)[0]).all(), b         # one value, the same bits everywhere
        m32 = np.float32(want["mean"][b])
        assert abs(np.float64(vals[0]) - np.float64(m32)) <= np.spacing(np.abs(m32)), (b, vals[0], m32)
        assert vals[0] != 0


# ---------------------------------------------------------------------------------------------------------------- 4. a row alone
def test_a_row_has_the_same_bits_alone_at_another_width_alignment_and_rank():
    for kw in (dict(time_warp=5, freq_masks=2, freq_width=2, time_masks=2, time_width=40, fill="mean"),
               dict(time_warp=80, freq_masks=0, time_masks=1, time_width=30, time_ratio=0.3)):
        sa = _sa(**kw)
        x = _x(5, offset=0.25)
        d = _draws(31)
        batch = _run(sa, x, list(LENS), d)
        for b, n in enumerate(LENS):                                     # a batch of one at NF = n (n = 4: the 16-byte path)
            alone = _run(sa, x[b:b + 1, :, :n], None, d[b:b + 1])
            assert alone.shape == (1, 5, n) and _same_bits(alone[0], batch[b, :, :n]), (b, n)
        # the 16-byte path at full size: the batch padded to 1032 frames
        xp = np.concatenate([x, np.full((B, 5, 1), np.nan, dtype=np.float32)], axis=2)
        wide = _run(sa, xp, list(LENS), d)
        assert _same_bits(wide[:, :, :NF], batch) and (wide[:, :, NF] == 0).all()
        # full lengths = no lengths; [B, 1, F, T] = [B, F, T]
        full = np.random.default_rng(32).standard_normal((B, 5, NF)).astype(np.float32)
        xf = torch.from_numpy(full).to(DEV)
        p = {"draws": d}
        none = sa(xf, None, params=p)
        assert torch.equal(sa(xf, torch.full((B,), NF, dtype=torch.int32, device=DEV), params=p), none)
        assert torch.equal(sa(xf, [NF] * B, params=p), none)
        four = sa(xf.view(B, 1, 5, NF), None, params=p)
        assert four.shape == (B, 1, 5, NF) and torch.equal(four.view(B, 5, NF), none)


# ------------------------------------------------------------------------------------------ 5. device lengths and the step plan
def test_device_lengths_are_clamped_and_a_recorded_plan_follows_new_inputs():
    from deeplip_amd.plan import StepPlan
    sa = _sa(time_warp=5, freq_masks=2, freq_width=2, time_masks=2, time_width=40, fill="mean")
    sz = _sa(freq_masks=8, freq_width=1, time_masks=8, time_width=25)
    x0 = torch.from_numpy(np.array(_x(5))).to(DEV)
    d0 = torch.from_numpy(_draws(41)).to(DEV)
    wild = torch.tensor([NF + 7, 0, 2, 4, 5, 1025], dtype=torch.int32, device=DEV)
    want = sa(x0, list(LENS), params={"draws": d0})
    assert torch.equal(sa(x0, wild, params={"draws": d0}), want) and not torch.isnan(want).any()

    def step(x, lens, draws):
        return sa(x, lens, params={"draws": draws}), sz(x, lens, params={"draws": draws})

    ins0 = (x0, torch.tensor(LENS, dtype=torch.int32, device=DEV), d0)
    plan = StepPlan(step, *ins0)
    first = [t.clone() for t in plan.run()]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, step(*ins0)))
    lens1 = [5, 1031, 700, 1, 1025, 300]
    x1 = np.full((B, 5, NF), np.nan, dtype=np.float32)
    for b, n in enumerate(lens1):
        x1[b, :, :n] = np.random.default_rng(50 + b).standard_normal((5, n))
    ins1 = (torch.from_numpy(x1).to(DEV), torch.tensor(lens1, dtype=torch.int32, device=DEV), torch.from_numpy(_draws(42)).to(DEV))
    got = [t.clone() for t in plan(*ins1)]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, step(*ins1))) and not torch.equal(got[0], first[0])
    assert _same_bits(got[1].cpu().numpy(), _ref(sz, x1, lens1, _draws(42))["y"])
    print(f"launches in the plan: {plan.launches}")
    plan.close()


# ----------------------------------------------------------------------------------------------------------------- 6. the trainer
SMALL = {"data.n_spk": 6, "data.utt_per_spk": 4, "data.audio_frames": 60, "data.test_speakers": 2, "data.test_utt_per_spk": 2,
         "model.arch": "tdnn", "model.tdnn": tdnn_opts()["tdnn"], "train.bs": 8, "train.steps_per_epoch": 2, "train.crop_frames": [40, 40]}
SPEC = {"time_warp": 5, "freq_masks": 2, "freq_width": 4, "time_masks": 2, "time_width": 10, "time_ratio": 0.5, "fill": "mean"}


def _epoch(overrides):
    import train_audio
    torch.manual_seed(0)                    # the criterion's weights come from torch's generator (nn.init in LMCL)
    tr = train_audio.Trainer("conf/audio_config.yaml", overrides=dict(SMALL, **overrides))
    try:
        tr.current_epoch = 1
        tr._adjust_margin()
        loss = tr._train_epoch()
        return loss, dict(tr.last_epoch_stats)
    finally:
        tr.close()


def test_train_audio_with_spec_augment(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plain, st_plain = _epoch({})
    again, st_again = _epoch({"data.spec_augment": None})              # an absent and an empty section: one path, one random stream
    assert plain == again and np.isfinite(plain) and "spec_augment" not in st_plain and "spec_augment" not in st_again
    for extra in ({}, {"data.train_from_waves": True}):
        loss, st = _epoch(dict({"data.spec_augment": dict(SPEC)}, **extra))
        assert np.isfinite(loss) and np.isfinite(st["loss"]) and loss != plain
        assert st["step_mode"] == st_plain["step_mode"] == "graph", st["step_mode"]      # the recorded step sees the same [B, F, T]
        assert st["spec_augment"] == SPEC and st.get("from_waves", False) is bool(extra)
        assert st["crop_ladder"] == st_plain["crop_ladder"] == [40]
