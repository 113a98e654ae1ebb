"""SpecAugment (deeplip_amd/spec_augment.py), host side (-m "not gpu"): the parser and its refusals, the
length-free draws, the invariants of the definition (tests/spec_augment_ref.py) at every short length with extreme draws, the C ABI
(declared, exported, bound, ABI number unchanged, the refusals in front of any launch), CPU tensors, and the trainer's refusal of a bad
section in front of its GPU requirement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import spec_augment_ref as ref
import test_abi_cpu as abi
from conftest import ROOT

NAMES = ("dlip_spec_augment_f32", "dlip_spec_augment_workspace_bytes")
GOOD = {"time_warp": 5, "freq_masks": 2, "freq_width": 4, "time_masks": 3, "time_width": 20, "time_ratio": 0.2, "fill": "mean"}


# ------------------------------------------------------------------------------------------------------------------ the parser
def test_parser_defaults_and_absent_section():
    from deeplip_amd.spec_augment import SPEC_AUGMENT_KEYS, parse_spec_augment_section
    assert SPEC_AUGMENT_KEYS == ("time_warp", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "fill")
    assert parse_spec_augment_section(None) is None and parse_spec_augment_section(False) is None
    assert parse_spec_augment_section(dict(GOOD)) == GOOD
    got = parse_spec_augment_section({"freq_width": 3, "time_width": 7})
    assert got == {"time_warp": 0, "freq_masks": 2, "freq_width": 3, "time_masks": 2, "time_width": 7, "time_ratio": 1.0, "fill": "zero"}
    assert tuple(got) == SPEC_AUGMENT_KEYS
    # a count of 0 needs no width; the warp alone is a section
    assert parse_spec_augment_section({"freq_masks": 0, "time_width": 5})["freq_width"] == 0
    assert parse_spec_augment_section({"time_warp": 3, "freq_masks": 0, "time_masks": 0})["time_warp"] == 3
    assert parse_spec_augment_section({"freq_masks": 8, "freq_width": 1, "time_masks": 0})["freq_masks"] == 8
    assert parse_spec_augment_section({"freq_width": 1, "time_width": 1, "time_ratio": 1})["time_ratio"] == 1.0


@pytest.mark.parametrize("bad", [
    {"bogus": 1, "freq_width": 1, "time_width": 1},                       # an unknown key
    {"freq_masks": 9, "freq_width": 1, "time_width": 1},                  # counts outside [0, 8]
    {"time_masks": 9, "freq_width": 1, "time_width": 1},
    {"freq_masks": -1, "freq_width": 1, "time_width": 1},
    {"time_masks": 1.5, "freq_width": 1, "time_width": 1},
    {"freq_masks": True, "freq_width": 1, "time_width": 1},
    {"freq_width": -1, "time_width": 1},                                  # negative widths, a negative warp
    {"freq_width": 1, "time_width": -4},
    {"time_warp": -1, "freq_width": 1, "time_width": 1},
    {"freq_width": 1, "time_width": 1, "time_ratio": 1.5},                # a ratio outside [0, 1]
    {"freq_width": 1, "time_width": 1, "time_ratio": -0.1},
    {"freq_width": 1, "time_width": 1, "time_ratio": float("nan")},
    {"freq_width": 1, "time_width": 1, "time_ratio": "half"},
    {"freq_width": 1, "time_width": 1, "fill": "noise"},                  # a fill other than zero / mean
    {"freq_width": 1, "time_width": 1, "fill": 0},
    {"time_width": 1},                                                    # a width that is required (2 masks by default)
    {"freq_width": 1},
    {},
    {"freq_masks": 0, "time_masks": 0},                                   # sections that would do nothing
    {"freq_width": 0, "time_width": 0},
    {"freq_masks": 0, "time_width": 5, "time_ratio": 0.0},
    ["freq_width", 1], "on", 3,                                           # not a mapping
])
def test_parser_refusals(bad):
    from deeplip_amd.spec_augment import parse_spec_augment_section
    with pytest.raises(ValueError, match="spec_augment"):
        parse_spec_augment_section(bad)


def test_module_refusals():
    from deeplip_amd.spec_augment import SpecAugment
    for kw in (dict(freq_masks=9, freq_width=1), dict(time_masks=-1, freq_width=1), dict(freq_width=-1), dict(time_warp=-2),
               dict(freq_width=1, time_ratio=2.0), dict(freq_width=1, fill="median"), dict(), dict(freq_masks=0, time_masks=0)):
        with pytest.raises(ValueError, match="SpecAugment"):
            SpecAugment(device="cpu", **kw)
    sa = SpecAugment(device="cpu", **GOOD)
    assert (sa.time_warp, sa.freq_masks, sa.freq_width, sa.time_masks, sa.time_width, sa.time_ratio, sa.fill) == (5, 2, 4, 3, 20, 0.2, "mean")


# ------------------------------------------------------------------------------------------------------------------ the draws
def test_draw_is_reproducible_length_free_and_31_bit():
    from deeplip_amd import _lib
    from deeplip_amd.spec_augment import DRAWS, MAX_MASKS, SpecAugment
    assert MAX_MASKS == _lib.HEADER["DLIP_SPECAUG_MAX_MASKS"] == ref.MAX_MASKS == 8
    assert DRAWS == _lib.HEADER["DLIP_SPECAUG_DRAWS"] == ref.DRAWS == 2 + 4 * MAX_MASKS
    sa = SpecAugment(device="cpu", **GOOD)
    a = sa.draw(257, np.random.default_rng(7))
    b = sa.draw(257, np.random.default_rng(7))
    assert sorted(a) == ["draws"] and a["draws"].dtype == np.int32 and a["draws"].shape == (257, DRAWS)
    assert np.array_equal(a["draws"], b["draws"]) and not np.array_equal(a["draws"], sa.draw(257, np.random.default_rng(8))["draws"])
    assert a["draws"].min() >= 0 and int(a["draws"].max()) < 2 ** 31
    assert a["draws"].max() > 2 ** 30 and a["draws"].min() < 2 ** 28          # the whole range is drawn from
    # what the draw consumes of the generator does not depend on the module's settings
    other = SpecAugment(device="cpu", time_warp=80).draw(257, np.random.default_rng(7))
    assert np.array_equal(a["draws"], other["draws"])


# ------------------------------------------------------------------------------------------------------------------ the definition
def test_pick():
    for m in (1, 2, 3, 7, 1000, 2 ** 31 - 1):
        assert ref.pick(0, m) == 0 and ref.pick(ref.TOP, m) == m - 1 and ref.pick(-5, m) == 0
    assert [ref.pick(r, 4) for r in (0, 2 ** 29 - 1, 2 ** 29, 2 ** 30, 3 * 2 ** 29, ref.TOP)] == [0, 0, 1, 2, 3, 3]


def test_invariants_at_short_lengths_with_extreme_draws():
    """n = 1 .. 40, W in {1, 2, 5, 40, 1000}, every pair of extreme draws: c and c' in range, s strictly increasing with fixed ends and
    s(c') = c, masks inside the row, no mask wider than its cap."""
    for n in range(1, 41):
        for W in (1, 2, 5, 40, 1000):
            for r0 in (0, ref.TOP):
                for r1 in (0, ref.TOP):
                    wp = ref.warp_params(n, W, r0, r1)
                    if n < 5:
                        assert wp is None                   # the first length that warps is 5
                        continue
                    c, cp = wp
                    We = min(W, (n - 3) // 2)
                    assert 1 <= c <= n - 2 and 1 <= cp <= n - 2 and abs(cp - c) <= We, (n, W, r0, r1)
                    s = ref.warp_positions(n, c, cp)
                    assert s[0] == 0.0 and s[n - 1] == float(n - 1) and s[cp] == float(c)
                    assert (np.diff(s) > 0).all() and s.min() >= 0 and s.max() <= n - 1
        for C in (1, 5, 24):
            for width in (0, 1, 3, 1000):
                for ratio in (0.0, 0.2, 1.0):
                    for lo in (0, ref.TOP):
                        for hi in (0, ref.TOP):
                            row = [0, 0] + [lo, hi] * (2 * ref.MAX_MASKS)
                            for f0, w in ref.freq_masks(C, row, ref.MAX_MASKS, width):
                                assert 0 <= w <= min(width, C) and 0 <= f0 and f0 + w <= C
                            cap = ref.time_cap(n, width, ratio)
                            assert cap == min(width, int(np.floor(ratio * n))) and cap <= n
                            for t0, w in ref.time_masks(n, row, ref.MAX_MASKS, width, ratio):
                                assert 0 <= w <= cap and 0 <= t0 and t0 + w <= n
                            if lo == ref.TOP:               # the widest draw reaches the cap
                                assert ref.time_masks(n, row, 1, width, ratio)[0][1] == cap


def test_reference_on_a_case_done_by_hand():
    """n = 5, W = 1: We = 1, c = 2 + pick(r0, 1) = 2, d = pick(r1, 3) - 1.  r1 = TOP: d = 1, c' = 3: s = t 2/3 up to 3, then 2 + (t - 3) 2.
    One frequency mask of width 1 at feature 1 (of 2), one time mask of width 1 at frame 4 -- fill: the mean of the input."""
    x = np.array([[[0.0, 3.0, 6.0, 9.0, 12.0], [1.0, 1.0, 1.0, 1.0, 1.0]]], dtype=np.float32)
    row = np.zeros((1, ref.DRAWS), dtype=np.int64)
    row[0, 1] = ref.TOP
    out = ref.spec_augment(x, None, row, warp=1)
    assert np.abs(out["y"][0, 0] - [0.0, 2.0, 4.0, 6.0, 12.0]).max() <= 1e-14 and not out["mask"].any()
    assert out["y"][0, 0, [0, 3, 4]].tolist() == [0.0, 6.0, 12.0] and out["y"][0, 1].tolist() == [1.0] * 5
    assert out["interp"][0, 0].tolist() == [False, True, True, False, False]
    assert out["scale"][0, 0].tolist() == [0.0, 3.0, 6.0, 0.0, 0.0]
    row[0, 2], row[0, 3] = ref.TOP, ref.TOP                 # frequency mask 0: w = pick(TOP, 2) = 1, f0 = pick(TOP, 2) = 1
    row[0, 18], row[0, 19] = ref.TOP, ref.TOP               # time mask 0: cap = 1, w = 1, t0 = pick(TOP, 5) = 4
    out = ref.spec_augment(x, None, row, warp=1, n_freq=1, freq_width=1, n_time=1, time_width=1, fill=1)
    assert out["mean"][0] == 3.5
    assert np.abs(out["y"][0] - [[0.0, 2.0, 4.0, 6.0, 3.5], [3.5] * 5]).max() <= 1e-14 and out["mask"][0].sum() == 6
    short = ref.spec_augment(x, [3], row, warp=1, n_freq=0, n_time=1, time_width=9, time_ratio=0.5)    # n = 3: no warp, cap = 1, t0 = 2
    assert short["y"][0].tolist() == [[0.0, 3.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0, 0.0]]


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from deeplip_amd import _lib, build
    assert "spec_augment_ops.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.HEADER["DLIP_ABI_VERSION"] == _lib.ABI_VERSION == 67       # a pure addition: no bump
    for n in NAMES:
        assert n in abi.header_symbols() and hasattr(lib, n) and n in _lib.SIGNATURES, n
    VP, I32, I64, F64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert _lib.PROTOTYPES["dlip_spec_augment_workspace_bytes"] == (I64, [I32] * 3)
    assert _lib.PROTOTYPES["dlip_spec_augment_f32"] == (ctypes.c_int, [VP] * 5 + [I64] + [I32] * 8 + [F64, I32, VP])
    with open(os.path.join(ROOT, "include", "deeplip_hip.h")) as f:
        assert "(ABI 67, added) SPECAUGMENT" in f.read()


def test_workspace_bytes_and_the_launch_refuse_on_the_host():
    """The size query and every DLIP_EINVAL of the launch (dummy addresses, nothing dereferenced, no launch)."""
    from deeplip_amd import _lib
    l = _lib.lib()
    EINVAL = _lib.HEADER["DLIP_EINVAL"]
    for B, C, NF in ((1, 1, 1), (6, 5, 1031), (256, 80, 3000), (65535, 257, 302)):
        assert l.dlip_spec_augment_workspace_bytes(B, C, NF) >= 8 * B
    for B, C, NF in ((0, 5, 10), (5, 0, 10), (5, 5, 0), (-1, 5, 10), (65536, 5, 10), (5, 5, 2 ** 31 - 1)):
        assert l.dlip_spec_augment_workspace_bytes(B, C, NF) < 0, (B, C, NF)
    need = l.dlip_spec_augment_workspace_bytes(2, 5, 100)
    p, q, w = 4096, 8192, 16384

    def launch(**kw):
        a = dict(x=p, lens=None, draws=p, y=q, ws=w, wsb=need, B=2, C=5, NF=100, warp=5, nf=2, fw=3, nt=2, tw=10, ratio=1.0, fill=0)
        a.update(kw)
        return l.dlip_spec_augment_f32(a["x"], a["lens"], a["draws"], a["y"], a["ws"], a["wsb"], a["B"], a["C"], a["NF"], a["warp"], a["nf"],
                                       a["fw"], a["nt"], a["tw"], a["ratio"], a["fill"], None)
    for kw in (dict(B=0), dict(C=0), dict(NF=0), dict(B=65536), dict(warp=-1), dict(fw=-1), dict(tw=-1), dict(nf=-1), dict(nf=9),
               dict(nt=-1), dict(nt=9), dict(ratio=-0.5), dict(ratio=1.25), dict(ratio=float("nan")), dict(fill=2), dict(fill=-1),
               dict(y=p), dict(x=None), dict(y=None), dict(draws=None), dict(ws=None), dict(ws=w + 4), dict(wsb=need - 1), dict(wsb=0)):
        assert launch(**kw) == EINVAL, kw


def test_cpu_tensors_are_refused():
    from deeplip_amd import _lib
    from deeplip_amd.spec_augment import DRAWS, SpecAugment
    sa = SpecAugment(device="cpu", **GOOD)
    with pytest.raises(_lib.DeepLipHipError, match="no CPU path"):
        sa(torch.zeros(2, 5, 100), params={"draws": np.zeros((2, DRAWS), dtype=np.int32)})
    with pytest.raises(_lib.DeepLipHipError, match="no CPU path"):
        sa(torch.zeros(2, 1, 5, 100))


# ------------------------------------------------------------------------------------------------------------------ the trainer
def test_trainer_refuses_a_bad_section_before_its_gpu_requirement():
    import train_audio
    for bad in ({"bogus": 1}, {"freq_masks": 9, "freq_width": 1, "time_width": 1}, {"freq_width": 1, "time_width": 1, "fill": "noise"},
                {"freq_masks": 0, "time_masks": 0}):
        for extra in ({}, {"data.train_from_waves": True}):               # both paths read the section
            with pytest.raises(ValueError, match="spec_augment"):
                train_audio.Trainer(overrides=dict({"data.spec_augment": bad}, **extra))
    assert train_audio.parse_spec_augment({}) is None and train_audio.parse_spec_augment({"spec_augment": None}) is None
    assert train_audio.parse_spec_augment({"spec_augment": dict(GOOD)}) == GOOD          # no train_from_waves needed
    # the sibling parsers keep their results beside the new key
    assert train_audio.parse_wave_training({"spec_augment": dict(GOOD)}) == (False, None)
    assert train_audio.parse_speed_perturb({"spec_augment": dict(GOOD)}) is None


def test_the_shipped_config_does_not_name_the_key():
    import yaml
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        text = f.read()
    assert "spec_augment" not in yaml.safe_load(text)["data"] and "spec_augment" in text          # documented in a comment only
