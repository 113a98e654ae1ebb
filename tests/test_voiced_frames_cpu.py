"""Sliding-window CMN and energy-VAD frame selection, host side (no GPU): the window rule against hand-typed cases, the config
section, the ABI 62 entry points and their refusals, the trainers' refusals in front of their GPU requirement."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

import test_abi_cpu as abi
from conftest import ROOT

NAMES = ("dlip_vad_energy_select_i32", "dlip_cmn_sliding_select_f32")
ARITY = {"dlip_vad_energy_select_i32": 15, "dlip_cmn_sliding_select_f32": 13}


# ------------------------------------------------------------------------------------------------------------ the window rule
def test_window_bounds_centred_300_of_1000():
    from deeplip_amd.voiced_frames import window_bounds as wb
    want = {0: (0, 300), 149: (0, 300), 150: (0, 300), 151: (1, 301), 849: (699, 999), 850: (700, 1000), 999: (700, 1000)}
    for t, be in want.items():
        assert wb(t, 1000, 300) == be, t
    assert wb(500, 1000, 300) == (350, 650)
    assert wb(851, 1000, 300) == (700, 1000)                       # shifted, not shrunk, at the end


def test_window_bounds_short_utterances_and_small_windows():
    from deeplip_amd.voiced_frames import window_bounds as wb
    for t in (0, 57, 119):                                          # n < window: the whole utterance, for every frame
        assert wb(t, 120, 300) == (0, 120)
    for t in (0, 150, 299):                                         # n == window
        assert wb(t, 300, 300) == (0, 300)
    assert [wb(t, 301, 300) for t in (0, 150, 151, 300)] == [(0, 300), (0, 300), (1, 301), (1, 301)]      # n == window + 1
    assert [wb(t, 20, 7) for t in (0, 2, 3, 4, 10, 16, 17, 19)] == [(0, 7), (0, 7), (0, 7), (1, 8), (7, 14), (13, 20), (13, 20), (13, 20)]
    assert [wb(t, 5, 1) for t in range(5)] == [(t, t + 1) for t in range(5)]                              # window 1: the frame itself
    assert wb(0, 1, 300) == (0, 1) and wb(0, 1, 1) == (0, 1)


def test_window_bounds_not_centred():
    from deeplip_amd.voiced_frames import window_bounds as wb
    # the window ends behind t; below min_window frames of history it reaches forward to min_window
    assert wb(0, 1000, 300, center=False, min_window=100) == (0, 100)
    assert wb(50, 1000, 300, center=False, min_window=100) == (0, 100)
    assert wb(99, 1000, 300, center=False, min_window=100) == (0, 100)
    assert wb(100, 1000, 300, center=False, min_window=100) == (0, 101)
    assert wb(299, 1000, 300, center=False, min_window=100) == (0, 300)
    assert wb(300, 1000, 300, center=False, min_window=100) == (0, 301)      # begin = t - window: window + 1 frames
    assert wb(301, 1000, 300, center=False, min_window=100) == (1, 302)
    assert wb(999, 1000, 300, center=False, min_window=100) == (699, 1000)
    assert wb(10, 40, 300, center=False, min_window=100) == (0, 40)          # min_window beyond the utterance: all of it
    assert wb(3, 40, 300, center=False, min_window=1) == (0, 4)


def test_window_bounds_hold_their_invariants():
    """0 <= begin <= t < end <= n, and neither bound ever decreases with t (what the kernel relies on when it sizes a tile's LDS image
    from the first frame's begin and the last frame's end)."""
    from deeplip_amd.voiced_frames import window_bounds as wb
    for n in (1, 2, 6, 7, 8, 50):
        for window in (1, 2, 7, 8, 300):
            for center, mw in ((True, 100), (False, 1), (False, 5), (False, 100)):
                prev = (0, 0)
                for t in range(n):
                    b, e = wb(t, n, window, center, mw)
                    assert 0 <= b <= t < e <= n and b >= prev[0] and e >= prev[1], (n, window, center, mw, t)
                    prev = (b, e)


# ------------------------------------------------------------------------------------------------------------ the section
def test_section_parsing():
    from deeplip_amd import _lib
    from deeplip_amd.voiced_frames import VAD_DEFAULTS, parse_voiced_frames_section as parse
    assert parse(None) is None and parse(False) is None
    assert VAD_DEFAULTS == {"energy_threshold": 5.5, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12}
    assert parse({}) == {"cmn_window": 300, "center": True, "min_window": 100, "norm_vars": False, "vad": VAD_DEFAULTS, "energy_row": 0,
                         "min_keep": None}
    got = parse({"cmn_window": None, "vad": {"frames_context": 0, "proportion_threshold": 0.6}, "min_keep": 24, "energy_row": 3})
    assert got["cmn_window"] is None and got["min_keep"] == 24 and got["energy_row"] == 3
    assert got["vad"] == dict(VAD_DEFAULTS, frames_context=0, proportion_threshold=0.6)
    assert parse({"vad": None, "cmn_window": 600, "center": False, "norm_vars": True})["vad"] is None
    assert _lib.DLIP_CMN_MAX_WINDOW >= 600 and parse({"cmn_window": _lib.DLIP_CMN_MAX_WINDOW})["cmn_window"] == _lib.DLIP_CMN_MAX_WINDOW
    bad = [{"window": 300}, {"cmn_window": 0}, {"cmn_window": _lib.DLIP_CMN_MAX_WINDOW + 1}, {"cmn_window": 2.5}, {"min_window": 0},
           {"vad": {"proportion_threshold": 1.5}}, {"vad": {"proportion_threshold": -0.1}}, {"vad": {"frames_context": -1}},
           {"vad": {"context": 2}}, {"vad": [1]}, {"cmn_window": None, "vad": None}, {"min_keep": 0}, {"energy_row": -1}, [300]]
    for b in bad:
        with pytest.raises(ValueError):
            parse(b)


def test_the_stage_refuses_both_halves_off_and_cpu_tensors():
    from deeplip_amd._lib import DeepLipHipError
    from deeplip_amd.voiced_frames import VoicedFrames
    with pytest.raises(ValueError):
        VoicedFrames(cmn_window=None, vad=None)
    vf = VoicedFrames()
    assert vf.cmn_window == 300 and vf.vad["energy_threshold"] == 5.5 and vf.min_keep == 1 and vf.last_fallback is None
    with pytest.raises(DeepLipHipError):
        vf(torch.zeros(2, 24, 10))
    with pytest.raises(DeepLipHipError):
        VoicedFrames(vad=None)(torch.zeros(2, 24, 10), [10, 4])


def test_shipped_configs_carry_no_voiced_frames_key():
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        a = yaml.safe_load(f)
    with open(os.path.join(ROOT, "conf", "fusion_config.yaml")) as f:
        fu = yaml.safe_load(f)
    assert "voiced_frames" not in a["data"] and "voiced_frames" not in (fu["data"].get("python_data_config") or {})


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from deeplip_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.HEADER["DLIP_ABI_VERSION"] == _lib.ABI_VERSION >= 62
    for n in NAMES:
        assert n in abi.header_symbols() and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[n]) == ARITY[n], n
        assert _lib.PROTOTYPES[n][0] is ctypes.c_int, n
    assert _lib.HEADER["DLIP_CMN_TILE"] == _lib.DLIP_CMN_TILE and _lib.DLIP_CMN_TILE % 256 == 0
    VP, I32 = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SIGNATURES["dlip_vad_energy_select_i32"] == [VP, ctypes.c_int64, VP, VP, ctypes.c_double, ctypes.c_double, I32,
                                                            ctypes.c_float, I32, VP, VP, VP, I32, I32, VP]
    assert _lib.SIGNATURES["dlip_cmn_sliding_select_f32"] == [VP] * 5 + [I32] * 7 + [VP]


def test_refuses_bad_arguments_on_the_host():
    """Every refusal returns DLIP_EINVAL in front of any device call: dummy addresses, nothing dereferenced, no launch."""
    from deeplip_amd import _lib
    l = _lib.lib()
    EINVAL = _lib.HEADER["DLIP_EINVAL"]
    p, q = 4096, 8192

    def vad(**kw):
        a = dict(e=p, stride=72, voiced=None, lens=None, thr=5.5, scale=0.5, ctx=2, prop=0.12, keep=1, pos=p, ol=p, fb=p, B=2, NF=12)
        a.update(kw)
        return l.dlip_vad_energy_select_i32(a["e"], a["stride"], a["voiced"], a["lens"], a["thr"], a["scale"], a["ctx"], a["prop"], a["keep"],
                                            a["pos"], a["ol"], a["fb"], a["B"], a["NF"], None)

    def cmn(**kw):
        a = dict(x=p, lens=None, pos=None, ol=None, y=q, B=2, C=3, NF=12, window=300, center=1, mw=100, nv=0)
        a.update(kw)
        return l.dlip_cmn_sliding_select_f32(a["x"], a["lens"], a["pos"], a["ol"], a["y"], a["B"], a["C"], a["NF"], a["window"], a["center"],
                                             a["mw"], a["nv"], None)
    for kw in (dict(ctx=-1), dict(keep=0), dict(keep=-3), dict(prop=1.5), dict(prop=-0.5), dict(prop=float("nan")), dict(B=0), dict(NF=0),
               dict(e=None), dict(pos=None), dict(ol=None), dict(fb=None), dict(stride=11), dict(thr=float("nan")),
               dict(NF=(1 << 30) + 1, stride=1 << 31)):
        assert vad(**kw) == EINVAL, kw
    cap = _lib.DLIP_CMN_MAX_WINDOW
    for kw in (dict(window=cap + 1), dict(window=-1), dict(C=0), dict(NF=0), dict(B=0), dict(mw=0), dict(mw=cap + 1), dict(x=None),
               dict(y=None), dict(y=p), dict(pos=p), dict(ol=p), dict(B=1 << 20, C=1 << 11)):
        assert cmn(**kw) == EINVAL, kw


# ------------------------------------------------------------------------------------------------------------ the trainers
def test_trainers_refuse_malformed_sections_before_their_gpu_requirement():
    import train_audio
    import train_fusion
    for bad in ({"bogus": 1}, {"cmn_window": 0}, {"cmn_window": None, "vad": None}, {"vad": {"proportion_threshold": 2}}):
        with pytest.raises(ValueError, match="voiced_frames"):
            train_audio.Trainer(overrides={"data.voiced_frames": bad})
        with pytest.raises(ValueError, match="voiced_frames"):
            train_fusion.Trainer("av_test", overrides={"data.python_data_config.test_from_waves": True,
                                                       "data.python_data_config.voiced_frames": bad})
    with pytest.raises(ValueError, match="test_from_waves"):        # the stage sits behind the front-end
        train_fusion.Trainer("av_test", overrides={"data.python_data_config.voiced_frames": {}})


def test_restatement_agrees_with_a_direct_computation():
    """tests/voiced_frames_ref.py on a case small enough to type the arithmetic out."""
    import voiced_frames_ref as R
    x = np.array([[1.0, 2.0, 4.0, 8.0, 16.0]], dtype=np.float32)
    got = R.cmn(x, 3)                                               # centred, window 3: [0,3) [0,3) [1,4) [2,5) [2,5)
    want = x[0] - np.array([7 / 3, 7 / 3, 14 / 3, 28 / 3, 28 / 3])
    assert np.allclose(got[0], want, rtol=2e-7, atol=0)
    assert np.array_equal(R.cmn(x, 300), (x.astype(np.float64) - 31 / 5).astype(np.float32))
    e = np.array([0, 0, 10, 10, 10, 0, 0, 0], dtype=np.float32)
    v, thr, margin = R.vad(e, 5.5, 0.0, 0, 0.6)
    assert thr == np.float32(5.5) and margin == 4.5 and v.tolist() == [False, False, True, True, True, False, False, False]
    v, thr, _ = R.vad(e, 1.0, 0.5, 1, 0.6)                          # thr = 1 + 0.5 * 30 / 8; two of three neighbours decide
    assert thr == np.float32(2.875) and v.tolist() == [False, False, True, True, True, False, False, False]
    # the 5 * 0.6f tie: 0.6f lies above 0.6 and the exact product exactly between 3 and the next float -- it rounds to 3 (even), so
    # three voiced frames of five are enough in fp32 where the fp64 product 3.0000001 would refuse them
    assert np.float32(5) * np.float32(0.6) == np.float32(3) and 5 * float(np.float32(0.6)) > 3.0
    v, _, _ = R.vad(e, 5.5, 0.0, 2, 0.6)
    assert v.tolist() == [False, False, True, True, True, False, False, False]
    v, _, _ = R.vad(e, 5.5, 0.0, 2, 0.12)
    assert v.tolist() == [True, True, True, True, True, True, True, False]
    packed, k, fb = R.select(np.arange(8, dtype=np.float32)[None], v, min_keep=1)
    assert k == 7 and fb == 0 and packed[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 0]
    assert R.select(np.arange(8, dtype=np.float32)[None], v, min_keep=8)[1:] == (8, 1)
