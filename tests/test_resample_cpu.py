"""Waveform resampling (deeplip_amd/resample.py), host side (-m "not gpu"): the default filter design against
scipy's, the fp64 restatement of the definition (tests/resample_ref.py) against scipy.signal.resample_poly, the band-limited behaviour
of the design, the host logic (lengths, speed -> ratio, draws, both parsers, the trainers' refusals in front of their GPU requirement,
CPU tensors), the C ABI and the composite geometry train_fusion hands the extractor."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import resample_ref as ref
import test_abi_cpu as abi
from conftest import ROOT

RATIOS = ((1, 3), (3, 1), (2, 3), (10, 9), (10, 11), (160, 441))
LENGTHS = (1, 7, 257, 1000)
NAMES = ("dlip_wave_resample_f32", "dlip_wave_resample_fits", "dlip_wave_resample_span_words")


# ------------------------------------------------------------------------------------------------------------------ the design
def test_design_is_scipys_default():
    firwin = pytest.importorskip("scipy.signal").firwin
    from deeplip_amd.resample import design
    for up, down in RATIOS + ((441, 160), (1, 6), (147, 160)):
        u, d, h = design(up, down)
        assert (u, d) == (up, down) and h.dtype == np.float64 and h.size == 2 * 10 * max(up, down) + 1
        want = up * firwin(h.size, 1.0 / max(up, down), window=("kaiser", 5.0))
        assert np.abs(h - want).max() <= 1e-14, (up, down)
    assert design(4, 12)[:2] == (1, 3) and np.array_equal(design(4, 12)[2], design(1, 3)[2])        # reduced by the gcd
    u, d, h = design(7, 7)
    assert (u, d) == (1, 1) and h.tolist() == [1.0]
    for bad in ((0, 1), (1, -2), (1.5, 2), (True, 2)):
        with pytest.raises(ValueError):
            design(*bad)


def test_restatement_is_resample_poly():
    resample_poly = pytest.importorskip("scipy.signal").resample_poly
    from deeplip_amd.resample import design
    for up, down in RATIOS:
        h = design(up, down)[2]
        for n in LENGTHS:
            x = np.random.default_rng(1000 * up + n).standard_normal(n)
            got, want = ref.resample(x, up, down, h), resample_poly(x, up, down)
            assert got.shape == want.shape == (ref.n_out(n, up, down),)
            assert np.abs(got - want).max() <= 1e-12, (up, down, n)


def test_restatement_agrees_with_a_direct_computation():
    """The definition typed out on a case small enough to do by hand: up 2, down 3, h = [1, 2, 3, 4, 5] (c = 2), x = [1, 10, 100]:
    n_out = 2, y[0] = x[0] h[2] + x[1] h[0], y[1] = x[1] h[3] + x[2] h[1]."""
    y, a = ref.resample([1.0, 10.0, 100.0], 2, 3, [1.0, 2.0, 3.0, 4.0, 5.0], with_abs=True)
    assert y.tolist() == [3.0 + 10.0, 40.0 + 200.0] and a.tolist() == y.tolist()
    y = ref.resample([1.0, -10.0, 100.0], 2, 3, [1.0, 2.0, 3.0, 4.0, 5.0], m=[1])
    assert y.tolist() == [-40.0 + 200.0]


def _tone_run(up, down, f, n=12000):
    """A unit tone of f cycles per INPUT sample through the design: (outputs, their times in input samples), the filter's
    half length skipped at each end."""
    from deeplip_amd.resample import design
    h = design(up, down)[2]
    x = np.sin(2.0 * np.pi * f * np.arange(n) + 0.3)
    y = ref.resample(x, up, down, h)
    skip = math.ceil(10 * max(up, down) / down) + 2
    m = np.arange(y.size)[skip:-skip]
    return y[skip:-skip], m * (down / up)


@pytest.mark.parametrize("up,down", [(1, 3), (3, 1), (10, 9), (10, 11), (160, 441)])
def test_design_passes_the_band_and_stops_what_would_alias(up, down):
    narrow = 0.5 * min(1.0, up / down)                        # the narrower Nyquist, cycles per input sample
    for frac in (0.05, 0.25, 0.5, 0.75):
        y, t = _tone_run(up, down, frac * narrow)
        err = np.abs(y - np.sin(2.0 * np.pi * frac * narrow * t + 0.3)).max()
        print(f"{up}/{down}: tone at {frac} of the narrower Nyquist reproduced within {err:.2e}")
        assert err <= 4e-3, (up, down, frac)
    f = 1.25 * 0.5 * up / down                                # 1.25 x the output Nyquist
    if up < down and f < 0.5:                                 # (10/11: that tone lies above the INPUT Nyquist -- it does not exist)
        y, _ = _tone_run(up, down, f)
        print(f"{up}/{down}: tone at 1.25 x the output Nyquist leaves {np.abs(y).max():.2e}")
        assert np.abs(y).max() <= 3e-3, (up, down)


# ---------------------------------------------------------------------------------------------------------------- host logic
def test_lengths_and_speed_ratios():
    from deeplip_amd.resample import SpeedPerturb, in_len, out_len, pack_table, speed_ratio
    for up, down in RATIOS + ((441, 160),):
        for n in (1, 2, 7, 160, 441, 1000, 5_000_000):
            assert out_len(n, up, down) == math.ceil(n * up / down) == ref.n_out(n, up, down)
        for m in (1, 2, 9, 10, 11, 400, 6640):
            n = in_len(m, up, down)
            assert out_len(n, up, down) >= m and (n == 1 or out_len(n - 1, up, down) < m), (up, down, m)
    assert [speed_ratio(s) for s in (0.9, 1.0, 1.1)] == [(10, 9), (1, 1), (10, 11)]
    assert speed_ratio(0.5) == (2, 1) and speed_ratio(2.0) == (1, 2) and speed_ratio(0.95) == (20, 19)
    sp = SpeedPerturb(device="cpu")
    assert sp.speeds == (0.9, 1.0, 1.1) and sp.ratios == [(10, 9), (1, 1), (10, 11)]
    for m in (1, 400, 6640, 6641):
        n = sp.in_samples(m)
        assert all(out_len(n, u, d) >= m for u, d in sp.ratios) and any(out_len(n - 1, u, d) < m for u, d in sp.ratios)
        assert sp.out_samples(m) == out_len(m, 10, 9)
    # the polyphase table: tab[r][j] = h[r + j up], an odd row stride
    h = np.arange(1.0, 8.0)
    tab, K = pack_table(h, 3)
    assert K == 3 and tab.shape == (3, 3) and tab.tolist() == [[1, 4, 7], [2, 5, 0], [3, 6, 0]]
    tab, K = pack_table(h, 2)
    assert K == 4 and tab.shape == (2, 5) and tab.tolist() == [[1, 3, 5, 7, 0], [2, 4, 6, 0, 0]]


def test_draw_is_uniform_and_reproducible():
    from deeplip_amd.resample import SpeedPerturb
    sp = SpeedPerturb((0.9, 1.0, 1.1), device="cpu")
    a = sp.draw(3000, np.random.default_rng(7))
    b = sp.draw(3000, np.random.default_rng(7))
    assert sorted(a) == ["speed_idx"] and a["speed_idx"].dtype == np.int32 and a["speed_idx"].shape == (3000,)
    assert np.array_equal(a["speed_idx"], b["speed_idx"])
    counts = np.bincount(a["speed_idx"], minlength=3)
    assert counts.sum() == 3000 and (np.abs(counts - 1000) < 5 * math.sqrt(3000 * (1 / 3) * (2 / 3))).all(), counts   # five sigma


def test_parser_refusals():
    from deeplip_amd.resample import Resample, SpeedPerturb, parse_speed_perturb_section
    assert parse_speed_perturb_section(None) is None and parse_speed_perturb_section(False) is None
    assert parse_speed_perturb_section({"speeds": [0.9, 1, 1.1]}) == {"speeds": (0.9, 1.0, 1.1)}
    for bad in ({}, {"speeds": []}, {"speeds": [0.4]}, {"speeds": [2.5]}, {"speeds": 1.0}, {"speeds": ["fast"]}, {"speeds": [True]},
                {"speeds": [1.0], "bogus": 1}, [0.9, 1.1], "on", {"speed": [1.0]}):
        with pytest.raises(ValueError, match="speed_perturb"):
            parse_speed_perturb_section(bad)
    with pytest.raises(ValueError):
        SpeedPerturb((), device="cpu")
    with pytest.raises(ValueError):
        SpeedPerturb((0.9, 3.0), device="cpu")
    with pytest.raises(ValueError, match="nothing to apply"):
        Resample(16000, 16000, device="cpu")
    with pytest.raises(ValueError, match="LDS"):                     # 1000 / 1001: a table of 1000 x 21 words
        Resample(1001, 1000, device="cpu")
    r = Resample(48000, 16000, device="cpu")
    assert (r.up, r.down) == (1, 3) and r.out_len(2500) == 834 and r.h.size == 61
    r = Resample(44100, 16000, device="cpu", filter=np.ones(5))
    assert (r.up, r.down) == (160, 441) and r.h.tolist() == [1.0] * 5


def test_trainers_refuse_before_their_gpu_requirement():
    import train_audio
    import train_fusion
    with pytest.raises(ValueError, match="train_from_waves"):
        train_audio.Trainer(overrides={"data.speed_perturb": {"speeds": [0.9, 1.0, 1.1]}})
    for bad in ({"bogus": 1}, {"speeds": []}, {"speeds": [3.0]}):
        with pytest.raises(ValueError, match="speed_perturb"):
            train_audio.Trainer(overrides={"data.train_from_waves": True, "data.speed_perturb": bad})
    with pytest.raises(ValueError, match="test_from_waves"):
        train_fusion.Trainer("av_test", overrides={"data.python_data_config.source_rate": 48000})
    with pytest.raises(ValueError, match="source_rate"):
        train_fusion.Trainer("av_test", overrides={"data.python_data_config.test_from_waves": True,
                                                   "data.python_data_config.source_rate": 16000, "data.python_data_config.rate": 16000})
    with pytest.raises(ValueError, match="source_rate"):
        train_fusion.Trainer("av_test", overrides={"data.python_data_config.test_from_waves": True,
                                                   "data.python_data_config.source_rate": -8000})
    # the parsers the augmentation tests pin keep their results
    assert train_audio.parse_wave_training({"train_from_waves": True, "speed_perturb": {"speeds": [1.1]}}) == (True, None)
    assert train_audio.parse_speed_perturb({"train_from_waves": True}) is None


def test_cpu_tensors_are_refused():
    from deeplip_amd import _lib
    from deeplip_amd.resample import Resample, SpeedPerturb
    x = torch.zeros(2, 100)
    with pytest.raises(_lib.DeepLipHipError, match="no CPU path"):
        Resample(48000, 16000, device="cpu")(x)
    with pytest.raises(_lib.DeepLipHipError, match="no CPU path"):
        SpeedPerturb(device="cpu")(x, params={"speed_idx": np.zeros(2, dtype=np.int32)})


def test_the_shipped_configs_do_not_name_the_keys():
    import yaml
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        a = yaml.safe_load(f)
    with open(os.path.join(ROOT, "conf", "fusion_config.yaml")) as f:
        fu = yaml.safe_load(f)
    assert "speed_perturb" not in a["data"] and "source_rate" not in (fu["data"].get("python_data_config") or {})


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from deeplip_amd import _lib, build
    assert "wave_resample_ops.hip" in build.SOURCES
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.HEADER["DLIP_ABI_VERSION"] == _lib.ABI_VERSION >= 63
    for n in NAMES:
        assert n in abi.header_symbols() and hasattr(lib, n) and n in _lib.SIGNATURES, n
    VP, I32, I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    assert _lib.SIGNATURES["dlip_wave_resample_f32"] == [VP] * 7 + [I32, I64, I64, I32, I32, I32, I32, VP]
    assert _lib.PROTOTYPES["dlip_wave_resample_f32"][0] is ctypes.c_int
    assert _lib.PROTOTYPES["dlip_wave_resample_fits"] == (I32, [I32] * 3)
    assert _lib.PROTOTYPES["dlip_wave_resample_span_words"] == (I64, [I32] * 4)
    for c in ("DLIP_RESAMPLE_TILE", "DLIP_RESAMPLE_LDS_WORDS", "DLIP_RESAMPLE_MAX_FACTOR"):
        assert _lib.HEADER[c] > 0, c
    assert _lib.HEADER["DLIP_RESAMPLE_TILE"] % 256 == 0 and _lib.HEADER["DLIP_RESAMPLE_LDS_WORDS"] * 4 <= 64 * 1024


def test_fits_and_the_launch_refuse_on_the_host():
    """The ratios the kernel must take fit; one that does not gives 0 here and DLIP_EINVAL from the launch (dummy addresses, nothing
    dereferenced, no launch)."""
    from deeplip_amd import _lib
    from deeplip_amd.resample import Resample, design
    l = _lib.lib()
    EINVAL, cap, tile = _lib.HEADER["DLIP_EINVAL"], _lib.HEADER["DLIP_RESAMPLE_LDS_WORDS"], _lib.HEADER["DLIP_RESAMPLE_TILE"]
    for up, down in ((1, 3), (3, 1), (1, 6), (2, 3), (10, 9), (10, 11), (147, 160), (160, 441), (441, 160)):
        L = design(up, down)[2].size
        t = l.dlip_wave_resample_fits(up, down, L)
        K = -(-L // up)
        assert t in (256, 512, tile) and up * (K | 1) + l.dlip_wave_resample_span_words(up, down, K, t) <= cap, (up, down)
        assert l.dlip_wave_resample_span_words(up, down, K, t) == math.ceil((t - 1) * down / up) + K
        bank = Resample(down, up, device="cpu")._bank                 # what the module hands the launch
        assert (bank.tile, bank.tab_stride, bank.span_words) == (t, up * (K | 1), math.ceil((t - 1) * down / up) + K)
        assert bank.bank.tolist() == [[up, down, (L - 1) // 2, K]] and bank.tabs.shape == (1, up * (K | 1))
    assert l.dlip_wave_resample_fits(1000, 1001, 20021) == 0 and l.dlip_wave_resample_fits(0, 1, 1) == 0
    assert l.dlip_wave_resample_fits(1, _lib.HEADER["DLIP_RESAMPLE_MAX_FACTOR"] + 1, 1) == 0
    assert l.dlip_wave_resample_span_words(1, 3, 61, 100) < 0
    p, q = 4096, 8192

    def launch(**kw):
        a = dict(x=p, lens=None, tabs=p, bank=p, ridx=p, out=q, ol=p, B=2, S=100, So=34, Q=1, ts=61, sw=3130, tile=tile)
        a.update(kw)
        return l.dlip_wave_resample_f32(a["x"], a["lens"], a["tabs"], a["bank"], a["ridx"], a["out"], a["ol"], a["B"], a["S"], a["So"], a["Q"],
                                        a["ts"], a["sw"], a["tile"], None)
    for kw in (dict(x=None), dict(tabs=None), dict(bank=None), dict(ridx=None), dict(out=None), dict(ol=None), dict(out=p), dict(B=0),
               dict(B=65536), dict(S=0), dict(So=0), dict(S=1 << 31), dict(So=1 << 31), dict(Q=0), dict(ts=0), dict(sw=0), dict(tile=100),
               dict(tile=2048), dict(ts=cap, sw=1), dict(ts=21021, sw=1045)):
        assert launch(**kw) == EINVAL, kw


# ----------------------------------------------------------------------------------------------------- the composite geometry
class _Frames:
    """The front-end's geometry (sigproc.framesig), host only."""
    frame_len, frame_step, min_samples = 400, 160, 1

    def frames_for_samples(self, n):
        return 1 if n <= self.frame_len else 1 + math.ceil((n - self.frame_len) / self.frame_step)

    def samples_for_frames(self, T):
        return self.frame_len + (T - 1) * self.frame_step


@pytest.mark.parametrize("src,dst", [(48000, 16000), (44100, 16000), (8000, 16000), (16000, 44100), (24000, 16000), (17600, 16000)])
def test_composite_geometry_answers_in_source_samples(src, dst):
    from deeplip_amd.resample import Resample, ResampledGeometry, out_len
    rs = Resample(src, dst, device="cpu")
    fe = _Frames()
    g = ResampledGeometry(fe, rs)
    assert g.frame_len == round(400 * src / dst) and g.frame_step == round(160 * src / dst)
    for T in (1, 2, 3, 24, 25, 60, 61, 120, 137, 412, 1000):
        S = g.samples_for_frames(T)
        assert g.frames_for_samples(S) == T and g.frames_for_samples(S + 1) > T, (T, S)
        assert g.frames_for_samples(S) == fe.frames_for_samples(out_len(S, rs.up, rs.down))
    assert g.min_samples == 1
    fe.min_samples = 257
    assert out_len(g.min_samples, rs.up, rs.down) >= 257 > out_len(g.min_samples - 1, rs.up, rs.down)
