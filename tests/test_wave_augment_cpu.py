"""Waveform augmentation, host side (no GPU): the ABI 60 entry points in header, library and binding; the tile constants; the random
draws of ``WaveAugment.draw``; the drop-in ``AddNoise``'s use of Python's ``random`` stream against a literal restatement of the
reference's lines (models/video_models/preprocess.py:165-173); the ``data.augment`` section's refusals; CPU tensors refused.
DESIGN.md section 4d holds the definitions."""
import ctypes
import random
import warnings

import numpy as np
import pytest
import torch

import test_abi_cpu as abi
from deeplip_amd import weightgen as wg

NAMES = ("dlip_wave_reverb_workspace_bytes", "dlip_wave_reverb_f32", "dlip_wave_add_noise_f32", "dlip_wave_normalize_f32")
ARITY = {"dlip_wave_reverb_workspace_bytes": 2, "dlip_wave_reverb_f32": 15, "dlip_wave_add_noise_f32": 12, "dlip_wave_normalize_f32": 8}


def test_entry_points_are_declared_exported_and_bound():
    from deeplip_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.HEADER["DLIP_ABI_VERSION"] == _lib.ABI_VERSION >= 60
    for n in NAMES:
        assert n in abi.header_symbols() and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[n]) == ARITY[n], n
        assert all(t in (_lib.c_f, _lib.c_i32, _lib.c_i64) for t in _lib.SIGNATURES[n]), n     # no host pointer, no float scalar
    assert _lib.PROTOTYPES["dlip_wave_reverb_workspace_bytes"][0] is ctypes.c_int64
    # host-only queries of the built library: two doubles per row and tile; bad sizes are refused
    l = _lib.lib()
    T = _lib.DLIP_FIR_TILE
    assert l.dlip_wave_reverb_workspace_bytes(3, 2 * T + 3) == 3 * 3 * 16
    assert l.dlip_wave_reverb_workspace_bytes(1, T) == 16
    assert l.dlip_wave_reverb_workspace_bytes(0, T) < 0 and l.dlip_wave_reverb_workspace_bytes(1, 0) < 0
    assert l.dlip_wave_reverb_workspace_bytes(65536, T) < 0


def test_tile_constants_come_from_the_header():
    from deeplip_amd import _lib
    assert _lib.DLIP_FIR_TILE == _lib.HEADER["DLIP_FIR_TILE"] and _lib.DLIP_FIR_TAP_CHUNK == _lib.HEADER["DLIP_FIR_TAP_CHUNK"]
    assert _lib.DLIP_FIR_TILE % 256 == 0 and _lib.DLIP_FIR_TAP_CHUNK % 16 == 0
    assert _lib.DLIP_FIR_MAX_TAPS == 8192 and _lib.DLIP_FIR_MAX_TAPS % _lib.DLIP_FIR_TAP_CHUNK == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is visible: an accepted call would launch on made-up addresses")
def test_refuses_bad_arguments_on_the_host():
    """Argument checks run before any launch: a response wider than the compiled cap, null pointers, a short workspace."""
    from deeplip_amd import _lib
    l = _lib.lib()
    p = 4096                                                       # any non-null, 8-byte aligned address: nothing is dereferenced
    ok = dict(B=2, S=100, R=1)
    assert l.dlip_wave_reverb_f32(p, None, p, p, p, p, p + 8, p, 32, ok["B"], ok["S"], ok["R"], _lib.DLIP_FIR_MAX_TAPS + 1, 1, None) == -1
    assert l.dlip_wave_reverb_f32(p, None, p, p, p, p, p, p, 32, ok["B"], ok["S"], ok["R"], 8, 1, None) == -1          # y is x
    assert l.dlip_wave_reverb_f32(p, None, p, p, p, p, p + 8, p, 31, ok["B"], ok["S"], ok["R"], 8, 1, None) == -1      # workspace short
    assert l.dlip_wave_add_noise_f32(p, None, None, 10, p, p, p, p, 32, 2, 100, None) == -1
    assert l.dlip_wave_add_noise_f32(p, None, p, 0, p, p, p, p, 32, 2, 100, None) == -1
    assert l.dlip_wave_normalize_f32(p, None, p, p + 4, 64, 2, 100, None) == -1                                        # misaligned
    assert l.dlip_wave_normalize_f32(p, None, None, p, 32, 2, 100, None) == -1


# ------------------------------------------------------------------------------------------------------------------- the draws
def _aug(**kw):
    from deeplip_amd.augment import WaveAugment
    kw.setdefault("noise", wg.gen("wa.cpu.noise", (1000,)))
    return WaveAugment(**kw)


def test_draw_is_reproducible_and_within_bounds():
    aug = _aug(rirs=[np.array([1.0, 0.5]), np.array([0.1, 1.0, 0.2])], p_reverb=0.5)
    lens = [1000, 999, 400, 1]
    a = aug.draw(lens, np.random.default_rng(7))
    b = aug.draw(np.asarray(lens), np.random.default_rng(7))
    assert sorted(a) == ["noise_start", "rir_idx", "snr_db"]
    assert a["snr_db"].dtype == np.float32 and a["noise_start"].dtype == np.int64 and a["rir_idx"].dtype == np.int32
    for k in a:
        assert a[k].shape == (4,) and np.array_equal(a[k], b[k]), k
    assert not all(np.array_equal(a[k], aug.draw(lens, np.random.default_rng(8))[k]) for k in a)
    # many draws: every level and every response comes up; the starts stay in [0, len(noise) - n] and reach both ends
    rng = np.random.default_rng(0)
    seen_snr, seen_rir, starts = set(), set(), []
    for _ in range(300):
        p = aug.draw([998] * 8, rng)
        seen_snr |= set(p["snr_db"].tolist())
        seen_rir |= set(p["rir_idx"].tolist())
        live = p["snr_db"] < 9999
        assert (p["noise_start"][~live] == 0).all()
        starts += p["noise_start"][live].tolist()
    assert seen_snr == {-5.0, 0.0, 5.0, 10.0, 15.0, 20.0, 9999.0} and seen_rir == {-1, 0, 1}
    assert min(starts) == 0 and max(starts) == 2 and set(starts) == {0, 1, 2}
    # a row as long as the bank has the one start 0
    assert (aug.draw([1000] * 50, np.random.default_rng(1))["noise_start"] == 0).all()


def test_sentinel_level_yields_pass_through_rows():
    p = _aug(snr_levels=(9999,)).draw([10] * 6, np.random.default_rng(0))
    assert (p["snr_db"] == 9999).all() and (p["noise_start"] == 0).all() and (p["rir_idx"] == -1).all()
    from deeplip_amd.augment import WaveAugment
    p = WaveAugment(noise=None, normalize=True).draw([10] * 3, np.random.default_rng(0))          # no bank: every row at the sentinel
    assert (p["snr_db"] == 9999).all()


def test_p_reverb_zero_and_one_give_none_and_all():
    rirs = [np.array([1.0]), np.array([0.0, 1.0]), np.array([1.0, 0.0, 0.3])]
    none = _aug(rirs=rirs, p_reverb=0.0).draw([5] * 64, np.random.default_rng(3))["rir_idx"]
    every = _aug(rirs=rirs, p_reverb=1.0).draw([5] * 64, np.random.default_rng(3))["rir_idx"]
    assert (none == -1).all() and (every >= 0).all() and set(every.tolist()) == {0, 1, 2}


def test_a_bank_shorter_than_a_row_raises():
    aug = _aug(snr_levels=(0,))
    with pytest.raises(ValueError, match="row 2"):
        aug.draw([1000, 5, 1001], np.random.default_rng(0))
    aug.draw([1000, 5, 1000], np.random.default_rng(0))


def test_long_responses_are_truncated_and_their_peak_recomputed():
    from deeplip_amd.augment import WaveAugment
    h = np.zeros(40, dtype=np.float32)
    h[3], h[30] = 0.5, 1.0                                         # the largest tap lies in the part that is cut
    with pytest.warns(UserWarning, match="truncated"):
        aug = WaveAugment(rirs=[np.array([0.2, 1.0, 0.1]), h], p_reverb=1.0, max_taps=16)
    assert aug.truncated == [1]
    assert aug.rir.shape == (2, 16) and aug.rir_len.tolist() == [3, 16] and aug.rir_peak.tolist() == [1, 3]
    assert np.array_equal(aug.rir[1], h[:16]) and not aug.rir[0, 3:].any()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert WaveAugment(rirs=[h], p_reverb=1.0, max_taps=64).rir_peak.tolist() == [30]
    with pytest.raises(ValueError):
        WaveAugment(rirs=[h], max_taps=8193)
    # the synthetic set holds one response longer than the default cap, lengths differ, the direct path is the largest tap
    from deeplip_amd.synthetic import noise_bank, room_responses
    rs = room_responses()
    assert len({r.size for r in rs}) == len(rs) and max(r.size for r in rs) > 8192
    assert all(r[int(np.argmax(np.abs(r)))] == 1.0 and int(np.argmax(np.abs(r))) < 48 for r in rs)
    assert np.array_equal(rs[2], room_responses()[2])
    bank = noise_bank(0.5)
    assert bank.shape == (8000,) and bank.dtype == np.float32 and np.array_equal(bank, noise_bank(0.5)) and bank.std() > 0


# ------------------------------------------------------------------------------------------------------------------ the drop-in
def _reference_draws(noise_len, levels, lengths):
    """models/video_models/preprocess.py:165-173, the lines that consume ``random``, restated literally."""
    out = []
    for n in lengths:
        snr_target = random.choice(levels)
        if snr_target == 9999:
            out.append((snr_target, None))
        else:
            start_idx = random.randint(0, noise_len - n)
            out.append((snr_target, start_idx))
    return out


def test_drop_in_add_noise_consumes_the_random_stream_as_the_reference_does():
    from models.video_models.preprocess import AddNoise, NormalizeUtterance
    levels = [-5, 0, 5, 10, 15, 20, 9999]
    noise = wg.gen("wa.cpu.dropin", (5000,))
    t = AddNoise(noise)
    assert t.snr_levels == levels and t.noise is noise
    NormalizeUtterance()
    lengths = [4000, 5000, 17, 2500, 1, 4999, 300, 1234]
    random.seed(11)
    want = [_reference_draws(len(noise), levels, [n])[0] for n in lengths]                # 8 calls on one signal each
    state = random.getstate()
    random.seed(11)
    got = []
    for n in lengths:
        snr, start = t.draw([n])
        got.append((int(snr[0]), None if snr[0] == 9999 else int(start[0])))
    assert got == want and random.getstate() == state
    assert {s for s, _ in want} > {9999} and any(s == 9999 for s, _ in want)              # both branches were taken
    random.seed(11)                                                                       # ... and one batch of 8 rows likewise
    snr, start = t.draw(lengths)
    assert [(int(a), None if a == 9999 else int(b)) for a, b in zip(snr, start)] == want and random.getstate() == state
    with pytest.raises(AssertionError):
        AddNoise(np.arange(10))                                                           # preprocess.py:155


# ---------------------------------------------------------------------------------------------------------------- the trainer
def test_malformed_augment_sections_are_refused():
    import train_audio
    from deeplip_amd.augment import parse_augment_section
    assert train_audio.parse_wave_training({}) == (False, None)
    assert train_audio.parse_wave_training({"train_from_waves": False}) == (False, None)
    on, aug = train_audio.parse_wave_training({"train_from_waves": True, "augment": {"snr_levels": [0, 9999], "p_reverb": 0.25}})
    assert on and aug == {"snr_levels": (0.0, 9999.0), "p_reverb": 0.25, "keep_power": True, "normalize": False, "max_taps": 8192}
    assert parse_augment_section({}) == {"p_reverb": 0.0, "keep_power": True, "normalize": False, "max_taps": 8192}
    for bad in ({"snr": [0]}, {"p_reverb": 1.5}, {"p_reverb": -0.1}, {"snr_levels": []}, {"max_taps": 0}, {"max_taps": 10 ** 6}, [1, 2]):
        with pytest.raises(ValueError):
            train_audio.parse_wave_training({"train_from_waves": True, "augment": bad})
    with pytest.raises(ValueError, match="train_from_waves"):
        train_audio.parse_wave_training({"augment": {"p_reverb": 0.5}})
    # ... and by the Trainer itself, in front of its GPU requirement
    for bad in ({"bogus": 1}, {"p_reverb": 2}, {"snr_levels": []}):
        with pytest.raises(ValueError, match="augment"):
            train_audio.Trainer(overrides={"data.train_from_waves": True, "data.augment": bad})
    import yaml
    from conftest import ROOT
    import os
    with open(os.path.join(ROOT, "conf", "audio_config.yaml")) as f:
        d = yaml.safe_load(f)["data"]
    assert d["train_from_waves"] is False and "augment" not in d


def test_cpu_tensors_are_refused():
    from deeplip_amd._lib import DeepLipHipError
    from deeplip_amd.augment import WaveAugment
    from models.video_models.preprocess import NormalizeUtterance
    with pytest.raises(DeepLipHipError):
        WaveAugment(normalize=True)(torch.zeros(2, 16))
    with pytest.raises(DeepLipHipError):
        _aug()(torch.zeros(2, 16), params={"snr_db": np.zeros(2, np.float32), "noise_start": np.zeros(2, np.int64)})
    with pytest.raises(DeepLipHipError):
        NormalizeUtterance()(torch.zeros(16))
