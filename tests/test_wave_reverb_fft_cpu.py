"""The transform route of the reverberation, host side (no GPU): the ABI 65 entry points in header, library and binding; the
overlap-save constants; the two size queries; the refusals in front of any launch; ``WaveAugment(reverb="fft")`` and the ``reverb``
key of ``data.augment`` on the host.  DESIGN.md section 4i holds the definitions."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import test_abi_cpu as abi

NAMES = ("dlip_wave_rir_spectra_bytes", "dlip_wave_rir_spectra_f32", "dlip_wave_reverb_fft_workspace_bytes", "dlip_wave_reverb_fft_f32")
ARITY = {"dlip_wave_rir_spectra_bytes": 2, "dlip_wave_rir_spectra_f32": 7, "dlip_wave_reverb_fft_workspace_bytes": 3,
         "dlip_wave_reverb_fft_f32": 15}


def test_entry_points_are_declared_exported_and_bound():
    from deeplip_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.HEADER["DLIP_ABI_VERSION"] == _lib.ABI_VERSION >= 65
    for n in NAMES:
        assert n in abi.header_symbols() and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[n]) == ARITY[n], n
        assert all(t in (_lib.c_f, _lib.c_i32, _lib.c_i64) for t in _lib.SIGNATURES[n]), n     # no host pointer, no float scalar
    assert _lib.PROTOTYPES["dlip_wave_rir_spectra_bytes"] == (ctypes.c_int64, [_lib.c_i32] * 2)
    assert _lib.PROTOTYPES["dlip_wave_reverb_fft_workspace_bytes"] == (ctypes.c_int64, [_lib.c_i64, _lib.c_i64, _lib.c_i32])
    # the call takes the direct route's arguments in the direct route's order (the spectra block in the responses' place)
    assert _lib.SIGNATURES["dlip_wave_reverb_fft_f32"] == _lib.SIGNATURES["dlip_wave_reverb_f32"]
    assert _lib.SIGNATURES["dlip_wave_rir_spectra_f32"] == [_lib.c_f] * 3 + [_lib.c_i64, _lib.c_i32, _lib.c_i32, _lib.c_f]
    # the direct route's declarations are what they were
    assert _lib.DLIP_FIR_MAX_TAPS == 8192 and len(_lib.SIGNATURES["dlip_wave_reverb_f32"]) == 15


def test_block_constants_come_from_the_header():
    from deeplip_amd import _lib
    P, cap = _lib.DLIP_OLS_BLOCK, _lib.DLIP_OLS_MAX_TAPS
    assert P == _lib.HEADER["DLIP_OLS_BLOCK"] and cap == _lib.HEADER["DLIP_OLS_MAX_TAPS"] == 65536
    assert P in (1024, 2048) and P & (P - 1) == 0
    assert cap % P == 0 and _lib.DLIP_FIR_MAX_TAPS < cap < 10 ** 6


def test_size_queries_are_monotone_and_refuse_bad_sizes():
    from deeplip_amd import _lib
    l = _lib.lib()
    P, T, cap = _lib.DLIP_OLS_BLOCK, _lib.DLIP_FIR_TILE, _lib.DLIP_OLS_MAX_TAPS
    sp, ws = l.dlip_wave_rir_spectra_bytes, l.dlip_wave_reverb_fft_workspace_bytes
    # the twiddle table and one half spectrum (P complex words) per (response, partition of Lmax)
    assert sp(1, 1) == sp(1, P) == 2 * P * 8 and sp(1, P + 1) == 3 * P * 8 and sp(3, 2 * P + 5) == (1 + 3 * 3) * P * 8
    assert sp(2, cap) == (1 + 2 * cap // P) * P * 8
    for bad in ((0, 8), (1, 0), (1, cap + 1), (-1, 8), (1, -1)):
        assert sp(*bad) < 0, bad
    lens = (1, P - 1, P, P + 1, 3 * P + 1, _lib.DLIP_FIR_MAX_TAPS + 1, cap)
    for R in (1, 2, 7):
        vals = [sp(R, L) for L in lens]
        assert all(v > 0 for v in vals) and vals == sorted(vals)
        assert all(sp(R + 1, L) > sp(R, L) for L in lens)
    # the power partials of the direct route's workspace, then P complex words per (row, input block): blocks -1 .. ceil(S / P) - 1
    part = l.dlip_wave_reverb_workspace_bytes
    assert ws(1, 1, 1) == part(1, 1) + 2 * P * 8 and ws(1, P, 1) == part(1, P) + 2 * P * 8
    assert ws(3, 3 * P + 3, 2 * P + 5) == part(3, 3 * P + 3) + 3 * 5 * P * 8
    for bad in ((0, 100, 8), (1, 0, 8), (1, 100, 0), (1, 100, cap + 1), (65536, 100, 8), (1, 2 ** 31, 8)):
        assert ws(*bad) < 0, bad
    sizes = sorted({1, P - 1, P, P + 1, T - 1, T, T + 1, 3 * P + 3, 48000})
    for B in (1, 2, 256):
        vals = [ws(B, S, 8192) for S in sizes]
        assert all(v > 0 and v % 8 == 0 for v in vals) and vals == sorted(vals)
        assert all(ws(B + 1, S, 8192) > ws(B, S, 8192) for S in sizes)
        assert all(ws(B, S, lo) <= ws(B, S, hi) for S in sizes for lo, hi in zip(lens, lens[1:]))
        assert all(ws(B, S, 8) >= part(B, S) + 16 for S in sizes)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is visible: an accepted call would launch on made-up addresses")
def test_refuses_bad_arguments_on_the_host():
    """Argument checks run before any launch: a response wider than the cap, null pointers, y == x, a short or misaligned workspace."""
    from deeplip_amd import _lib
    l = _lib.lib()
    p = 4096                                                       # any non-null, 8-byte aligned address: nothing is dereferenced
    B, S, R, L = 2, 100, 1, 8
    need = l.dlip_wave_reverb_fft_workspace_bytes(B, S, L)
    cap = _lib.DLIP_OLS_MAX_TAPS

    def call(x=p, sp=p, rl=p, rp=p, ri=p, y=p + 8, ws=p, nbytes=need, Lmax=L, B=B, S=S, R=R):
        return l.dlip_wave_reverb_fft_f32(x, None, sp, rl, rp, ri, y, ws, nbytes, B, S, R, Lmax, 1, None)
    assert call(Lmax=cap + 1, nbytes=1 << 40) == -1
    assert call(Lmax=0) == -1 and call(R=0) == -1 and call(B=0) == -1 and call(S=0) == -1
    for name in ("x", "sp", "rl", "rp", "ri", "y", "ws"):
        assert call(**{name: None}) == -1, name
    assert call(y=p) == -1                                         # y is x
    assert call(nbytes=need - 1) == -1                             # workspace short
    assert call(ws=p + 4) == -1 and call(sp=p + 4) == -1           # misaligned
    sb = l.dlip_wave_rir_spectra_bytes(R, L)

    def spectra(rir=p, rl=p, sp=p, nbytes=sb, R=R, Lmax=L):
        return l.dlip_wave_rir_spectra_f32(rir, rl, sp, nbytes, R, Lmax, None)
    assert spectra(Lmax=cap + 1, nbytes=1 << 40) == -1 and spectra(Lmax=0) == -1 and spectra(R=0) == -1
    for name in ("rir", "rl", "sp"):
        assert spectra(**{name: None}) == -1, name
    assert spectra(nbytes=sb - 1) == -1 and spectra(sp=p + 4) == -1


def test_wave_augment_fft_keeps_long_responses_whole():
    from deeplip_amd import _lib
    from deeplip_amd.augment import WaveAugment
    h = np.zeros(40000, dtype=np.float32)
    h[5], h[39999] = 1.0, 0.25
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        aug = WaveAugment(rirs=[np.array([0.2, 1.0, 0.1]), h], p_reverb=1.0, reverb="fft", device="cpu")
    assert aug.reverb == "fft" and aug.max_taps == _lib.DLIP_OLS_MAX_TAPS and aug.truncated == []
    assert aug.rir.shape == (2, 40000) and aug.rir_len.tolist() == [3, 40000] and aug.rir_peak.tolist() == [1, 5]
    assert np.array_equal(aug.rir[1], h)
    # beyond the route's own cap: truncated, with the warning
    with pytest.warns(UserWarning, match="truncated"):
        aug = WaveAugment(rirs=[np.ones(_lib.DLIP_OLS_MAX_TAPS + 1, dtype=np.float32)], reverb="fft", device="cpu")
    assert aug.truncated == [0] and aug.rir.shape == (1, _lib.DLIP_OLS_MAX_TAPS)
    with pytest.raises(ValueError):
        WaveAugment(rirs=[h], reverb="fft", max_taps=65537)
    with pytest.raises(ValueError):
        WaveAugment(rirs=[h], reverb="fft", max_taps=0)
    with pytest.raises(ValueError, match="reverb"):
        WaveAugment(rirs=[h], reverb="fast")
    with pytest.raises(ValueError, match="reverb"):
        WaveAugment(rirs=[h], reverb="auto")
    # the synthetic set's long response is kept whole
    from deeplip_amd.synthetic import room_responses
    rs = room_responses()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        aug = WaveAugment(rirs=rs, p_reverb=0.5, reverb="fft", device="cpu")
    assert aug.truncated == [] and aug.rir.shape[1] == max(r.size for r in rs) > _lib.DLIP_FIR_MAX_TAPS


def test_the_default_object_is_unchanged():
    from deeplip_amd.augment import WaveAugment
    h = np.zeros(40, dtype=np.float32)
    h[3], h[30] = 0.5, 1.0
    with pytest.warns(UserWarning, match="truncated"):
        aug = WaveAugment(rirs=[np.array([0.2, 1.0, 0.1]), h], p_reverb=1.0, max_taps=16)
    assert aug.reverb == "fir" and aug.truncated == [1]
    assert aug.rir.shape == (2, 16) and aug.rir_len.tolist() == [3, 16] and aug.rir_peak.tolist() == [1, 3]
    assert WaveAugment(normalize=True).max_taps == 8192 == WaveAugment(normalize=True, reverb="fir").max_taps
    with pytest.raises(ValueError):
        WaveAugment(rirs=[h], max_taps=8193)
    with pytest.raises(ValueError):
        WaveAugment(rirs=[h], max_taps=8193, reverb="fir")
    long = np.zeros(40000, dtype=np.float32)
    long[0] = 1.0
    with pytest.warns(UserWarning, match="truncated"):
        aug = WaveAugment(rirs=[long], p_reverb=1.0)
    assert aug.truncated == [0] and aug.rir.shape == (1, 8192)


def test_parse_augment_section_takes_the_route():
    import train_audio
    from deeplip_amd.augment import parse_augment_section
    base = {"p_reverb": 0.0, "keep_power": True, "normalize": False}
    assert parse_augment_section({}) == dict(base, max_taps=8192)                          # absent key: today's dict
    assert parse_augment_section({"reverb": "fft"}) == dict(base, max_taps=65536, reverb="fft")
    assert parse_augment_section({"reverb": "fir"}) == dict(base, max_taps=8192, reverb="fir")
    assert parse_augment_section({"reverb": "fft", "max_taps": 65536, "p_reverb": 0.5}) == dict(base, p_reverb=0.5, max_taps=65536, reverb="fft")
    assert parse_augment_section({"reverb": "fft", "max_taps": 100})["max_taps"] == 100
    for bad in ({"reverb": "fft", "max_taps": 70000}, {"reverb": "x"}, {"reverb": "auto"}, {"reverb": None}, {"reverb": "fir", "max_taps": 8193},
                {"max_taps": 8193}, {"reverb": "fft", "max_taps": 0}):
        with pytest.raises(ValueError):
            parse_augment_section(bad)
        with pytest.raises(ValueError):
            train_audio.parse_wave_training({"train_from_waves": True, "augment": bad})
    on, aug = train_audio.parse_wave_training({"train_from_waves": True, "augment": {"reverb": "fft", "p_reverb": 0.5}})
    assert on and aug["reverb"] == "fft" and aug["max_taps"] == 65536
