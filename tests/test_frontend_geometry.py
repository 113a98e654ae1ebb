"""The audio / video front-end away from the one geometry tests/test_frontend.py runs (16 kHz, 400 / 160-sample frames, nfft 512):
other FFT sizes and thread counts, 8 kHz telephone speech, non-power-of-two nfft (the GEMM route), 22.05 / 44.1 kHz (where
frame length and step round half UP), utterances of 1 .. 3 frames, digital silence, launches above the 2048-block grid cap, and the
entry points' parameters the Python classes never pass.  The reference is the oracle's fp64 restatement of python_speech_features
(oracle/deeplip_oracle.py) or, for the kernels called directly, a float64 numpy restatement written next to the call.

Tolerances are the ones tests/test_frontend.py already holds this code to:
  * un-normalised, "fft64" route: EVERY element within 1e-4 x the reference's largest magnitude;
  * un-normalised, fp32 routes ("gemm32", "direct64"): the same on every element but those where the reference is below -20 (the
    fp32 noise floor of test_default_route_resolves_the_bands_that_pre_emphasis_empties), which may be at most 1 % of the tensor.
    Elements that are at the floor BY CONSTRUCTION -- an empty mel filter, a frame of exact zeros -- are log(eps) exactly in any
    arithmetic: they are not excluded but held to the bound (or to log(eps) directly) on every route;
  * normalised: rel_err < 1e-4 on the bands with raw.std(axis=1) > 1e-4 * |raw|.max(), at most one band excluded;
  * the simple fp32 kernels called directly: rel_err < 1e-6; the crop is bit-exact.
"""
import functools

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import deeplip_oracle as O

LOG_EPS = float(np.log(2.220446049250313e-16))          # log(np.finfo(float).eps) = -36.04
ROUTES = ("fft64", "gemm32", "direct64")

# id -> AudioFrontend geometry (win_len / win_shift default to 0.025 / 0.01) and the utterance's duration in seconds
GEOMS = {
    "8k": dict(rate=8000, nfft=256),
    "fft1024": dict(rate=16000, nfft=1024),
    "fft128": dict(rate=16000, nfft=128, win_len=0.008, win_shift=0.004),      # frame = nfft = 128: no zero padding, one wave
    "n400": dict(rate=16000, nfft=400),
    "n200": dict(rate=8000, nfft=200),
    "22k": dict(rate=22050, nfft=1024),                                         # 551 / 221 samples: frame_len > blockDim = 512
    "44k": dict(rate=44100, nfft=2048),                                         # 1103 / 441 samples
}
DURATION = {"44k": 0.5}
# (geometry, mel bank sizes, routes (None: the default), feature types)
SWEEP = (
    ("8k", (26, 40), ROUTES, ("mfcc", "logfbank", "fbank")),
    ("fft1024", (26, 60), ROUTES, ("mfcc", "logfbank", "fbank")),
    ("fft128", (26,), ROUTES, ("mfcc", "logfbank", "fbank")),
    ("n400", (26,), (None,), ("mfcc",)),
    ("n200", (24,), (None,), ("mfcc",)),
    ("22k", (26,), ("fft64", "gemm32"), ("mfcc",)),
    ("44k", (26,), (None,), ("mfcc",)),
)
SWEEP_CASES = [(g, nb, r, f) for g, nbs, rs, fs in SWEEP for nb in nbs for r in rs for f in fs]
SWEEP_IDS = [f"{g}-{nb}-{r or 'default'}-{f}" for g, nb, r, f in SWEEP_CASES]


def _default_route(nfft):
    return "fft64" if 128 <= nfft <= 1024 and nfft & (nfft - 1) == 0 else "gemm32"


def _oracle_kw(gid, num_bin):
    g = GEOMS[gid]
    return dict(rate=g["rate"], nfft=g["nfft"], winlen=g.get("win_len", 0.025), winstep=g.get("win_shift", 0.01), nfilt=num_bin)


@functools.lru_cache(maxsize=None)
def _signal(gid):
    """B = 2 utterances of 0.3 sin + 0.05 white noise, 100 samples short of 1 s: the last frame is a partial one at every geometry,
    and at 22.05 kHz a step of 220 samples (round-half-even) makes 99 frames of the 21 950 samples where 221 makes 98."""
    rate = GEOMS[gid]["rate"]
    S = int(DURATION.get(gid, 1.0) * rate) - 100
    r = np.random.Generator(np.random.PCG64(2024))
    t = np.arange(S) / float(rate)
    sig = np.stack([0.3 * np.sin(2 * np.pi * (200 + 150 * b) * t) + 0.05 * r.standard_normal(S) for b in range(2)]).astype(np.float32)
    sig.setflags(write=False)
    return sig


@functools.lru_cache(maxsize=None)
def _ref(gid, num_bin, feat, normalize):
    """The oracle on each utterance of _signal(gid), computed once and shared: [B, F, NF] float32, read-only."""
    out = np.stack([O.audio_features(s.astype(np.float64), feat, normalize=normalize, **_oracle_kw(gid, num_bin)) for s in _signal(gid)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _empty_bands(gid, num_bin):
    """Mel filters without a single FFT bin (floor() collapses their corners): constant log(eps) rows of a (log-)fbank."""
    kw = _oracle_kw(gid, num_bin)
    return O.psf_get_filterbanks(num_bin, kw["nfft"], kw["rate"]).sum(axis=1) == 0


def _fp32_floor(ref, logfb, feat, empty, silent=None):
    """Elements an fp32 route is not held to.  The floor is a property of the log mel energies: the reference's un-normalised
    logfbank ``logfb`` [.., nfilt, NF] below -20, minus what is log(eps) by construction (``empty`` filters, ``silent`` frames).
    logfbank: those elements.  mfcc: the DCT spreads a frame's floor band over its cepstra, so c1 .. of the frames that hold such
    an element (c0 is the log frame energy); a cepstrum that is itself below -20 is an ordinary value and stays in.  fbank: none
    (the linear energies are compared against the largest one)."""
    low = (logfb < -20.0) & ~empty[:, None]
    if silent is not None:
        low = low & ~silent
    floor = np.zeros(ref.shape, bool)
    if feat == "logfbank":
        floor = low
    elif feat == "mfcc":
        floor[..., 1:, :] = low.any(axis=-2, keepdims=True)
    return floor


def _noise_floor(gid, num_bin, feat):
    return _fp32_floor(_ref(gid, num_bin, feat, False), _ref(gid, num_bin, "logfbank", False), feat, _empty_bands(gid, num_bin))


def _live_bands(raw):
    return raw.std(axis=1) > 1e-4 * np.abs(raw).max()


def _check_raw(y, ref, route, floor, what):
    """The un-normalised rule.  y, ref [F, NF]; floor: the fp32 routes' excluded elements (ignored on "fft64")."""
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    scale = np.abs(ref).max()
    err = np.abs(y.astype(np.float64) - ref)
    if route == "fft64":
        floor = np.zeros_like(floor)
    worst = (err * ~floor).max()
    print(f"{what}: max err {worst:.3e} = {worst / scale:.3e} x scale {scale:.4g}; {int(floor.sum())} of {floor.size} excluded")
    assert floor.mean() <= 0.01, what
    assert worst < 1e-4 * scale, what


# ------------------------------------------------------------------------------------------------------------------------------------
# CPU: the geometry arithmetic, the filterbank, the constructor, and the conditions the GPU tests' rules rest on (reference alone)
# ------------------------------------------------------------------------------------------------------------------------------------
def test_mel_filterbank_equals_the_oracles_at_every_geometry():
    from deeplip_amd.frontend import mel_filterbank
    for gid, nbs, _, _ in SWEEP:
        for nb in nbs:
            kw = _oracle_kw(gid, nb)
            ours, theirs = mel_filterbank(nb, kw["nfft"], kw["rate"]), O.psf_get_filterbanks(nb, kw["nfft"], kw["rate"])
            assert ours.shape == theirs.shape == (nb, kw["nfft"] // 2 + 1)
            assert np.array_equal(ours, theirs), (gid, nb, float(np.abs(ours - theirs).max()))
    assert int(_empty_bands("fft128", 26).sum()) == 1          # (the one empty filter the sweep's rules speak of)


def test_constructor_names_the_limit_it_refuses():
    from deeplip_amd.frontend import AudioFrontend
    with pytest.raises(ValueError, match=r"direct64.*power of two <= 1024.*nfft=400"):
        AudioFrontend(dft="direct64", nfft=400, device="cpu")
    with pytest.raises(ValueError, match=r"direct64.*power of two <= 1024.*nfft=2048"):
        AudioFrontend(dft="direct64", nfft=2048, rate=44100, device="cpu")
    with pytest.raises(ValueError, match=r"direct64.*power of two"):
        AudioFrontend(dft64=True, nfft=400, device="cpu")                       # the older switch for the same route
    for dft in (None,) + ROUTES:
        with pytest.raises(ValueError, match=r"nfft must be >= the frame length \(400 samples.*nfft=256"):
            AudioFrontend(dft=dft, nfft=256, device="cpu")                      # 16 kHz: 400-sample frames
    with pytest.raises(ValueError, match=r"nfft must be >= the frame length \(551 samples"):
        AudioFrontend(rate=22050, nfft=512, device="cpu")
    with pytest.raises(ValueError, match=r"gemm32.*multiple of 4.*nfft=402"):
        AudioFrontend(nfft=402, device="cpu")                                   # (the GEMM's reduction length)
    # the DEFAULT route still falls back to the GEMM for an nfft the FFT kernel does not take; an explicit route is kept
    for nfft, rate, want in ((400, 16000, "gemm32"), (200, 8000, "gemm32"), (2048, 44100, "gemm32"), (64, 2000, "gemm32"),
                             (128, 4000, "fft64"), (256, 8000, "fft64"), (1024, 22050, "fft64")):
        assert AudioFrontend(nfft=nfft, rate=rate, device="cpu").dft == want == _default_route(nfft), (nfft, rate)
    assert AudioFrontend(dft="fft64", nfft=400, device="cpu").dft == "gemm32"
    assert AudioFrontend(dft="direct64", nfft=1024, device="cpu").dft == "direct64"
    assert AudioFrontend(dft="gemm32", nfft=1024, device="cpu").dft == "gemm32"
    fe = AudioFrontend(rate=8000, nfft=256, device="cpu")
    assert (fe.frame_len, fe.frame_step, fe.nb, fe.nbp) == (200, 80, 129, 132)


def test_the_sweeps_rules_hold_for_its_signals_with_the_reference_alone():
    """What the GPU tests below take for granted, shown with the oracle alone: below-floor elements are at most 1 % of every
    un-normalised tensor, at most one band per case is not live (exactly one at fft128 / 26, whose band 0 is an empty filter), and
    NF is what the corrected rounding gives (with the 220-sample step of round-half-even, 22.05 kHz had 99 frames)."""
    from deeplip_amd.frontend import num_frames
    assert num_frames(21950, 551, 220) == 99 and num_frames(21950, 551, 221) == 98
    nf = {gid: _ref(gid, nbs[0], "mfcc", False).shape[2] for gid, nbs, _, _ in SWEEP}
    assert nf == {"8k": 98, "fft1024": 98, "fft128": 248, "n400": 98, "n200": 98, "22k": 98, "44k": 49}
    for gid, nb, _, feat in sorted(set((g, nb, None, f) for g, nb, _, f in SWEEP_CASES)):
        raw = _ref(gid, nb, feat, False)
        for b in range(raw.shape[0]):
            assert _noise_floor(gid, nb, feat)[b].mean() <= 0.01, (gid, nb, feat, b)
            dead = int((~_live_bands(raw[b])).sum())
            assert dead == (1 if (gid, feat != "mfcc") == ("fft128", True) else 0), (gid, nb, feat, b, dead)


# ------------------------------------------------------------------------------------------------------------------------------------
# (b) the geometry sweep
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("gid,num_bin,route,feat", SWEEP_CASES, ids=SWEEP_IDS)
def test_geometry_sweep_vs_oracle(gid, num_bin, route, feat):
    from deeplip_amd.frontend import AudioFrontend
    g = GEOMS[gid]
    x = torch.tensor(_signal(gid)).cuda()
    want_route = route or _default_route(g["nfft"])
    raw, ref = _ref(gid, num_bin, feat, False), _ref(gid, num_bin, feat, True)
    fe = AudioFrontend(feat, num_bin=num_bin, normalize=False, dft=route, **g)
    assert fe.dft == want_route
    y = fe(x).cpu().numpy()
    assert y.shape == raw.shape, (y.shape, raw.shape)                          # [B, F, NF]: NF is the oracle's
    floor = _noise_floor(gid, num_bin, feat)
    for b in range(raw.shape[0]):
        _check_raw(y[b], raw[b], want_route, floor[b], f"{gid}/{num_bin}/{want_route}/{feat} b={b} un-normalised")
    yn = AudioFrontend(feat, num_bin=num_bin, dft=route, **g)(x).cpu().numpy()
    assert yn.shape == ref.shape
    for b in range(raw.shape[0]):
        live = _live_bands(raw[b])
        assert live.sum() >= raw.shape[1] - 1
        e = rel_err(yn[b][live], ref[b][live])
        print(f"{gid}/{num_bin}/{want_route}/{feat} b={b} normalised: rel_err {e:.3e} on {int(live.sum())} of {live.size} bands")
        assert e < 1e-4, (gid, num_bin, want_route, feat, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# (c) utterances of one, two and three frames
# ------------------------------------------------------------------------------------------------------------------------------------
DEGENERATE = ((1, 1), (2, 1), (199, 1), (200, 1), (201, 2), (280, 2), (281, 3))      # (S, NF) at 8 kHz: 200 / 80-sample frames


@functools.lru_cache(maxsize=None)
def _short_signal(S):
    """White noise, the first S samples of one fixed draw (so x[0] != 0: S = 1 is the pre-emphasis' n == 0 branch alone)."""
    x = (0.1 * np.random.Generator(np.random.PCG64(77)).standard_normal((2, 281)))[:, :S].astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _short_ref(S, normalize):
    out = np.stack([O.audio_features(s.astype(np.float64), "mfcc", normalize=normalize, delta=True, **_oracle_kw("8k", 26))
                    for s in _short_signal(S)])
    out.setflags(write=False)
    return out


def test_short_utterances_reference_conditions():
    """With the reference alone: NF as listed; at NF = 1 CMVN is 0 / 2e-12 = 0 and so are the deltas; at NF = 2, 3 all 24 cepstra
    are live, so the normalised comparison below leaves nothing out."""
    for S, NF in DEGENERATE:
        raw, ref = _short_ref(S, False), _short_ref(S, True)
        assert raw.shape == ref.shape == (2, 72, NF)
        if NF == 1:
            assert not ref.any() and np.abs(raw[:, 24:]).max() < 1e-12     # (un-normalised deltas: the dot product's rounding)
        else:
            for b in range(2):
                assert _live_bands(raw[b, :24]).all(), (S, b)


@pytest.mark.gpu
@pytest.mark.parametrize("S,NF", DEGENERATE)
def test_short_utterances_vs_oracle(S, NF):
    from deeplip_amd.frontend import AudioFrontend
    x = torch.tensor(_short_signal(S)).cuda()
    raw, ref = _short_ref(S, False), _short_ref(S, True)
    fe = AudioFrontend("mfcc", normalize=False, delta=True, **GEOMS["8k"])
    assert fe.dft == "fft64" and fe.feat_dim == 72
    y = fe(x).cpu().numpy()
    assert y.shape == (2, 72, NF)
    for b in range(2):
        _check_raw(y[b], raw[b], "fft64", np.zeros(raw[b].shape, bool), f"S={S} b={b} un-normalised + deltas")
    yn = AudioFrontend("mfcc", delta=True, **GEOMS["8k"])(x).cpu().numpy()
    assert yn.shape == (2, 72, NF)
    if NF == 1:
        assert np.all(yn == 0.0)                                                # base, delta and delta-delta: exactly zero
    else:
        for b in range(2):
            e = rel_err(yn[b], ref[b])
            print(f"S={S} b={b} normalised + deltas: rel_err {e:.3e}")
            assert e < 1e-4, (S, b)


# ------------------------------------------------------------------------------------------------------------------------------------
# (d) digital silence
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gated_signal():
    """8 kHz, 1 s, exactly zero outside samples 3000 .. 5999 (leading / trailing padding of a real recording)."""
    S = 8000
    r = np.random.Generator(np.random.PCG64(5))
    x = np.zeros((2, S), np.float32)
    for b in range(2):
        x[b, 3000:6000] = (0.3 * np.sin(2 * np.pi * (200 + 150 * b) * np.arange(3000) / 8000.0) + 0.05 * r.standard_normal(3000))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _gated_ref(feat):
    out = np.stack([O.audio_features(s.astype(np.float64), feat, normalize=False, **_oracle_kw("8k", 26)) for s in _gated_signal()])
    out.setflags(write=False)
    return out


def _zero_frames():
    """Frames f = samples [80 f, 80 f + 200) that see only zeros: those ending by 3000 and those starting after sample 6000 (which
    pre-emphasis makes -0.97 x[5999])."""
    f = np.arange(99)
    return (80 * f + 200 <= 3000) | (80 * f >= 6001)


def test_gated_signal_reference_conditions():
    zf = _zero_frames()
    assert int(zf.sum()) == 59
    lf, mf = _gated_ref("logfbank"), _gated_ref("mfcc")
    assert lf.shape == (2, 26, 99) and mf.shape == (2, 24, 99)
    assert np.all(lf[:, :, zf] == np.float32(LOG_EPS)) and np.all(mf[:, 0, zf] == np.float32(LOG_EPS))
    assert np.all(lf[:, :, ~zf] > -30.0)                                        # ... and no other frame is silent
    for feat, ref in (("logfbank", lf), ("mfcc", mf)):                          # outside those frames the fp32 floor is <= 1 %
        assert _fp32_floor(ref, lf, feat, _empty_bands("8k", 26), silent=zf).mean() <= 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("feat", ["logfbank", "mfcc"])
def test_silent_frames_take_the_eps_branches(route, feat):
    from deeplip_amd.frontend import AudioFrontend
    zf = _zero_frames()
    ref = _gated_ref(feat)
    y = AudioFrontend(feat, normalize=False, dft=route, **GEOMS["8k"])(torch.tensor(_gated_signal()).cuda()).cpu().numpy()
    assert y.shape == ref.shape
    for b in range(2):
        floor = _fp32_floor(ref[b], _gated_ref("logfbank")[b], feat, _empty_bands("8k", 26), silent=zf)   # silent frames: NOT excluded ...
        _check_raw(y[b], ref[b], route, floor, f"gated/{route}/{feat} b={b}")
        silent = y[b][:, zf] if feat == "logfbank" else y[b][0:1, zf]           # ... and their log(0 -> eps) / log(energy 0 -> eps)
        e = np.abs(silent.astype(np.float64) - LOG_EPS).max() / abs(LOG_EPS)
        print(f"gated/{route}/{feat} b={b}: silent frames off log(eps) by {e:.3e} relative")
        assert e < 1e-6, (route, feat, b)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ROUTES)
def test_all_zero_utterance(route):
    from deeplip_amd.frontend import AudioFrontend
    x = torch.zeros((2, 8000), dtype=torch.float32).cuda()
    y = AudioFrontend("logfbank", normalize=False, dft=route, **GEOMS["8k"])(x).cpu().numpy()
    assert y.shape == (2, 26, 99)
    assert np.abs(y.astype(np.float64) - LOG_EPS).max() < 1e-6 * abs(LOG_EPS)
    yn = AudioFrontend("logfbank", dft=route, **GEOMS["8k"])(x).cpu().numpy()
    assert yn.shape == (2, 26, 99) and np.all(yn == 0.0)                        # (v - mean) / (0 + 2e-12), mean == v exactly


# ------------------------------------------------------------------------------------------------------------------------------------
# (e) the kernels through lib(), each against a float64 restatement
# ------------------------------------------------------------------------------------------------------------------------------------
GRID_CAP_THREADS = 2048 * 256          # frontend_ops.hip: kGridCap blocks of 256 threads; above it the kernels loop


def _L():
    from deeplip_amd import _lib
    return _lib


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args, L.stream_handle()), name)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_log_floor_above_the_grid_cap():
    n = GRID_CAP_THREADS + 777
    r = np.random.Generator(np.random.PCG64(1))
    x = (10.0 ** r.uniform(-20.0, 10.0, n)).astype(np.float32)
    x[r.integers(0, n, 5000)] = 0.0
    x[[0, n - 1, GRID_CAP_THREADS - 1, GRID_CAP_THREADS]] = 0.0                 # both sides of the wrap, first and last element
    xd = torch.from_numpy(x).cuda()
    yd = torch.full((n + 64,), float("nan"), device="cuda")
    _call("dlip_log_floor_f32", xd.data_ptr(), yd.data_ptr(), n)
    y = yd.cpu().numpy()
    ref = np.log(np.where(x == 0, 2.220446049250313e-16, x.astype(np.float64)))
    assert rel_err(y[:n], ref) < 1e-6
    assert np.isnan(y[n:]).all()                                                # nothing written past n


def _delta_ref(x, order):
    """[B, C, NF] float64 -> [B, (1 + order) C, NF]: base | delta(N=1) | delta(N=2), both of the base, edge-clamped."""
    NF = x.shape[2]
    at = lambda k: x[:, :, np.clip(np.arange(NF) + k, 0, NF - 1)]
    parts = [x, (at(1) - at(-1)) / 2.0]
    if order == 2:
        parts.append((2.0 * at(2) + at(1) - at(-1) - 2.0 * at(-2)) / 10.0)
    return np.concatenate(parts, axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("B,C,NF", [(2, 72, 3701), (2, 3, 1), (2, 3, 2), (3, 5, 3), (2, 3, 4), (2, 3, 5)])
def test_delta_orders_and_lengths(order, B, C, NF):
    assert (B * C * NF > GRID_CAP_THREADS) == (NF == 3701)
    x = np.random.Generator(np.random.PCG64(NF)).standard_normal((B, C, NF)).astype(np.float32)
    SENTINEL = -12345.0
    yd = torch.full((B * 3 * C * NF,), SENTINEL, device="cuda")                  # sized for order 2 either way
    _call("dlip_delta_nct_f32", torch.from_numpy(x).cuda().data_ptr(), yd.data_ptr(), B, C, NF, order)
    y = yd.cpu().numpy()
    n = B * (1 + order) * C * NF
    assert rel_err(y[:n].reshape(B, (1 + order) * C, NF), _delta_ref(x.astype(np.float64), order)) < 1e-6
    assert np.all(y[n:] == SENTINEL)                                            # order 1: the third block's room is untouched
    assert np.array_equal(y[:n].reshape(B, (1 + order) * C, NF)[:, :C], x)      # the base block is a copy


@pytest.mark.gpu
@pytest.mark.parametrize("NF", [1, 2, 300])
@pytest.mark.parametrize("with_energy", [False, True])
@pytest.mark.parametrize("normalize", [0, 1])
def test_cmvn_padded_rows_energy_and_raw(NF, with_energy, normalize):
    """C = 24 features in rows of pitch 28 whose padding columns hold NaN (a read of them shows); B * C = 264: two blocks, the
    second partial.  The kernel subtracts the fp32-rounded mean and divides by the fp32-rounded deviation: about
    6e-8 * (1 + |mean| / std) per element, so the inputs keep |mean| / std below ~2 (at NF = 2 the two values of a band are
    u -+ w with w in [0.5, 1.5]: std = w) and 1e-6 of the largest output is a bound with room, not a fit."""
    B, C, ldf = 11, 24, 28
    r = np.random.Generator(np.random.PCG64(100 + NF))
    if NF == 2:
        u, w = 0.3 * r.standard_normal((B, 1, C)), r.uniform(0.5, 1.5, (B, 1, C))
        v = np.concatenate([u - w, u + w], axis=1)
    else:
        v = r.standard_normal((B, NF, C))
    feat = np.full((B, NF, ldf), np.nan, np.float32)
    feat[:, :, :C] = v
    energy = np.exp(v[:, :, 0] if NF == 2 else r.standard_normal((B, NF))).astype(np.float32)
    fd, ed = torch.from_numpy(feat).cuda(), torch.from_numpy(energy).cuda()
    yd = torch.full((B * C * NF + 64,), float("nan"), device="cuda")
    _call("dlip_cmvn_nct_f32", fd.data_ptr(), ed.data_ptr() if with_energy else None, yd.data_ptr(), B, NF, C, ldf, normalize)
    y = yd.cpu().numpy()
    ref = feat[:, :, :C].astype(np.float64)
    if with_energy:
        ref[:, :, 0] = np.log(energy.astype(np.float64))
    if normalize:
        ref = (ref - ref.mean(axis=1, keepdims=True)) / (ref.std(axis=1, keepdims=True) + 2e-12)
    ref = ref.transpose(0, 2, 1)                                                # channel first
    got = y[:B * C * NF].reshape(B, C, NF)
    if NF == 1 and normalize:
        assert np.all(got == 0.0)
    else:
        assert rel_err(got, ref) < 1e-6
    assert np.isnan(y[B * C * NF:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [7, 1, 4, 261])
def test_powspec_rows_padding_and_the_zero_row(R):
    NB, NBp, nfft = 129, 132, 256
    spec = np.random.Generator(np.random.PCG64(R)).standard_normal((R, 2 * NB)).astype(np.float32)
    zero_row = R // 2
    spec[zero_row] = 0.0
    pw = torch.full((R * NBp + 64,), float("nan"), device="cuda")
    en = torch.full((R + 64,), float("nan"), device="cuda")
    _call("dlip_powspec_f32", torch.from_numpy(spec).cuda().data_ptr(), pw.data_ptr(), en.data_ptr(), R, NB, NBp, nfft)
    p, e = pw.cpu().numpy(), en.cpu().numpy()
    s = spec.astype(np.float64)
    ref = (s[:, :NB] ** 2 + s[:, NB:] ** 2) / nfft
    got = p[:R * NBp].reshape(R, NBp)
    assert np.all(got[:, NB:] == 0.0)                                           # the padding columns: exactly zero
    assert np.all(got[zero_row] == 0.0)
    assert rel_err(got[:, :NB], ref) < 1e-6
    eref = ref.sum(axis=1)
    live = np.arange(R) != zero_row
    assert e[zero_row] == np.float32(2.220446049250313e-16)
    if live.any():
        assert rel_err(e[:R][live], eref[live]) < 1e-6
    assert np.isnan(p[R * NBp:]).all() and np.isnan(e[R:]).all()


def _frames_ref(x, NF, L, step, nfft, coef):
    """[B, S] float64 -> [B * NF, nfft]: pre-emphasis (x[0] kept), frames of L samples every step, zeros beyond the signal and
    beyond L.  coef: the fp32 value the entry point is handed."""
    B, S = x.shape
    pre = np.concatenate([x[:, :1], x[:, 1:] - coef * x[:, :-1]], axis=1)
    pad = np.zeros((B, (NF - 1) * step + nfft))
    pad[:, :S] = pre
    out = np.zeros((B, NF, nfft))
    for f in range(NF):
        out[:, f, :L] = pad[:, f * step:f * step + L]
    return out.reshape(B * NF, nfft)


@pytest.mark.gpu
@pytest.mark.parametrize("S,L,step,nfft", [(1, 200, 80, 256), (150, 200, 80, 256), (8037, 200, 80, 256), (54910, 400, 160, 512),
                                            (1000, 128, 64, 128)])
def test_frame_preemph_short_ragged_and_above_the_cap(S, L, step, nfft):
    from deeplip_amd.frontend import num_frames
    B = 3
    NF = num_frames(S, L, step)
    assert (NF - 1) * step + L >= S                                             # (the last frame reaches the signal's end or runs off it)
    if S == 54910:
        assert B * NF * nfft > GRID_CAP_THREADS
    x = np.random.Generator(np.random.PCG64(S)).standard_normal((B, S)).astype(np.float32)
    coef = np.float32(0.97)
    fr = torch.full((B * NF * nfft + 64,), float("nan"), device="cuda")
    _call("dlip_frame_preemph_f32", torch.from_numpy(x).cuda().data_ptr(), fr.data_ptr(), B, S, NF, L, step, nfft, float(coef))
    y = fr.cpu().numpy()
    ref = _frames_ref(x.astype(np.float64), NF, L, step, nfft, float(coef))
    got = y[:B * NF * nfft].reshape(B * NF, nfft)
    assert rel_err(got, ref) < 1e-6
    assert np.all(got[ref == 0.0] == 0.0)                                       # zero padding is exact
    assert np.isnan(y[B * NF * nfft:]).all()


def _crop_ref(frames_u8, crop, oy, ox, flip):
    """[T, H, W] or [T, 3, H, W] uint8 -> [T, crop, crop]: BT.601 gray, / 255, crop at (oy, ox), left-right flip, (x - 0.421) / 0.165,
    in float32 step by step like the oracle's video_preprocess_train_u8."""
    x = frames_u8.astype(np.float32)
    if x.ndim == 4:
        x = np.float32(0.299) * x[:, 0] + np.float32(0.587) * x[:, 1] + np.float32(0.114) * x[:, 2]
    x = (x / np.float32(255.0))[:, oy:oy + crop, ox:ox + crop]
    if flip:
        x = x[:, :, ::-1]
    return ((x - np.float32(0.421)) / np.float32(0.165)).astype(np.float32)


def _crop(frames, T, crop, clip_params=None, lengths=None):
    """dlip_crop_normalize_u8 on [N, (3,) H, W] uint8 frames (N = clips of T) -> [N, crop, crop] + a NaN tail that must survive."""
    N, H, W = frames.shape[0], frames.shape[-2], frames.shape[-1]
    fd = frames.cuda()
    cp = None if clip_params is None else torch.tensor(clip_params, dtype=torch.int32).cuda()
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
    yd = torch.full((N * crop * crop + 64,), float("nan"), device="cuda")
    _call("dlip_crop_normalize_u8", fd.data_ptr(), None if cp is None else cp.data_ptr(), None if ln is None else ln.data_ptr(), T,
          yd.data_ptr(), N, 3 if frames.dim() == 4 else 1, H, W, crop)
    y = yd.cpu().numpy()
    assert np.isnan(y[N * crop * crop:]).all()
    return y[:N * crop * crop].reshape(N, crop, crop)


@pytest.mark.gpu
def test_crop_edges_bit_exact():
    from deeplip_amd.frontend import VideoFrontend
    g = torch.Generator().manual_seed(21)
    # 70 gray frames of 96 x 96 -> 88: 542 080 outputs, the kernel's first launch above the grid cap
    big = torch.randint(0, 256, (70, 96, 96), dtype=torch.uint8, generator=g)
    assert 70 * 88 * 88 > GRID_CAP_THREADS
    assert np.array_equal(_crop(big, 70, 88), O.video_preprocess_u8(big.numpy()))
    # crop == H == W: no margin at all
    full = torch.randint(0, 256, (3, 88, 88), dtype=torch.uint8, generator=g)
    assert np.array_equal(_crop(full, 3, 88), O.video_preprocess_u8(full.numpy()))
    assert np.array_equal(_crop(full, 3, 88, clip_params=[[0, 0, 1, 0]]), _crop_ref(full.numpy(), 88, 0, 0, True))
    # another crop size, RGB, odd margins (7 and 5: CenterCrop takes 3 and 2), through the Python class
    rgb = torch.randint(0, 256, (2, 3, 3, 31, 29), dtype=torch.uint8, generator=g)
    y = VideoFrontend(24)(rgb.cuda())
    torch.cuda.synchronize()
    assert y.shape == (2, 1, 3, 24, 24)
    for b in range(2):
        assert np.array_equal(y[b, 0].cpu().numpy(), O.video_preprocess_u8(rgb[b].numpy(), crop=24))
        assert np.array_equal(y[b, 0].cpu().numpy(), _crop_ref(rgb[b].numpy(), 24, 3, 2, False))
    # crop origins outside the frame are clamped: (-5, 1000) -> (0, W - crop), flipped; (1000, -5) -> (H - crop, 0)
    T, H, W = 2, 91, 95
    clips = torch.randint(0, 256, (2 * T, H, W), dtype=torch.uint8, generator=g)
    y = _crop(clips, T, 88, clip_params=[[-5, 1000, 1, 0], [1000, -5, 0, 0]])
    assert np.array_equal(y[:T], _crop_ref(clips[:T].numpy(), 88, 0, W - 88, True))
    assert np.array_equal(y[T:], _crop_ref(clips[T:].numpy(), 88, H - 88, 0, False))
    # lengths 0, T and T + 3: a clip of zeros, and two clips with every frame valid
    T = 4
    clips = torch.randint(0, 256, (3 * T, 3, 91, 95), dtype=torch.uint8, generator=g)
    y = _crop(clips, T, 88, lengths=[0, T, T + 3])
    assert np.all(y[:T] == 0.0)
    assert np.array_equal(y[T:], O.video_preprocess_u8(clips[T:].numpy()))


@pytest.mark.gpu
def test_entry_points_refuse_on_the_host():
    """Arguments the entry points reject before any launch (DLIP_EINVAL through check())."""
    L = _L()
    buf = torch.zeros(4096, device="cuda")
    u8 = torch.zeros(4 * 3 * 32 * 32, dtype=torch.uint8, device="cuda")
    p, q = buf.data_ptr(), u8.data_ptr()
    with pytest.raises(L.DeepLipHipError, match="invalid argument"):
        _call("dlip_frame_preemph_f32", p, p, 1, 100, 1, 200, 80, 128, 0.97)            # nfft < frame_len
    with pytest.raises(L.DeepLipHipError, match="invalid argument"):
        _call("dlip_delta_nct_f32", p, p, 1, 2, 5, 3)                                   # order = 3
    with pytest.raises(L.DeepLipHipError, match="invalid argument"):
        _call("dlip_crop_normalize_u8", q, None, None, 2, p, 4, 2, 32, 32, 24)          # channels = 2
    with pytest.raises(L.DeepLipHipError, match="invalid argument"):
        _call("dlip_crop_normalize_u8", q, None, None, 2, p, 4, 1, 20, 32, 24)          # H < crop
    with pytest.raises(L.DeepLipHipError, match="invalid argument"):
        _call("dlip_crop_normalize_u8", q, None, None, 3, p, 4, 1, 32, 32, 24)          # n_frames % T != 0
    _call("dlip_crop_normalize_u8", q, None, None, 2, p, 4, 1, 32, 32, 24)              # (the same call, consistent: accepted)
