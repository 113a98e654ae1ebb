"""The ``stft`` feature type, host side (no GPU): the definition, the geometry, the ABI 61 entry points and their refusals.

The loaders' fourth feature type (models/audio_models/datasets.py:72-76) is ``librosa.stft`` -> ``magphase`` -> ``log1p`` with
librosa's defaults (center=True, pad_mode="reflect", window="hann").  ``stft_logmag_ref`` below restates it in fp64 numpy and is the
definition the GPU tests (tests/test_stft_gpu.py) hold the kernel to; here it is itself checked against ``torch.stft`` in fp64, an
independent implementation of the same conventions.  DESIGN.md section 4e."""
import ctypes

import numpy as np
import pytest
import torch

import test_abi_cpu as abi
from deeplip_amd import weightgen as wg
from oracle import deeplip_oracle as O

NAMES = ("dlip_stft_logmag_wave_f32", "dlip_stft_logmag_wave_ragged_f32", "dlip_stft_frame_lengths_i32")
ARITY = {"dlip_stft_logmag_wave_f32": 11, "dlip_stft_logmag_wave_ragged_f32": 12, "dlip_stft_frame_lengths_i32": 7}
GEOMETRIES = ((512, 160, 400, 5040), (128, 40, 100, 257), (128, 40, 100, 65), (1024, 220, 551, 3000), (256, 64, 256, 129))


# ------------------------------------------------------------------------------------------------------------ the definition
def stft_logmag_ref(y, n_fft, hop, win):
    """log1p|librosa.stft(y, n_fft, hop, win)| transposed, [T, F] float64: periodic Hann window of ``win`` points centred in the
    n_fft-point frame, reflect padding by n_fft // 2 (the edge sample not repeated), T = 1 + n // hop frames, rfft."""
    y = np.asarray(y, dtype=np.float64)
    w = np.zeros(n_fft)
    lp = (n_fft - win) // 2
    w[lp:lp + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    T = 1 + y.size // hop
    frames = np.stack([yp[t * hop:t * hop + n_fft] for t in range(T)]) * w
    return np.log1p(np.abs(np.fft.rfft(frames, axis=1)))


def stft_features_ref(y, n_fft, hop, win, normalize=True, delta=False):
    """_extract_feature + _normalize + _delta (datasets.py:52-63,72-82) on the restatement -> channel-first [F (x3), T] float64."""
    feat = stft_logmag_ref(y, n_fft, hop, win)
    if normalize:
        feat = (feat - feat.mean(axis=0)) / (feat.std(axis=0) + 2e-12)
    if delta:
        feat = O.add_deltas(feat, order=2)
    return feat.T


def noise(key, n):
    return (0.1 * wg.gen(key, (n,))).astype(np.float32)


# The noise rows of the NORMALISED parity test (tests/test_stft_gpu.py), per geometry (n_fft, hop, win, S): seeds of
# noise(f"stft.norm.{n_fft}.{S}.{seed}", S) whose spectrogram keeps every bin's deviation over time healthy -- min over bins of
# std / |mean| > 0.05 -- so that the 1e-4 bar is not spent on the cancellation in x - mean.  From seven frames on the first three seeds
# do; at two and three frames a bin's values lie within a few percent of each other by accident in most rows, and the seeds are the
# first that hold, found by walking seed = 0, 1, 2, ... (at S = 80 the first three among 0 .. 10; at S = 129 three among 0 .. 2563;
# at S = 65 two among 0 .. 2298, seed 1742 left out because it holds only by a margin of 1e-5; at S = 79 the only two among 0 .. 2999).
NORM_SEEDS = {(128, 40, 100, 65): (2097, 2298), (128, 40, 100, 79): (86, 333), (128, 40, 100, 80): (3, 8, 10),
              (128, 40, 100, 257): (0, 1, 2), (256, 64, 256, 129): (79, 324, 2563), (256, 64, 256, 1000): (0, 1, 2),
              (1024, 220, 551, 3000): (0, 1, 2), (512, 160, 400, 5040): (0, 1, 2)}


def norm_signals(n_fft, hop, win, S):
    return np.stack([noise(f"stft.norm.{n_fft}.{S}.{seed}", S) for seed in NORM_SEEDS[(n_fft, hop, win, S)]])


@pytest.mark.parametrize("n_fft,hop,win,S", sorted(NORM_SEEDS))
def test_normalised_parity_rows_have_healthy_bins(n_fft, hop, win, S):
    for b, y in enumerate(norm_signals(n_fft, hop, win, S)):
        raw = stft_logmag_ref(y, n_fft, hop, win)
        health = float((raw.std(axis=0) / np.abs(raw.mean(axis=0))).min())
        print(f"({n_fft}, {hop}, {win}, {S}) seed {NORM_SEEDS[(n_fft, hop, win, S)][b]}: min std / |mean| = {health:.4f}")
        assert health > 0.05, b


@pytest.mark.parametrize("n_fft,hop,win,n", GEOMETRIES)
def test_restatement_agrees_with_torch_stft_in_fp64(n_fft, hop, win, n):
    y = noise(f"stft.cpu.{n_fft}.{n}", n).astype(np.float64)
    X = torch.stft(torch.from_numpy(y), n_fft, hop_length=hop, win_length=win, window=torch.hann_window(win, periodic=True, dtype=torch.float64),
                   center=True, pad_mode="reflect", return_complex=True)
    want = torch.log1p(X.abs()).T.numpy()
    got = stft_logmag_ref(y, n_fft, hop, win)
    assert got.shape == want.shape == (1 + n // hop, n_fft // 2 + 1)
    err = float(np.abs(got - want).max())
    print(f"({n_fft}, {hop}, {win}, {n}): max |restatement - torch.stft fp64| = {err:.2e}")
    assert err <= 1e-12


def test_frame_count_rule():
    for n, T in ((64, 2), (65, 2), (79, 2), (80, 3), (119, 3), (120, 4)):
        if n >= 65:                              # (a 128-point frame reflects signals of >= 65 samples)
            assert stft_logmag_ref(np.ones(n), 128, 40, 100).shape[0] == T
        assert 1 + n // 40 == T


def _cpu_frontend(feat, **kw):
    from deeplip_amd.frontend import AudioFrontend
    return AudioFrontend(feat, device="cpu", **kw)


def test_truncated_geometry_at_22050_hz():
    from deeplip_amd.frontend import round_half_up
    fe = _cpu_frontend("stft", rate=22050, nfft=1024)
    assert (fe.hop, fe.win_length) == (220, 551) == (int(22050 * 0.01), int(22050 * 0.025))
    assert (round_half_up(22050 * 0.01), round_half_up(22050 * 0.025)) == (221, 551)
    mel = _cpu_frontend("logfbank", rate=22050, nfft=1024)
    assert (mel.frame_step, mel.frame_len) == (221, 551)
    assert (fe.frame_step, fe.frame_len) == (220, 551)              # the samples a loader's crop is cut by (datasets.py:113-115)
    fe = _cpu_frontend("stft")
    assert (fe.hop, fe.win_length, fe.nfft, fe.nb, fe.nbp) == (160, 400, 512, 257, 260)
    assert fe.feat_dim == 257 and _cpu_frontend("stft", delta=True).feat_dim == 771 and _cpu_frontend("stft", nfft=1024).feat_dim == 513
    assert not any(hasattr(fe, n) for n in ("w_dft", "w_mel", "w_dct"))                    # no matrix is built or uploaded


def test_sample_and_frame_counts_round_trip_for_all_feature_types():
    from deeplip_amd.frontend import num_frames
    for feat, kw in (("stft", {}), ("stft", {"rate": 22050, "nfft": 1024}), ("mfcc", {}), ("fbank", {"rate": 22050, "nfft": 1024}),
                     ("logfbank", {})):
        fe = _cpu_frontend(feat, **kw)
        for T in (2, 3, 30, 32, 401):
            S = fe.samples_for_frames(T)
            assert fe.frames_for_samples(S) == T and fe.frames_for_samples(S + 1) == T + 1, (feat, T)     # the longest such signal
        if feat == "stft":
            assert fe.frames_for_samples(5040) == 1 + 5040 // fe.hop and fe.samples_for_frames(4) == 4 * fe.hop - 1
        else:
            assert fe.frames_for_samples(5040) == num_frames(5040, fe.frame_len, fe.frame_step)
            assert fe.samples_for_frames(4) == fe.frame_len + 3 * fe.frame_step
    # the shipped geometry: a crop of 30 frames is 5040 samples (collate_fn) and gives 32 spectrogram frames
    fe = _cpu_frontend("stft")
    assert fe.frame_len + 29 * fe.frame_step == 5040 and fe.frames_for_samples(5040) == 32


def test_constructor_refusals_come_before_any_upload():
    for bad in (64, 2048, 500, 0):
        with pytest.raises(ValueError, match="power of two"):
            _cpu_frontend("stft", nfft=bad)
    with pytest.raises(ValueError, match="window"):
        _cpu_frontend("stft", nfft=256)                                                    # 400-sample window
    for kw in ({"dft": "gemm32"}, {"dft": "direct64"}, {"dft64": True}, {"dft64": False}):
        with pytest.raises(ValueError, match="fft64"):
            _cpu_frontend("stft", **kw)
    with pytest.raises(ValueError):
        _cpu_frontend("stft", win_shift=1e-6)
    assert _cpu_frontend("stft", dft="fft64").dft == "fft64"
    with pytest.raises(NotImplementedError):
        _cpu_frontend("spectrogram")


def test_extractor_takes_the_frontend_as_its_wave_geometry():
    from deeplip_amd.extract import RaggedExtractor
    from deeplip_amd.frontend import num_frames
    ex = RaggedExtractor(None, None, torch.device("cpu"), wave_geometry=(400, 160))
    assert (ex.frame_len, ex.frame_step) == (400, 160)
    assert ex._frames_for(5040) == num_frames(5040, 400, 160) == 30 and ex._samples_for(30) == 5040
    fe = _cpu_frontend("stft", nfft=128, rate=4000)
    ex = RaggedExtractor(None, None, torch.device("cpu"), wave_geometry=fe)
    assert (ex.frame_len, ex.frame_step) == (100, 40)
    assert ex._frames_for(257) == 7 and ex._samples_for(7) == 279 and ex._frames_for(279) == 7


def test_extractor_refuses_utterances_shorter_than_the_frontend_takes():
    """The sample counts reach the kernels as a device vector, which clamps: the minimum is checked on the host, before any batch."""
    from deeplip_amd.extract import RaggedExtractor
    from deeplip_amd.synthetic import SyntheticAVSet
    ds = SyntheticAVSet(2, 3, 1, key="stft.min", ragged=True, audio_range=(1, 3))
    fe = _cpu_frontend("stft", nfft=512, rate=4000)                        # window 100, hop 40: the set's utterances have <= 180 samples
    assert fe.min_samples == 257 and _cpu_frontend("mfcc").min_samples == 1 and int(ds.wave_len(100, 40).max()) < 257
    ex = RaggedExtractor(None, None, torch.device("cpu"), wave_geometry=fe)
    ex.pa = object()                                                       # (no device: the check runs in front of any pipeline)
    with pytest.raises(ValueError, match="front-end needs >= 257"):
        ex.run(ds, 0, len(ds), 8, waves=True)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_exported_and_bound():
    from deeplip_amd import _lib, build
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.HEADER["DLIP_ABI_VERSION"] == _lib.ABI_VERSION >= 61
    for n in NAMES:
        assert n in abi.header_symbols() and hasattr(lib, n), n
        assert len(_lib.SIGNATURES[n]) == ARITY[n], n
        assert all(t in (_lib.c_f, _lib.c_i32, _lib.c_i64) for t in _lib.SIGNATURES[n]), n     # device pointers and integers only
        assert _lib.PROTOTYPES[n][0] is ctypes.c_int, n


def test_refuses_bad_arguments_on_the_host():
    """Every refusal of the header's list returns DLIP_EINVAL in front of any device call: dummy addresses, nothing dereferenced, no
    launch (each call below is a refused one)."""
    from deeplip_amd import _lib
    l = _lib.lib()
    EINVAL = _lib.HEADER["DLIP_EINVAL"]
    p = 4096
    ok = dict(x=p, out=p, B=2, S=300, NF=8, win=100, hop=40, n_fft=128, F=65, Fp=68)

    def rect(**kw):
        a = dict(ok, **kw)
        return l.dlip_stft_logmag_wave_f32(a["x"], a["out"], a["B"], a["S"], a["NF"], a["win"], a["hop"], a["n_fft"], a["F"], a["Fp"], None)

    def ragged(slen=p, **kw):
        a = dict(ok, **kw)
        return l.dlip_stft_logmag_wave_ragged_f32(a["x"], slen, a["out"], a["B"], a["S"], a["NF"], a["win"], a["hop"], a["n_fft"], a["F"],
                                                  a["Fp"], None)
    bad = [dict(x=None), dict(out=None), dict(B=0),
           dict(n_fft=64, F=33, Fp=36, win=50), dict(n_fft=2048, F=1025, Fp=1028, S=2000, NF=51), dict(n_fft=192, F=97, Fp=100),
           dict(win=0), dict(win=129), dict(hop=0), dict(hop=-40),
           dict(S=64, NF=2), dict(NF=7), dict(NF=9), dict(F=64), dict(F=66), dict(Fp=64)]
    for kw in bad:
        assert rect(**kw) == EINVAL, kw
        assert ragged(**kw) == EINVAL, kw
    assert ragged(slen=None) == EINVAL
    fl = l.dlip_stft_frame_lengths_i32
    assert fl(None, p, 2, 300, 128, 40, None) == EINVAL and fl(p, None, 2, 300, 128, 40, None) == EINVAL
    assert fl(p, p, 0, 300, 128, 40, None) == EINVAL and fl(p, p, 2, 64, 128, 40, None) == EINVAL
    assert fl(p, p, 2, 300, 100, 40, None) == EINVAL and fl(p, p, 2, 3000, 2048, 40, None) == EINVAL
    assert fl(p, p, 2, 300, 128, 0, None) == EINVAL


def test_cpu_tensors_are_refused():
    from deeplip_amd._lib import DeepLipHipError
    fe = _cpu_frontend("stft", nfft=128, rate=4000)
    with pytest.raises(DeepLipHipError):
        fe(torch.zeros(2, 300))
    with pytest.raises(DeepLipHipError):
        fe(torch.zeros(2, 300), [300, 65])
