"""Host-side pieces of the audio front-end's ragged waveform batches (-m "not gpu"): the new entry points in header, binding and
library; length validation in front of any launch; the frame-count batch plan of RaggedExtractor.run(waves=True); SyntheticAVSet's
waveforms (deterministic, framing into audio_len frames) beside features that keep the values they had."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

RAGGED_ENTRY_POINTS = ("dlip_wave_frame_lengths_i32", "dlip_frame_preemph_ragged_f32", "dlip_powspec_wave_fft64_ragged_f32",
                       "dlip_cmvn_nct_ragged_f32", "dlip_delta_nct_ragged_f32")


def test_header_binding_and_library_agree_on_the_ragged_entry_points():
    from deeplip_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "deeplip_hip.h")).read()
    assert int(re.search(r"#define DLIP_ABI_VERSION (\d+)", text).group(1)) == _lib.ABI_VERSION >= 57
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(build.build(verbose=False))
    assert lib.dlip_abi_version() == _lib.ABI_VERSION
    for name in RAGGED_ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
        assert m, f"{name} not declared in deeplip_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert hasattr(lib, name), f"{name} not exported"
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):           # pointers, 32- and 64-bit integers, float / double: each in its place
            want = (_lib.c_f if "*" in a or a.startswith("dlip_stream_t") else _lib.c_i64 if a.startswith("int64_t") else
                    _lib.c_i32 if a.startswith("int32_t") else ctypes.c_double if a.startswith("double") else ctypes.c_float)
            assert c is want, (name, a, c)
    # the rectangular entry points keep the signatures they had
    assert len(_lib.SIGNATURES["dlip_powspec_wave_fft64_f32"]) == 13 and len(_lib.SIGNATURES["dlip_frame_preemph_f32"]) == 10
    assert len(_lib.SIGNATURES["dlip_cmvn_nct_f32"]) == 9 and len(_lib.SIGNATURES["dlip_delta_nct_f32"]) == 7


def test_host_lengths_are_validated_before_the_library_is_touched(monkeypatch):
    from deeplip_amd import _lib, frontend

    def no_library():
        raise AssertionError("the library was reached before the lengths were validated")
    monkeypatch.setattr(frontend, "lib", no_library)
    monkeypatch.setattr(_lib, "lib", no_library)
    fe = frontend.AudioFrontend("mfcc", device="cpu")
    wave = torch.zeros(3, 2160)
    for bad in ([2160, 100], [2160, 100, 50, 7], [2160, 0, 5], [2160, -3, 5], [2161, 5, 5], np.array([1, 2, 4000])):
        with pytest.raises(ValueError):
            fe(wave, bad)
    with pytest.raises(ValueError):
        fe(wave, lengths=torch.tensor([5, 5, 0]))                    # a CPU tensor is host data: validated like a list


def test_device_lengths_must_be_int32():
    """ops.lengths_i32 is what AudioFrontend hands its ``lengths`` to; its device branch needs a device tensor, so the dtype rule is
    shown on a stand-in that only claims to live there."""
    from deeplip_amd import ops

    class OnDevice(torch.Tensor):
        is_cuda = True
    for dt in (torch.int64, torch.float32):
        with pytest.raises(TypeError):
            ops.lengths_i32(torch.zeros(3, dtype=dt).as_subclass(OnDevice), "cuda", n=3, lo=1, hi=10)
    with pytest.raises(ValueError):
        ops.lengths_i32(torch.zeros(4, dtype=torch.int32).as_subclass(OnDevice), "cuda", n=3, lo=1, hi=10)


@pytest.mark.parametrize("L,step", [(400, 160), (200, 80), (551, 221)])
def test_a_rungs_padded_samples_frame_into_the_rungs_frames(L, step):
    """RaggedExtractor.run(waves=True) plans on frame counts and pads a rung of T frames to S = L + (T - 1) step samples:
    num_frames(S) = T, every utterance of the rung fits into S, and S is the LARGEST sample count with T frames."""
    from deeplip_amd.frontend import num_frames
    from deeplip_amd.ragged import plan_batches
    from deeplip_amd.synthetic import SyntheticAVSet
    ds = SyntheticAVSet(4, 6, 1, key="fe.plan", ragged=True, audio_range=(24, 90))
    slen = ds.wave_len(L, step)
    alen = np.array([num_frames(int(s), L, step) for s in slen])
    assert np.array_equal(alen, ds.audio_len)                        # the waveforms frame into the set's own frame counts
    batches = plan_batches(alen, 4, 0.10, 4)
    assert len({b.T for b in batches}) >= 3
    for b in batches:
        S = L + (b.T - 1) * step
        assert num_frames(S, L, step) == b.T and num_frames(S + 1, L, step) == b.T + 1
        assert slen[b.idx].max() <= S and alen[b.idx].max() <= b.T
    for S in range(1, 3 * L):                                         # the device rule (integers) == the host rule (float ceil)
        assert num_frames(S, L, step) == (1 if S <= L else 1 + (S - L + step - 1) // step)


def test_extractor_checks_min_frames_on_host_computed_frame_counts():
    from deeplip_amd.extract import RaggedExtractor
    from deeplip_amd.synthetic import SyntheticAVSet
    ds = SyntheticAVSet(2, 3, 1, key="fe.min", ragged=True, audio_range=(24, 40))
    ex = RaggedExtractor.__new__(RaggedExtractor)                     # (no device: the check runs in front of any pipeline)
    ex.device, ex.batch, ex.clip_batch, ex.waste, ex.aq, ex.vq = "cpu", 4, 4, 0.1, 4, 1
    ex.audio_min_frames, ex.video_min_frames, ex.frame_len, ex.frame_step = int(ds.audio_len.min()) + 1, 1, 400, 160
    ex.pa, ex.pv = object(), None
    with pytest.raises(ValueError, match="speech encoder needs"):
        ex.run(ds, 0, len(ds), 8, waves=True)


def test_synthetic_waveforms_are_deterministic():
    from deeplip_amd.synthetic import SyntheticAVSet
    kw = dict(key="fe.det", ragged=True, audio_range=(5, 30))
    a, b = SyntheticAVSet(3, 2, 1, **kw), SyntheticAVSet(3, 2, 1, **kw)
    assert np.array_equal(a.wave_len(), b.wave_len()) and a.wave_len().dtype == np.int64
    wa, la = a.waves_padded([0, 3, 5])
    wb, lb = b.waves_padded([0, 3, 5])
    assert wa.dtype == np.float32 and la.dtype == np.int32 and np.array_equal(wa, wb) and np.array_equal(la, lb)
    assert np.array_equal(la, a.wave_len()[[0, 3, 5]]) and wa.shape == (3, int(la.max()))
    w2, _ = a.waves_padded([3], S=int(la.max()) + 100)
    assert np.array_equal(w2[0, :la[1]], wa[1, :la[1]]) and not w2[0, la[1]:].any()          # zero padding behind the utterance
    assert np.array_equal(a.wave_item(3), wa[1, :la[1]]) and np.isfinite(wa).all() and 0.1 < np.abs(wa).max() < 10.0
    assert not np.array_equal(a.wave_item(0)[:300], a.wave_item(1)[:300])                     # utterances differ
    other = SyntheticAVSet(3, 2, 1, seed=a.seed + 1, **kw)
    assert not np.array_equal(other.wave_item(0)[:300], a.wave_item(0)[:300])


def test_synthetic_features_keep_their_values():
    """The waveforms draw from a generator key of their own: lengths, clip structure and feature values of a set are what they
    were before the waveforms existed (the hash below was computed with the commit in front of them)."""
    from deeplip_amd.synthetic import SyntheticAVSet
    h = hashlib.sha256()
    ds = SyntheticAVSet(3, 2, clips_per_utt=2, key="hashcheck", ragged=True, audio_range=(30, 60), video_range=(3, 5))
    ds.wave_len(); ds.wave_item(1)                                   # (using the waveforms does not disturb the rest either)
    for a in (ds.audio_len, ds.clip_ptr, ds.clip_len):
        h.update(np.ascontiguousarray(a).tobytes())
    x, L = ds.audio_padded([0, 3, 5])
    h.update(x.tobytes()); h.update(L.tobytes())
    h.update(ds.clip_item(1)[:2, 40:44, 40:44].tobytes())
    rect = SyntheticAVSet(2, 2, audio_frames=20, key="hashcheck")
    h.update(rect.audio([1, 2]).tobytes())
    assert h.hexdigest() == "30017e89c3e55e2b953c02d2ef7f79a41ab8c3896aabd73f8caf6c7c068c0797"
