"""Seeded synthetic A+V data with the shapes the reference's loaders produce
(models/fusion_models/datasets.py:115-156: ``(feats_video: list[list[np[T,88,88]]], feats_audio
[B,F,T], labels [B])``; test sets yield one utterance at a time) and trial lists shaped like
database/trial_grid_v1.txt (20 000 lines, 4 000 target / 16 000 non-target).  There is no network
and no dataset in this environment; the reference's disk/codec-bound loaders are out of scope
(SURVEY.md section 2.1 #13-15)."""
from __future__ import annotations

from typing import List, Tuple

import zlib

import numpy as np
import torch

from . import weightgen as wg


class SyntheticAVSet:
    """``n_spk`` speakers x ``utt_per_spk`` utterances; utterance u has ``clips_per_utt`` lip clips
    [T,88,88] and one [F,Ta] feature matrix; the speaker shapes both modalities.

    ``ragged=True``: what a real test list looks like (25 834 utterances of differing duration; long videos
    pre-split into several clip files per utterance, models/fusion_models/datasets.py:143-150) -- utterance u has its own number
    of audio frames in ``audio_range`` and 1 .. ``clips_per_utt`` clips, each with its own length in ``video_range``, all drawn
    from a generator keyed by (key, seed).  ``audio_len`` [N], ``clip_len`` [Nc], ``clip_ptr`` [N+1] (CSR: the clips of
    utterance u are clip_ptr[u] .. clip_ptr[u+1]) describe the set; ``audio_item`` / ``clip_item`` yield single items at their own
    length (the reference's loop), ``audio_padded`` / ``clips_padded`` the zero-padded batches of pad_packed_collate.  ``wave_len`` /
    ``wave_item`` / ``waves_padded``: the same utterances as waveforms, for pipelines that start in front of the feature extraction."""

    def __init__(self, n_spk: int, utt_per_spk: int, clips_per_utt: int = 1, video_frames: int = 29,
                 audio_dim: int = 24, audio_frames: int = 300, key: str = "synth", seed: int = wg.DEFAULT_SEED,
                 ragged: bool = False, audio_range: Tuple[int, int] = (137, 412), video_range: Tuple[int, int] = (11, 75),
                 session: float = 1.0, jitter: float = 1.0):
        self.n_spk, self.utt_per_spk, self.clips = n_spk, utt_per_spk, clips_per_utt
        self.T, self.F, self.Ta, self.key, self.seed = video_frames, audio_dim, audio_frames, key, seed
        # every utterance of a speaker shares the speaker's generator (weightgen: key + ".spk<s>") and has its own utterance
        # generator (utt_ids); ``session`` / ``jitter`` = the per-utterance variability beside the speaker's (weightgen.audio_input /
        # video_input) -- they set how separable the speakers are, i.e. where a trial list's EER lands
        self.session, self.jitter = float(session), float(jitter)
        self.utts = [(s, u) for s in range(n_spk) for u in range(utt_per_spk)]
        # ids are prefix-free (zero-padded utterance index): the reference's readers glob ``<pattern>*`` for an utterance's clip
        # files (models/fusion_models/utils.py:456-463), so "s3_u1" must not be a prefix of "s3_u10"
        w = max(2, len(str(max(utt_per_spk - 1, 0))))
        self.utt_ids = [f"s{s}/s{s}_u{u:0{w}d}.wav" for s, u in self.utts]
        self.ragged = bool(ragged)
        n = len(self.utts)
        if self.ragged:
            r = np.random.Generator(np.random.PCG64([int(seed) & 0xFFFFFFFF, zlib.crc32((key + ".ragged").encode())]))
            self.audio_len = r.integers(audio_range[0], audio_range[1] + 1, size=n).astype(np.int64)
            n_clips = r.integers(1, clips_per_utt + 1, size=n) if clips_per_utt > 0 else np.zeros((n,), dtype=np.int64)
            self.clip_ptr = np.concatenate([[0], np.cumsum(n_clips)]).astype(np.int32)
            self.clip_len = r.integers(video_range[0], video_range[1] + 1, size=int(self.clip_ptr[-1])).astype(np.int64)
        else:
            self.audio_len = np.full((n,), audio_frames, dtype=np.int64)
            self.clip_ptr = (np.arange(n + 1) * clips_per_utt).astype(np.int32)
            self.clip_len = np.full((n * clips_per_utt,), video_frames, dtype=np.int64)
        self.clip_utt = np.repeat(np.arange(n), np.diff(self.clip_ptr))          # clip -> its utterance

    def __len__(self):
        return len(self.utts)

    def labels(self, idx) -> np.ndarray:
        return np.array([self.utts[i][0] for i in idx], dtype=np.int64)

    # ---- single items at their own length (what the reference's test loop feeds, train_fusion.py:334-349)
    def audio_item(self, i: int) -> np.ndarray:
        """[F, audio_len[i]]"""
        return wg.audio_input(1, self.F, int(self.audio_len[i]), self.seed, key=f"{self.key}.a", speakers=[self.utts[i][0]],
                              utt_ids=[i], session=self.session)[0]

    def clip_item(self, c: int) -> np.ndarray:
        """[clip_len[c], 88, 88] normalised gray"""
        u = int(self.clip_utt[c])
        k = c - int(self.clip_ptr[u])
        return wg.video_input(1, int(self.clip_len[c]), 88, self.seed, key=f"{self.key}.v", speakers=[self.utts[u][0]],
                              utt_ids=[f"{u}.{k}"], jitter=self.jitter)[0, 0]

    # ---- zero-padded batches + lengths (pad_packed_collate, models/video_models/dataset.py:123-139)
    def audio_padded(self, idx, T: int = None, rows: int = None) -> Tuple[np.ndarray, np.ndarray]:
        from .ragged import pad_stack
        items = [self.audio_item(i) for i in idx]
        L = np.array([it.shape[1] for it in items], dtype=np.int32)
        return pad_stack(items, int(T or L.max()), axis=1, rows=rows), L

    def clips_padded(self, clip_idx, T: int = None, rows: int = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> ([n,1,T,88,88], lengths [n])"""
        from .ragged import pad_stack
        items = [self.clip_item(c)[None] for c in clip_idx]                      # [1,T_c,88,88]
        L = np.array([it.shape[1] for it in items], dtype=np.int32)
        return pad_stack(items, int(T or L.max()), axis=1, rows=rows), L

    # ---- waveforms: what the GPU front-end starts from (deeplip_amd/frontend.py; the reference's loaders read .wav files and compute
    #      the features per utterance on the host, models/audio_models/datasets.py:65-83).  A generator key of their own
    #      (key + ".wave"): the feature tensors above keep their values.
    def wave_len(self, frame_len: int = 400, frame_step: int = 160) -> np.ndarray:
        """Sample counts [N] int64: utterance u has a duration that frames into exactly ``audio_len[u]`` frames of ``frame_len`` /
        ``frame_step`` samples (sigproc.framesig) and, the single-frame ones apart, does not end on the frame grid -- its last frame
        is partly zero padding, as a real recording's is."""
        r = np.random.Generator(np.random.PCG64([int(self.seed) & 0xFFFFFFFF, zlib.crc32((self.key + ".wave").encode())]))
        cut = r.integers(0, frame_step, size=len(self.utts)).astype(np.int64)             # samples short of the frame grid
        full = frame_len + (self.audio_len - 1) * frame_step
        return np.where(self.audio_len > 1, full - cut, np.maximum(frame_len - cut, 1)).astype(np.int64)

    def wave_item(self, i: int, frame_len: int = 400, frame_step: int = 160) -> np.ndarray:
        """[wave_len[i]] float32: three partials whose frequencies and weights belong to the speaker, phases and noise to the utterance."""
        n = int(self.wave_len(frame_len, frame_step)[i])
        gen = lambda tag: np.random.Generator(np.random.PCG64([int(self.seed) & 0xFFFFFFFF, zlib.crc32(f"{self.key}.wave.{tag}".encode())]))
        spk, utt = gen(f"spk{self.utts[i][0]}"), gen(f"utt{i}")
        w = 2.0 * np.pi * spk.uniform(0.005, 0.2, size=3)                                # radians per sample
        amp = spk.uniform(0.2, 1.0, size=3)
        t = np.arange(n, dtype=np.float64)
        x = (amp[:, None] * np.sin(w[:, None] * t[None, :] + utt.uniform(0.0, 2.0 * np.pi, size=3)[:, None])).sum(0)
        return (x + 0.1 * self.session * utt.standard_normal(n)).astype(np.float32)

    def waves_padded(self, idx, S: int = None, rows: int = None, frame_len: int = 400, frame_step: int = 160) -> Tuple[np.ndarray, np.ndarray]:
        """-> (wave [n, S] float32 zero-padded, sample_lengths int32 [n])"""
        from .ragged import pad_stack
        items = [self.wave_item(i, frame_len, frame_step) for i in idx]
        L = np.array([it.shape[0] for it in items], dtype=np.int32)
        return pad_stack(items, int(S or L.max()), axis=0, rows=rows), L

    # ---- rectangular batches (every item the same length)
    def audio(self, idx) -> np.ndarray:
        if self.ragged:
            raise ValueError("SyntheticAVSet.audio: a ragged set has no rectangular batches; use audio_padded / audio_item")
        spk = [self.utts[i][0] for i in idx]
        out = np.empty((len(idx), self.F, self.Ta), dtype=np.float32)
        for j, i in enumerate(idx):
            out[j] = wg.audio_input(1, self.F, self.Ta, self.seed, key=f"{self.key}.a", speakers=[spk[j]], utt_ids=[i],
                                    session=self.session)[0]
        return out

    def video(self, idx) -> Tuple[np.ndarray, np.ndarray]:
        """All clips of the utterances in ``idx`` as one [G,1,T,88,88] batch + CSR group offsets."""
        if self.ragged:
            raise ValueError("SyntheticAVSet.video: a ragged set has no rectangular batches; use clips_padded / clip_item")
        clips, ptr = [], [0]
        for i in idx:
            s = self.utts[i][0]
            for c in range(self.clips):
                clips.append(wg.video_input(1, self.T, 88, self.seed, key=f"{self.key}.v", speakers=[s], utt_ids=[f"{i}.{c}"],
                                            jitter=self.jitter)[0])
            ptr.append(len(clips))
        return np.stack(clips), np.asarray(ptr, dtype=np.int32)


def noise_bank(seconds: float = 5.0, rate: int = 16000, key: str = "augment.noise", seed: int = wg.DEFAULT_SEED) -> np.ndarray:
    """A noise recording for deeplip_amd.augment.WaveAugment: [seconds * rate] float32 coloured noise -- white noise through a
    one-pole low-pass (most of its power below 1 kHz, as room and babble noise have) under a slow amplitude swell, so that two
    slices of it differ in power as slices of a real recording do."""
    n = int(round(seconds * rate))
    w = wg.gen(key, (n,), seed).astype(np.float64)
    x = np.empty(n)
    acc = 0.0
    for i in range(n):                       # y[i] = 0.9 y[i-1] + w[i]
        acc = 0.9 * acc + w[i]
        x[i] = acc
    x *= 0.1 * (1.0 + 0.5 * np.sin(2.0 * np.pi * np.arange(n) / (0.7 * rate)))
    return x.astype(np.float32)


def room_responses(n: int = 6, rate: int = 16000, key: str = "augment.rir", seed: int = wg.DEFAULT_SEED,
                   longest: int = 9000) -> List[np.ndarray]:
    """``n`` synthetic room impulse responses of differing length: a unit direct path after a small delay (0 .. 3 ms), then noise
    decaying exponentially (60 dB over the response's length).  The lengths run from 50 ms up to ``longest`` samples -- by default
    longer than WaveAugment's ``max_taps`` of 8192, so the set exercises the truncation."""
    out = []
    shortest = int(0.05 * rate)
    for i in range(n):
        L = longest if i == n - 1 else int(shortest * (longest / shortest) ** (i / max(n - 1, 1)))
        delay = (7 * i) % max(int(0.003 * rate), 1)
        h = 0.1 * wg.gen(f"{key}.{i}", (L,), seed).astype(np.float64) * np.exp(-6.9 * np.arange(L) / L)
        h[:delay] = 0.0
        h[delay] = 1.0
        out.append(h.astype(np.float32))
    return out


def frames_u8_from_clips(clips: np.ndarray, rgb: bool = True) -> np.ndarray:
    """Normalised float clips [G,1,T,H,W] -> the uint8 frames a loader would have held before dataloaders.py:17-24 normalised
    them: gray = round(255 * (x * 0.165 + 0.421)), as [G,T,3,H,W] RGB with R = G = B (BASELINE.json's input shape) or
    [G,T,H,W] gray.  (The engine's ingest of these frames gives the clip back up to the uint8 quantisation.)"""
    g = np.clip(np.rint((clips[:, 0].astype(np.float64) * 0.165 + 0.421) * 255.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2)) if rgb else g


def synthetic_trials(dataset: SyntheticAVSet, n_trials: int = 20000, n_target: int = 4000, seed: int = 3):
    """(labels [n], pairs [(utt1, utt2)]) with the target / non-target split of trial_grid_v1.txt."""
    r = np.random.Generator(np.random.PCG64(seed))
    by_spk = {}
    for i, (s, _) in enumerate(dataset.utts):
        by_spk.setdefault(s, []).append(i)
    spks = sorted(by_spk)
    y, pairs = [], []
    for t in range(n_trials):
        if t < n_target:
            s = spks[r.integers(len(spks))]
            a, b = r.choice(by_spk[s], 2, replace=len(by_spk[s]) < 2)
            y.append(1)
        else:
            s1, s2 = r.choice(len(spks), 2, replace=False)
            a = by_spk[spks[s1]][r.integers(len(by_spk[spks[s1]]))]
            b = by_spk[spks[s2]][r.integers(len(by_spk[spks[s2]]))]
            y.append(0)
        pairs.append((dataset.utt_ids[a], dataset.utt_ids[b]))
    perm = r.permutation(n_trials)
    return np.asarray(y, dtype=np.int64)[perm], [pairs[i] for i in perm]
