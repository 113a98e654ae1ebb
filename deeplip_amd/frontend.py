"""GPU-side preprocessing in front of the encoders.

``AudioFrontend`` turns waveforms [B, S] (with ``lengths``: a zero-padded batch of utterances of differing duration, each row
computed as if run alone -- DESIGN.md section 4c) into the [B, F, T] feature tensors the reference's loaders
produce with python_speech_features (models/audio_models/datasets.py:65-83: ``mfcc`` / ``fbank`` /
``logfbank`` with winlen 0.025, winstep 0.01; conf/fusion_config.yaml:8-40), followed by the
per-utterance mean/variance normalisation of datasets.py:52-53.  The 512-point real DFT, the mel
filterbank and the DCT-II(+lifter) are three fp32 MFMA GEMMs against constant matrices built once
on the host in fp64; framing/pre-emphasis, power spectrum, log and CMVN are small HIP kernels.
The loaders' fourth feature type, ``stft`` (datasets.py:72-76: log1p of the magnitude of librosa.stft), is one kernel from the
waveform to the log-magnitude rows, in fp64, with the same CMVN and deltas behind it.

``VideoFrontend`` is the test-time pipeline of models/video_models/dataloaders.py:11-22
(Normalize(0,255) -> CenterCrop(88) -> Normalize(0.421, 0.165)) on uint8 gray or RGB frames plus the
zero-pad collate of models/video_models/dataset.py:123-139.
"""
from __future__ import annotations

import decimal
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._lib import call
from ._lib import lib    # noqa: F401  (a test replaces it to show that nothing reaches the library)


def hz2mel(hz):
    return 2595.0 * np.log10(1.0 + hz / 700.0)


def mel2hz(mel):
    return 700.0 * (10.0 ** (mel / 2595.0) - 1.0)


def mel_filterbank(nfilt: int, nfft: int, rate: int, lowfreq: float = 0.0, highfreq: Optional[float] = None) -> np.ndarray:
    """python_speech_features.base.get_filterbanks: [nfilt, nfft//2+1] triangular filters on FFT bins
    floor((nfft+1)*hz/rate)."""
    highfreq = highfreq or rate / 2
    melpoints = np.linspace(hz2mel(lowfreq), hz2mel(highfreq), nfilt + 2)
    bins = np.floor((nfft + 1) * mel2hz(melpoints) / rate)
    fb = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fb


def round_half_up(x: float) -> int:
    """sigproc.round_half_up: ties go up (220.5 -> 221, 1102.5 -> 1103), where Python's round() takes them to the even
    neighbour.  Decided on the exact value of the double, as the package does."""
    return int(decimal.Decimal(x).quantize(decimal.Decimal("1"), rounding=decimal.ROUND_HALF_UP))


def num_frames(n_samples: int, frame_len: int, frame_step: int) -> int:
    """sigproc.framesig: 1 + ceil((slen - frame_len) / frame_step) for slen > frame_len, else 1."""
    return 1 if n_samples <= frame_len else 1 + int(math.ceil((1.0 * n_samples - frame_len) / frame_step))


class AudioFrontend:
    def __init__(self, feat_type: str = "mfcc", rate: int = 16000, win_len: float = 0.025, win_shift: float = 0.01,
                 nfft: int = 512, num_bin: int = 26, num_cep: int = 24, preemph: float = 0.97, ceplifter: int = 22,
                 energy: bool = True, normalize: bool = True, delta: bool = False, dft64: Optional[bool] = None, device="cuda",
                 dft: Optional[str] = None):
        if feat_type not in ("mfcc", "fbank", "logfbank", "stft"):
            raise NotImplementedError("Other features are not implemented!")   # datasets.py:75-76
        self.feat_type, self.rate, self.nfft = feat_type, rate, nfft
        if feat_type == "stft":
            self._init_stft(win_len, win_shift, normalize, delta, dft64, dft, device)
            return
        # sigproc.framesig rounds half UP: 22.05 kHz steps by 220.5 -> 221 samples and 44.1 kHz frames 1102.5 -> 1103, where
        # round() (half to even) gave 220 and 1102 -- another number of frames than the reference's loader produces
        self.frame_len = round_half_up(win_len * rate)
        self.frame_step = round_half_up(win_shift * rate)
        if self.frame_len < 1 or self.frame_step < 1:
            raise ValueError(f"AudioFrontend: win_len * rate and win_shift * rate must round to at least one sample, got "
                             f"{self.frame_len} and {self.frame_step}")
        if nfft < self.frame_len:
            raise ValueError(f"AudioFrontend: nfft must be >= the frame length ({self.frame_len} samples = win_len {win_len} s at "
                             f"{rate} Hz), got nfft={nfft}")
        self.num_bin, self.num_cep, self.preemph, self.normalize, self.energy = num_bin, num_cep, preemph, normalize, energy
        self.delta = delta            # datasets.py:81-82: [feat | delta(N=1) | delta(N=2)] after the normalisation
        # How the power spectrum is formed (``dft``):
        #   "fft64"    (default since ABI 46) pre-emphasis, framing and a radix-2 FFT in fp64, one launch from the waveform
        #              (dlip_powspec_wave_fft64_f32) -- the reference's own precision (numpy on doubles), every band of every frame at 1e-4;
        #   "gemm32"   fp32 pre-emphasis + the DFT as an fp32 MFMA GEMM (rounds 1 - 5's default): elements holding ~1e-12 of a frame's
        #              energy come out 0.3 .. 1 % off (tools/probes/frontend_fuzz.py); kept for A/B runs and as a second implementation;
        #   "direct64" fp32 pre-emphasis + a direct fp64 DFT (round 2's route for banks denser than 60 bands).
        # ``dft64`` (rounds 2 - 5's switch): True -> "direct64", False -> "gemm32".
        if dft is None:
            dft = "fft64" if dft64 is None else ("direct64" if dft64 else "gemm32")
        if dft not in ("fft64", "gemm32", "direct64"):
            raise ValueError(f"AudioFrontend: dft must be 'fft64', 'gemm32' or 'direct64', got {dft!r}")
        if dft == "fft64" and (nfft < 128 or nfft > 1024 or nfft & (nfft - 1)):
            dft = "gemm32"            # (the FFT kernel takes powers of two 128 .. 1024; any other nfft keeps the GEMM route)
        if dft == "direct64" and (nfft < 2 or nfft > 1024 or nfft & (nfft - 1)):
            raise ValueError(f"AudioFrontend: dft='direct64' needs nfft to be a power of two <= 1024, got nfft={nfft}")
        if dft == "gemm32" and nfft % 4:
            raise ValueError(f"AudioFrontend: dft='gemm32' needs nfft to be a multiple of 4 (the GEMM's reduction length), got nfft={nfft}")
        self.dft = dft
        self.dft64 = dft == "direct64"
        self.device = torch.device(device)
        nb = nfft // 2 + 1
        self.nb, self.nbp = nb, (nb + 3) // 4 * 4
        k = np.arange(nb)[:, None] * np.arange(nfft)[None, :] * (2.0 * np.pi / nfft)
        dft = np.concatenate([np.cos(k), -np.sin(k)], 0)                       # [2*nb, nfft]: re | im
        fb = np.zeros((num_bin, self.nbp)); fb[:, :nb] = mel_filterbank(num_bin, nfft, rate)
        self.nfp = (num_bin + 3) // 4 * 4
        self.w_dft = torch.from_numpy(dft).float().contiguous().to(self.device)
        self.w_mel = torch.from_numpy(fb).float().contiguous().to(self.device)
        if feat_type == "mfcc":
            n = np.arange(num_bin)
            dct = np.cos(np.pi * np.arange(num_cep)[:, None] * (2 * n[None, :] + 1) / (2.0 * num_bin))   # DCT-II
            dct *= np.sqrt(2.0 / num_bin); dct[0] *= np.sqrt(0.5)                                          # norm='ortho'
            lift = 1.0 + (ceplifter / 2.0) * np.sin(np.pi * np.arange(num_cep) / ceplifter) if ceplifter > 0 else np.ones(num_cep)
            d = np.zeros((num_cep, self.nfp)); d[:, :num_bin] = dct * lift[:, None]                        # lifter folded in
            self.w_dct = torch.from_numpy(d).float().contiguous().to(self.device)

    def _init_stft(self, win_len, win_shift, normalize, delta, dft64, dft, device):
        """``stft`` (datasets.py:72-76): librosa.stft(y, n_fft, hop_length=int(rate * win_shift), win_length=int(rate * win_len)) ->
        magphase -> log1p.  hop and window TRUNCATE, as the loader's own line does (22.05 kHz: 220 and 551, where framesig's
        round_half_up gives 221 and 551); num_bin / num_cep / preemph / ceplifter / energy do not enter, and no mel, DFT or DCT matrix
        is built or uploaded: one kernel goes from the waveform to log1p|X| (dlip_stft_logmag_wave_f32, fp64 inside), CMVN and deltas
        are the other feature types' kernels.  ``frame_len`` / ``frame_step`` name the window and the hop in samples, the numbers a
        loader's crop is cut by (collate_fn, datasets.py:113-115)."""
        nfft, rate = self.nfft, self.rate
        self.hop, self.win_length = int(rate * win_shift), int(rate * win_len)
        if self.win_length < 1 or self.hop < 1:
            raise ValueError(f"AudioFrontend: int(rate * win_len) and int(rate * win_shift) must be at least one sample, got "
                             f"{self.win_length} and {self.hop}")
        if nfft < 128 or nfft > 1024 or nfft & (nfft - 1):
            raise ValueError(f"AudioFrontend: feat_type 'stft' needs nfft to be a power of two in 128 .. 1024, got nfft={nfft}")
        if nfft < self.win_length:
            raise ValueError(f"AudioFrontend: nfft must be >= the window ({self.win_length} samples = win_len {win_len} s at {rate} Hz), "
                             f"got nfft={nfft}")
        if dft64 is not None or dft not in (None, "fft64"):
            raise ValueError(f"AudioFrontend: feat_type 'stft' has the one transform 'fft64' (dft=None or 'fft64', dft64=None), got "
                             f"dft={dft!r}, dft64={dft64!r}")
        self.frame_len, self.frame_step = self.win_length, self.hop
        self.normalize, self.delta = normalize, delta
        self.dft, self.dft64 = "fft64", False
        self.device = torch.device(device)
        nb = nfft // 2 + 1
        self.nb, self.nbp = nb, (nb + 3) // 4 * 4

    @property
    def feat_dim(self) -> int:
        if self.feat_type == "stft":
            return (3 if self.delta else 1) * self.nb
        return (3 if self.delta else 1) * (self.num_cep if self.feat_type == "mfcc" else self.num_bin)

    @property
    def min_samples(self) -> int:
        """The shortest utterance the front-end takes: one sample, resp. nfft // 2 + 1 for ``stft`` (one reflection per side)."""
        return self.nfft // 2 + 1 if self.feat_type == "stft" else 1

    def frames_for_samples(self, n: int) -> int:
        """Frames of an n-sample utterance: sigproc.framesig's count, resp. librosa.stft's 1 + n // hop (center=True)."""
        if self.feat_type == "stft":
            return 1 + int(n) // self.hop
        return num_frames(int(n), self.frame_len, self.frame_step)

    def samples_for_frames(self, T: int) -> int:
        """The longest signal that has T frames: a batch padded to it comes out [B, F, T]."""
        if self.feat_type == "stft":
            return int(T) * self.hop - 1
        return self.frame_len + (int(T) - 1) * self.frame_step

    def _call_stft(self, wave: torch.Tensor, lengths=None):
        ops._req(wave, "AudioFrontend('stft'): wave")
        B, S = wave.shape
        lo = self.min_samples                   # one reflection per side must reach every sample of a frame
        if S < lo:
            raise ValueError(f"AudioFrontend('stft'): the batch must be at least nfft // 2 + 1 = {lo} samples wide, got {S}")
        lens = ops.lengths_i32(lengths, wave.device, n=B, lo=lo, hi=S)
        NF = 1 + S // self.hop
        C_ = self.nb
        geom = (NF, self.win_length, self.hop, self.nfft, C_, self.nbp)
        feat = ops._empty((B * NF, self.nbp), wave.device)
        out = ops._empty((B, C_, NF), wave.device)
        nf = None
        if lens is None:
            call("dlip_stft_logmag_wave_f32", wave, feat, B, S, *geom)
            call("dlip_cmvn_nct_f32", feat, None, out, B, NF, C_, self.nbp, int(self.normalize))
        else:
            call("dlip_stft_logmag_wave_ragged_f32", wave, lens, feat, B, S, *geom)
            nf = ops._empty((B,), wave.device, torch.int32)
            call("dlip_stft_frame_lengths_i32", lens, nf, B, S, self.nfft, self.hop)
            call("dlip_cmvn_nct_ragged_f32", feat, None, nf, out, B, NF, C_, self.nbp, int(self.normalize))
        return self._deltas(out, nf, B, C_, NF, lens is None)

    def _deltas(self, out, nf, B, C_, NF, rect):
        if self.delta:
            out3 = ops._empty((B, 3 * C_, NF), out.device)
            if rect:
                call("dlip_delta_nct_f32", out, out3, B, C_, NF, 2)
            else:
                call("dlip_delta_nct_ragged_f32", out, nf, out3, B, C_, NF, 2)
            out = out3
        return out if rect else (out, nf)

    def __call__(self, wave: torch.Tensor, lengths=None):
        """wave [B, S] float32 (cuda) -> features [B, F, NF] float32.

        ``lengths`` (B sample counts in [1, S] as a sequence / numpy array, or an int32 device tensor [B]): a RAGGED batch -- wave is
        padded to S samples and row b holds lengths[b] of them.  Returns ``(features [B, F, NF], frame_lengths int32 device [B])`` with
        NF = num_frames(S): row b's columns [0, frame_lengths[b]) equal ``self(wave[b:b+1, :lengths[b]])``, the reference's
        one-utterance-at-a-time loop (train_fusion.py:334-349, train_audio.py:343-373), whatever the padding holds (it is never read:
        the reference pre-emphasises the utterance's own samples and zero-pads afterwards); columns past them are zeros.  Host lengths
        are validated here; a device vector is clamped by the kernels and never read on the host, and nothing below synchronises, so
        the call records into a step plan (deeplip_amd/plan.py) and ``frame_lengths`` is the encoders' ``lengths``."""
        wave = wave.contiguous().float()
        if self.feat_type == "stft":
            return self._call_stft(wave, lengths)
        B, S = wave.shape
        lens = ops.lengths_i32(lengths, wave.device, n=B, lo=1, hi=S)           # None: the rectangular batch, no length is read
        NF = num_frames(S, self.frame_len, self.frame_step)
        R = B * NF
        pw = ops._empty((R, self.nbp), wave.device)
        energy = ops._empty((R,), wave.device)
        geom = (self.frame_len, self.frame_step, self.nfft)
        if self.dft == "fft64":
            if lens is None:
                call("dlip_powspec_wave_fft64_f32", wave, pw, energy, B, S, NF, *geom, float(self.preemph), self.nb, self.nbp)
            else:
                call("dlip_powspec_wave_fft64_ragged_f32", wave, lens, pw, energy, B, S, NF, *geom, float(self.preemph), self.nb, self.nbp)
        else:
            frames = ops._empty((R, self.nfft), wave.device)
            if lens is None:
                call("dlip_frame_preemph_f32", wave, frames, B, S, NF, *geom, self.preemph)
            else:
                call("dlip_frame_preemph_ragged_f32", wave, lens, frames, B, S, NF, *geom, self.preemph)
            if self.dft == "direct64":
                call("dlip_powspec_dft64_f32", frames, pw, energy, R, self.nb, self.nbp, self.nfft)
            else:
                spec = ops.linear(frames, self.w_dft)                          # [R, 2*nb]  (DFT as GEMM)
                call("dlip_powspec_f32", spec, pw, energy, R, self.nb, self.nbp, self.nfft)
        if lens is None:
            mel = torch.zeros((R, self.nfp), device=wave.device, dtype=torch.float32)
        else:                   # (a buffer of the plan's arena when a step is being recorded: nothing is allocated under capture)
            mel = ops._empty((R, self.nfp), wave.device).zero_()
        ops.conv_nhwc(pw.view(1, 1, R, self.nbp), self.w_mel.view(self.num_bin, 1, 1, self.nbp),
                      out=mel.view(1, 1, R, self.nfp))                         # [R, num_bin] (+ zero pad)
        feat, C_, en = mel, self.num_bin, None
        if self.feat_type in ("mfcc", "logfbank"):
            lg = ops._empty(tuple(mel.shape), mel.device)
            call("dlip_log_floor_f32", mel, lg, mel.numel())
            feat = lg
        if self.feat_type == "mfcc":
            feat = ops.linear(feat, self.w_dct)                                # [R, num_cep]
            C_ = self.num_cep
            en = energy if self.energy else None                               # appendEnergy: c0 = log(energy)
        out = ops._empty((B, C_, NF), wave.device)
        nf = None
        if lens is None:
            call("dlip_cmvn_nct_f32", feat, en, out, B, NF, C_, feat.shape[1], int(self.normalize))
        else:
            nf = ops._empty((B,), wave.device, torch.int32)
            call("dlip_wave_frame_lengths_i32", lens, nf, B, S, self.frame_len, self.frame_step)
            call("dlip_cmvn_nct_ragged_f32", feat, en, nf, out, B, NF, C_, feat.shape[1], int(self.normalize))
        return self._deltas(out, nf, B, C_, NF, lens is None)


class VideoFrontend:
    """uint8 frames -> normalised grayscale clips [B,1,T,88,88] ready for Lipreading."""

    def __init__(self, crop: int = 88):
        self.crop = crop

    def __call__(self, frames: torch.Tensor, clip_params: Optional[torch.Tensor] = None,
                 lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames [B,T,H,W] (gray) or [B,T,3,H,W] (RGB) uint8 cuda.  Default: the "val" pipeline (CenterCrop).  ``clip_params``
        (int32 cuda [B,4] = (oy, ox, flip, 0), see ops.draw_clip_params): the "train" pipeline's RandomCrop + HorizontalFlip per
        clip (preprocess.py:95-138).  ``lengths`` (int32 cuda [B]): frames t >= lengths[b] become zeros of the NORMALISED clip,
        the padding of pad_packed_collate."""
        if frames.dtype != torch.uint8 or not frames.is_cuda:
            raise TypeError("VideoFrontend expects uint8 CUDA frames")
        frames = frames.contiguous()
        ch = 3 if frames.dim() == 5 else 1
        B, T = frames.shape[0], frames.shape[1]
        H, W = frames.shape[-2], frames.shape[-1]
        for t, n, shape in ((clip_params, "clip_params", (B, 4)), (lengths, "lengths", (B,))):
            if t is not None and (t.dtype != torch.int32 or not t.is_cuda or tuple(t.shape) != shape or not t.is_contiguous()):
                raise ValueError(f"VideoFrontend: {n} must be a contiguous int32 CUDA tensor of shape {shape}")
        y = ops._empty((B, 1, T, self.crop, self.crop), frames.device)   # (arena-aware: this may run inside a recorded step plan)
        call("dlip_crop_normalize_u8", frames, clip_params, lengths, T, y, B * T, ch, H, W, self.crop)
        return y

    def collate(self, clips: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, List[int]]:
        """pad_packed_collate (dataset.py:123-139): clips [T_i,H,W] (or [T_i,3,H,W]) uint8 cuda, sorted by length (desc),
        normalised, and zero-padded to the longest AFTER the normalisation, as the reference does (its dataset normalises in
        __getitem__, dataset.py:117, and the collate pads the normalised clips with zeros, :130-134).  Round 4 padded the raw
        bytes and normalised the padding along: (0 / 255 - 0.421) / 0.165 = -2.55 in every padding pixel instead of 0."""
        order = sorted(range(len(clips)), key=lambda i: clips[i].shape[0], reverse=True)
        lengths = [int(clips[i].shape[0]) for i in order]
        shape = (len(clips), lengths[0]) + tuple(clips[0].shape[1:])
        buf = torch.zeros(shape, dtype=torch.uint8, device=clips[0].device)
        for j, i in enumerate(order):
            buf[j, :lengths[j]] = clips[i]
        return self(buf, lengths=torch.tensor(lengths, dtype=torch.int32).to(buf.device)), lengths
