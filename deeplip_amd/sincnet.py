"""The SincNet front layer of ``arch: sincnet`` (Ravanelli & Bengio 2018): a bank of learnable band-pass filters on
the raw waveform in front of the TDNN stack -- the one front-end of this project that is trained.

``SincConv`` holds the two parameters of the widely used layer under its own names and shapes (``low_hz_``, ``band_hz_``: fp32 [F, 1],
so its checkpoints load) and turns waveforms [B, S] (+ ``lengths``) into frame-level log band energies: [B, F, NF] like
``AudioFrontend`` for the extraction chain, or channels-last [B, NF, Fp] for the training step.  Nothing upstream defines the layer:
include/deeplip_hip.h with DESIGN.md 4l is the definition, tests/sinc_ref.py restates it in fp64.  Two kernel pairs under one autograd
``Function`` each: parameters <-> taps (``dlip_sinc_taps_*``) and waveform + taps <-> features (``dlip_sinc_features_*``); the stride-1
filter output is never stored, forward or backward.  Exact fp32 whatever the arithmetic mode of the encoder behind it.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch
import torch.nn as nn
from torch.autograd import Function

from . import _lib, ops
from ._lib import call, lib
from .frontend import num_frames, round_half_up

SINC_KEYS = ("kernel_size", "min_low_hz", "min_band_hz", "eps")
GEOMETRY_KEYS = ("rate", "win_len", "win_shift")        # filled in from the data section by trainer_common.build_speech_encoder
MAX_TAPS = _lib.HEADER["DLIP_SINC_MAX_TAPS"]
MAX_FILTERS = _lib.HEADER["DLIP_SINC_MAX_FILTERS"]
LDS_SAMPLES = _lib.HEADER["DLIP_SINC_LDS_SAMPLES"]


def parse_sinc_section(section) -> dict:
    """The keyword arguments of ``SincConv`` a ``model.sincnet.sinc`` section names (host only).  Defaults: ``kernel_size`` 251,
    ``min_low_hz`` 50, ``min_band_hz`` 50, ``eps`` 1e-6, ``rate`` 16000, ``win_len`` 0.025, ``win_shift`` 0.01.  Unknown keys, an even
    ``kernel_size`` or one outside [3, 1023], negative edges and a non-positive ``eps`` or ``rate`` raise ValueError."""
    section = {} if section is None else section
    if not isinstance(section, dict):
        raise ValueError(f"model.sincnet.sinc: expected a mapping of {list(SINC_KEYS)}, got {type(section).__name__}")
    unknown = sorted(set(section) - set(SINC_KEYS) - set(GEOMETRY_KEYS))
    if unknown:
        raise ValueError(f"model.sincnet.sinc: unknown key(s) {unknown}; expected {list(SINC_KEYS)}")
    L = section.get("kernel_size", 251)
    if isinstance(L, bool) or not isinstance(L, int) or L % 2 == 0 or not 3 <= L <= MAX_TAPS:
        raise ValueError(f"model.sincnet.sinc.kernel_size: an odd integer in [3, {MAX_TAPS}], got {L!r}")
    out = {"kernel_size": L}
    for key, default, positive in (("min_low_hz", 50.0, False), ("min_band_hz", 50.0, False), ("eps", 1e-6, True), ("rate", 16000, True),
                                   ("win_len", 0.025, True), ("win_shift", 0.01, True)):
        v = section.get(key, default)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0 or (positive and v <= 0):
            raise ValueError(f"model.sincnet.sinc.{key}: expected a {'positive' if positive else 'non-negative'} number, got {v!r}")
        out[key] = int(v) if key == "rate" else float(v)
    return out


def mel_edges(n_filters: int, rate: int, min_low_hz: float, min_band_hz: float):
    """The initial (low_hz_, band_hz_) of the layer, float64 [F]: mel-spaced edges between 30 Hz and rate / 2 - (min_low_hz + min_band_hz)."""
    to_mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
    to_hz = lambda mel: 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    hz = to_hz(np.linspace(to_mel(30.0), to_mel(rate / 2.0 - (min_low_hz + min_band_hz)), n_filters + 1))
    return hz[:-1].copy(), np.diff(hz)


class SincTapsFn(Function):
    """(low_hz_, band_hz_) [F, 1] -> g [F, L]: one launch each way, so a recorded step holds them."""

    @staticmethod
    def forward(ctx, low, band, L, rate, min_low, min_band):
        ops._req(low, "SincConv: low_hz_")
        ops._req(band, "SincConv: band_hz_")
        F_ = low.numel()
        g = ops._empty((F_, L), low.device)
        call("dlip_sinc_taps_f32", low, band, g, F_, L, float(rate), float(min_low), float(min_band))
        ctx.save_for_backward(low, band)
        ctx.cfg = (L, float(rate), float(min_low), float(min_band))
        return g

    @staticmethod
    def backward(ctx, dg):
        low, band = ctx.saved_tensors
        L, rate, min_low, min_band = ctx.cfg
        dlow, dband = torch.empty_like(low), torch.empty_like(band)
        call("dlip_sinc_taps_bwd_f32", low, band, dg.contiguous(), dlow, dband, low.numel(), L, rate, min_low, min_band)
        return dlow, dband, None, None, None, None


class SincFeaturesFn(Function):
    """(g [F, L], wave [B, S], lengths) -> (y, frame_lengths); y [B, F, NF] (``Fp`` = 0) or channels-last [B, NF, Fp].  The waveform is
    data: the backward returns the gradient of the taps alone (dg, symmetrised: include/deeplip_hip.h), z recomputed."""

    @staticmethod
    def forward(ctx, g, wave, lens, frame_len, frame_step, Fp, eps):
        B, S = wave.shape
        F_, L = g.shape
        NF = num_frames(S, frame_len, frame_step)
        layout = 1 if Fp else 0
        y = ops._empty((B, NF, Fp) if layout else (B, F_, NF), wave.device)
        nf = ops._empty((B,), wave.device, torch.int32)
        call("dlip_sinc_features_f32", wave, lens, g, y, nf, B, S, F_, L, frame_len, frame_step, NF, layout, Fp if layout else F_, float(eps))
        ctx.save_for_backward(g, wave, lens, y)
        ctx.cfg = (frame_len, frame_step, NF, layout, Fp if layout else F_)
        ctx.mark_non_differentiable(nf)
        return y, nf

    @staticmethod
    def backward(ctx, dy, _dnf=None):
        g, wave, lens, y = ctx.saved_tensors
        frame_len, frame_step, NF, layout, Fp = ctx.cfg
        B, S = wave.shape
        F_, L = g.shape
        nbytes = int(lib().dlip_sinc_features_bwd_workspace_bytes(B, S, F_, L, frame_len, frame_step))
        if nbytes <= 0:
            raise _lib.DeepLipHipError(f"dlip_sinc_features_bwd_workspace_bytes refused B = {B}, S = {S}, F = {F_}, L = {L}")
        ws = torch.empty((nbytes // 4,), device=wave.device, dtype=torch.float32)
        dg = torch.empty_like(g)
        call("dlip_sinc_features_bwd_f32", wave, lens, g, y, dy.contiguous(), dg, ws, nbytes, B, S, F_, L, frame_len, frame_step, NF, layout, Fp)
        return dg, None, None, None, None, None, None


class SincConv(nn.Module):
    """``n_filters`` band-pass filters of ``kernel_size`` taps on the waveform, then the log of each band's mean energy per frame of
    ``win_len`` seconds every ``win_shift`` (rounded as ``AudioFrontend`` rounds them).  Stands where a front-end stands:
    ``self(wave, lengths) -> (features [B, F, NF], frame_lengths)``, ``frame_len`` / ``frame_step`` / ``frames_for_samples``.  There is no
    mean or variance normalisation in the layer: the TDNN's BatchNorm follows."""
    feat_type = "sinc"

    def __init__(self, n_filters: int, kernel_size: int = 251, min_low_hz: float = 50.0, min_band_hz: float = 50.0, eps: float = 1e-6,
                 rate: int = 16000, win_len: float = 0.025, win_shift: float = 0.01):
        super().__init__()
        o = parse_sinc_section(dict(kernel_size=kernel_size, min_low_hz=min_low_hz, min_band_hz=min_band_hz, eps=eps, rate=rate,
                                    win_len=win_len, win_shift=win_shift))
        if isinstance(n_filters, bool) or not isinstance(n_filters, int) or not 1 <= n_filters <= MAX_FILTERS:
            raise ValueError(f"SincConv: 1 .. {MAX_FILTERS} filters, got {n_filters!r}")
        self.n_filters, self.kernel_size, self.rate = n_filters, o["kernel_size"], o["rate"]
        self.min_low_hz, self.min_band_hz, self.eps = o["min_low_hz"], o["min_band_hz"], o["eps"]
        if self.min_low_hz + self.min_band_hz + 30.0 >= self.rate / 2.0:
            raise ValueError(f"SincConv: min_low_hz + min_band_hz = {self.min_low_hz + self.min_band_hz} leaves no band below rate / 2 = "
                             f"{self.rate / 2.0}")
        self.frame_len = round_half_up(o["win_len"] * self.rate)
        self.frame_step = round_half_up(o["win_shift"] * self.rate)
        if self.frame_len < 1 or self.frame_step < 1:
            raise ValueError(f"SincConv: win_len * rate and win_shift * rate must round to at least one sample, got {self.frame_len} and "
                             f"{self.frame_step}")
        if self.frame_len + self.kernel_size - 1 > LDS_SAMPLES:
            raise ValueError(f"SincConv: frame_len + kernel_size - 1 = {self.frame_len + self.kernel_size - 1} samples exceed the "
                             f"{LDS_SAMPLES} a workgroup's tile holds")
        low, band = mel_edges(n_filters, self.rate, self.min_low_hz, self.min_band_hz)
        self.low_hz_ = nn.Parameter(torch.from_numpy(low).float().view(-1, 1))
        self.band_hz_ = nn.Parameter(torch.from_numpy(band).float().view(-1, 1))

    feat_dim = property(lambda self: self.n_filters)
    min_samples = 1

    def frames_for_samples(self, n: int) -> int:
        return num_frames(int(n), self.frame_len, self.frame_step)

    def samples_for_frames(self, T: int) -> int:
        """The longest signal that has T frames: a batch padded to it comes out with T frames."""
        return self.frame_len + (int(T) - 1) * self.frame_step

    def taps(self) -> torch.Tensor:
        """g [F, L] (differentiable with respect to the two parameters)."""
        return SincTapsFn.apply(self.low_hz_, self.band_hz_, self.kernel_size, self.rate, self.min_low_hz, self.min_band_hz)

    def features(self, wave: torch.Tensor, lengths=None, channels_last_pad: Optional[int] = None):
        """wave [B, S] float32 (cuda) -> (y, frame_lengths int32 device [B]).  ``channels_last_pad``: None -> y [B, F, NF]; Fp >= F -> y
        [B, NF, Fp] channels-last, channels >= F zero (what the first TDNN block of the training step reads).  ``lengths``: sample counts in
        [1, S] -- host values are validated, an int32 device tensor is clamped by the kernel and never read on the host; row b's frames
        [0, frame_lengths[b]) equal the row run alone whatever the padding holds, frames past them are zeros.  Launches only."""
        if wave.dim() != 2:
            raise ValueError(f"SincConv takes waveforms [B, S], got {tuple(wave.shape)}")
        ops._req(wave, "SincConv: wave")
        B, S = wave.shape
        lens = ops.lengths_i32(lengths, wave.device, n=B, lo=1, hi=S)
        Fp = 0 if channels_last_pad is None else int(channels_last_pad)
        if Fp and not self.n_filters <= Fp <= self.n_filters + 31:
            raise ValueError(f"SincConv: channels_last_pad {Fp} must lie in [{self.n_filters}, {self.n_filters + 31}]")
        return SincFeaturesFn.apply(self.taps(), wave, lens, self.frame_len, self.frame_step, Fp, self.eps)

    def forward(self, wave: torch.Tensor, lengths=None):
        """As ``AudioFrontend.__call__``: features [B, F, NF] for a rectangular batch, ``(features, frame_lengths)`` with ``lengths``."""
        y, nf = self.features(wave.contiguous().float(), lengths)
        return y if lengths is None else (y, nf)
