"""Kaldi-style sliding-window CMN and energy-VAD frame selection behind the audio front-end (ABI 62).

The reference's speech pipeline feeds its encoder and its PLDA back-end through

    apply-cmvn-sliding --norm-vars=false --center=true --cmn-window=300 ... | select-voiced-frames ... vad.scp

(conf/audio_config.yaml:21 ``plda_input``, :25 ``nn_input``): a 300-frame sliding mean normalisation, then the frames an energy VAD
marks unvoiced are dropped.  No source for these tools ships upstream and Kaldi is not a dependency: parity is UNPINNED, and
include/deeplip_hip.h with DESIGN.md 4f is the definition, restated from Kaldi's published ``SlidingWindowCmn`` and
``ComputeVadEnergy``.  ``VoicedFrames`` runs both on a ragged batch ``x [B, C, NF]`` (+ ``lengths``) with the ``dlip_vad_energy_select_i32``
and ``dlip_cmn_sliding_select_f32`` kernels and hands the encoders a NEW length vector -- the kept frames per row -- that lives on the
device like every other one (``extract_embedding(lengths=)``): a data-dependent length the host never reads.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib, ops
from ._lib import call, ptr

SECTION_KEYS = ("cmn_window", "center", "min_window", "norm_vars", "vad", "energy_row", "min_keep")
VAD_KEYS = ("energy_threshold", "energy_mean_scale", "frames_context", "proportion_threshold")
# the VoxCeleb recipe's conf/vad.conf (Kaldi's own defaults are 5.0, 0.5, 0, 0.6)
VAD_DEFAULTS = {"energy_threshold": 5.5, "energy_mean_scale": 0.5, "frames_context": 2, "proportion_threshold": 0.12}


def window_bounds(t: int, n: int, window: int, center: bool = True, min_window: int = 100) -> Tuple[int, int]:
    """The window ``[begin, end)`` of frame ``t`` of an ``n``-frame utterance, as Kaldi's SlidingWindowCmn cuts it (host restatement
    of the kernel's rule, for tests and documentation): centred on t or ending behind it, shifted -- not shrunk -- at either end of
    the utterance, the whole utterance where it is shorter than the window."""
    if center:
        begin = t - window // 2
        end = begin + window
    else:
        begin, end = t - window, t + 1
    if begin < 0:
        end -= begin
        begin = 0
    if not center and end > t:
        end = max(t + 1, min_window)
    if end > n:
        begin -= end - n
        end = n
        if begin < 0:
            begin = 0
    return begin, end


def _parse_vad(v) -> Optional[dict]:
    if v is None or v is False:
        return None
    if v is True:
        v = {}
    if not isinstance(v, dict):
        raise ValueError(f"voiced_frames.vad: expected a mapping of {list(VAD_KEYS)} or null, got {type(v).__name__}")
    unknown = sorted(set(v) - set(VAD_KEYS))
    if unknown:
        raise ValueError(f"voiced_frames.vad: unknown key(s) {unknown}; expected {list(VAD_KEYS)}")
    out = dict(VAD_DEFAULTS, **v)
    out["energy_threshold"], out["energy_mean_scale"] = float(out["energy_threshold"]), float(out["energy_mean_scale"])
    if out["energy_threshold"] != out["energy_threshold"] or out["energy_mean_scale"] != out["energy_mean_scale"]:
        raise ValueError("voiced_frames.vad: energy_threshold and energy_mean_scale must be numbers")
    if isinstance(out["frames_context"], bool) or int(out["frames_context"]) != out["frames_context"] or int(out["frames_context"]) < 0:
        raise ValueError(f"voiced_frames.vad.frames_context: {out['frames_context']!r} is not a non-negative frame count")
    out["frames_context"] = int(out["frames_context"])
    p = float(out["proportion_threshold"])
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"voiced_frames.vad.proportion_threshold: {p} is not a proportion")
    out["proportion_threshold"] = p
    return out


def parse_voiced_frames_section(section) -> Optional[dict]:
    """A ``voiced_frames:`` config section (``data.voiced_frames`` of conf/audio_config.yaml, ``data.python_data_config.voiced_frames``
    of the fusion config) as the keyword arguments of ``VoicedFrames``, or None for an absent one.  Absent keys take Kaldi's values
    of the reference's pipe (window 300, centred, means only) and the VoxCeleb recipe's VAD; ``cmn_window: null`` means selection
    only, ``vad: null`` CMN only; ``min_keep`` stays None where the section does not name it (the caller's encoder decides).
    Unknown keys, a window outside [1, DLIP_CMN_MAX_WINDOW], a proportion outside [0, 1], a negative context and both halves
    switched off raise ValueError."""
    if section is None or section is False:
        return None
    if section is True:
        section = {}
    if not isinstance(section, dict):
        raise ValueError(f"voiced_frames: expected a mapping of {list(SECTION_KEYS)}, got {type(section).__name__}")
    unknown = sorted(set(section) - set(SECTION_KEYS))
    if unknown:
        raise ValueError(f"voiced_frames: unknown key(s) {unknown}; expected {list(SECTION_KEYS)}")
    cap = _lib.DLIP_CMN_MAX_WINDOW
    out = {}
    window = section.get("cmn_window", 300)
    if window is not None:
        if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= cap:
            raise ValueError(f"voiced_frames.cmn_window: {window!r} is outside [1, {cap}] (the kernel's cap; null switches the CMN off)")
        window = int(window)
    out["cmn_window"] = window
    out["center"] = bool(section.get("center", True))
    min_window = section.get("min_window", 100)
    if isinstance(min_window, bool) or int(min_window) != min_window or not 1 <= int(min_window) <= cap:
        raise ValueError(f"voiced_frames.min_window: {min_window!r} is outside [1, {cap}]")
    out["min_window"] = int(min_window)
    out["norm_vars"] = bool(section.get("norm_vars", False))
    out["vad"] = _parse_vad(section.get("vad", {}))
    if out["cmn_window"] is None and out["vad"] is None:
        raise ValueError("voiced_frames: cmn_window and vad are both null -- nothing to apply (leave the section out instead)")
    row = section.get("energy_row", 0)
    if isinstance(row, bool) or int(row) != row or int(row) < 0:
        raise ValueError(f"voiced_frames.energy_row: {row!r} is not a feature row")
    out["energy_row"] = int(row)
    keep = section.get("min_keep")
    if keep is not None:
        if isinstance(keep, bool) or int(keep) != keep or int(keep) < 1:
            raise ValueError(f"voiced_frames.min_keep: {keep!r} must be a frame count >= 1")
        keep = int(keep)
    out["min_keep"] = keep
    return out


class VoicedFrames:
    """``cmn_window``: frames of the sliding mean (None: no CMN), ``center`` / ``min_window`` / ``norm_vars`` as apply-cmvn-sliding's
    options.  ``vad``: the four options of compute-vad-energy (None: no selection unless a call brings its own mask).
    ``energy_row``: the row of x that holds the log-energy (MFCC c0 with ``energy: true``).  ``min_keep``: a row with fewer voiced
    frames keeps all of its frames (pass the encoder's minimum frame count)."""

    def __init__(self, cmn_window: Optional[int] = 300, center: bool = True, min_window: int = 100, norm_vars: bool = False,
                 vad: Optional[dict] = VAD_DEFAULTS, energy_row: int = 0, min_keep: Optional[int] = 1):
        o = parse_voiced_frames_section({"cmn_window": cmn_window, "center": center, "min_window": min_window, "norm_vars": norm_vars,
                                         "vad": vad, "energy_row": energy_row, "min_keep": min_keep})
        self.cmn_window, self.center, self.min_window, self.norm_vars = o["cmn_window"], o["center"], o["min_window"], o["norm_vars"]
        self.vad, self.energy_row = o["vad"], o["energy_row"]
        self.min_keep = 1 if o["min_keep"] is None else o["min_keep"]
        self.last_fallback = None      # int32 device [B] of the last call that selected: 1 where a row kept all its frames

    def __call__(self, x: torch.Tensor, lengths=None, log_energy: Optional[torch.Tensor] = None,
                 voiced: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """x [B, C, NF] float32 (cuda) -> ``(y [B, C, NF], out_len int32 device [B])``: row b's first out_len[b] columns hold its kept
        frames in order, the rest exact zeros.  ``lengths``: as ``AudioFrontend``'s (host values are validated; an int32 device
        tensor is clamped by the kernels and never read on the host).  ``log_energy`` [B, NF] float32: the VAD's input instead of
        row ``energy_row`` of x.  ``voiced`` [B, NF] uint8 / bool: an external decision (``vad.scp``) instead of the energy VAD.
        Launches only: no synchronisation, no host read, buffers from ``ops._empty`` -- the call records into a step plan and
        replays with new data and lengths."""
        ops._req(x, "VoicedFrames: x")
        if x.dim() != 3:
            raise ValueError(f"VoicedFrames: expected x [B, C, NF], got {tuple(x.shape)}")
        B, C, NF = x.shape
        dev = x.device
        lens = ops.lengths_i32(lengths, dev, n=B, lo=1, hi=NF)
        select = voiced is not None or self.vad is not None
        if not select and log_energy is not None:
            raise ValueError("VoicedFrames: log_energy given but the VAD is switched off")
        window = 0 if self.cmn_window is None else self.cmn_window
        if not select and window == 0:
            raise ValueError("VoicedFrames: nothing to apply (no CMN window, no VAD, no mask)")
        pos = out_len = None
        if select:
            e_ptr = stride = None
            if voiced is not None:
                if voiced.dtype == torch.bool:
                    voiced = voiced.view(torch.uint8)
                ops._req(voiced, "VoicedFrames: voiced", torch.uint8)
                if tuple(voiced.shape) != (B, NF):
                    raise ValueError(f"VoicedFrames: voiced must be [B, NF] = {(B, NF)}, got {tuple(voiced.shape)}")
                e_ptr, stride = None, NF
            elif log_energy is not None:
                ops._req(log_energy, "VoicedFrames: log_energy")
                if tuple(log_energy.shape) != (B, NF):
                    raise ValueError(f"VoicedFrames: log_energy must be [B, NF] = {(B, NF)}, got {tuple(log_energy.shape)}")
                e_ptr, stride = ptr(log_energy), NF
            else:
                if not self.energy_row < C:
                    raise ValueError(f"VoicedFrames: energy_row {self.energy_row} but x has {C} rows")
                e_ptr, stride = ptr(x) + 4 * self.energy_row * NF, C * NF          # row energy_row of every utterance, no copy
            v = self.vad or VAD_DEFAULTS                                            # (an external mask reads none of them)
            pos = ops._empty((B, NF), dev, torch.int32)
            out_len = ops._empty((B,), dev, torch.int32)
            self.last_fallback = ops._empty((B,), dev, torch.int32)
            call("dlip_vad_energy_select_i32", e_ptr, stride, voiced, lens, v["energy_threshold"], v["energy_mean_scale"], v["frames_context"],
                 v["proportion_threshold"], self.min_keep, pos, out_len, self.last_fallback, B, NF)
        else:
            # CMN only: every frame stays, the length vector is the input's (clamped like the kernels clamp it)
            out_len = ops._empty((B,), dev, torch.int32)
            if lens is None:
                out_len.fill_(NF)
            else:
                torch.clamp(lens, 1, NF, out=out_len)
            self.last_fallback = None
        y = ops._empty((B, C, NF), dev)
        call("dlip_cmn_sliding_select_f32", x, lens, pos, out_len if select else None, y, B, C, NF, window, int(self.center), self.min_window,
             int(self.norm_vars))
        return y, out_len
