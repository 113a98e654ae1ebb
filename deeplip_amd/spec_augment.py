"""SpecAugment on the device, on the feature batch in front of the encoder (ABI 67, added).

The one augmentation of a speaker-embedding recipe that acts on the features rather than the waveform (Park et al. 2019): a time
warp, then frequency masks, then time masks.  Nothing upstream defines the stage -- include/deeplip_hip.h with DESIGN.md 4j is the
definition.  ``SpecAugment`` draws LENGTH-FREE 31-bit integers on the host (``draw``: the host never sees a row's length behind
``VoicedFrames`` or in a recorded plan) and the ``dlip_spec_augment_f32`` kernel resolves them against each row's own length
(``pick(r, m) = (r m) >> 31``) on a batch ``x [B, C, NF]`` (+ ``lengths``), each row as if it were alone.  tests/spec_augment_ref.py
is the definition in numpy.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, lib

SPEC_AUGMENT_KEYS = ("time_warp", "freq_masks", "freq_width", "time_masks", "time_width", "time_ratio", "fill")
FILLS = ("zero", "mean")            # exact zeros (the row's mean after CMVN) | the mean of the row's own input
MAX_MASKS = _lib.HEADER["DLIP_SPECAUG_MAX_MASKS"]
DRAWS = _lib.HEADER["DLIP_SPECAUG_DRAWS"]     # words per row: warp centre, warp shift, (width, start) per frequency mask, per time mask


def _count(section, key, default, hi=None):
    v = section.get(key, default)
    if isinstance(v, bool) or not isinstance(v, int) or v < 0 or (hi is not None and v > hi):
        raise ValueError(f"spec_augment.{key}: expected an integer " + (f"in [0, {hi}]" if hi is not None else ">= 0") + f", got {v!r}")
    return int(v)


def parse_spec_augment_section(section) -> Optional[dict]:
    """The keyword arguments of ``SpecAugment`` a ``spec_augment:`` config section names (``data.spec_augment`` of
    conf/audio_config.yaml), or None for an absent one.  Defaults: no warp, 2 frequency and 2 time masks, ``time_ratio: 1.0``,
    ``fill: zero``; ``freq_width`` / ``time_width`` are required when their count is above 0.  Unknown keys, counts outside
    [0, DLIP_SPECAUG_MAX_MASKS], negative widths, a ratio outside [0, 1], a ``fill`` other than ``zero`` / ``mean`` and a section that
    would do nothing raise ValueError."""
    if section is None or section is False:
        return None
    if not isinstance(section, dict):
        raise ValueError(f"spec_augment: expected a mapping of {list(SPEC_AUGMENT_KEYS)}, got {type(section).__name__}")
    unknown = sorted(set(section) - set(SPEC_AUGMENT_KEYS))
    if unknown:
        raise ValueError(f"spec_augment: unknown key(s) {unknown}; expected {list(SPEC_AUGMENT_KEYS)}")
    out = {"time_warp": _count(section, "time_warp", 0)}
    for count, width in (("freq_masks", "freq_width"), ("time_masks", "time_width")):
        out[count] = _count(section, count, 2, MAX_MASKS)
        if out[count] > 0 and width not in section:
            raise ValueError(f"spec_augment.{width}: the section needs it ({count} = {out[count]})")
        out[width] = _count(section, width, 0)
    r = section.get("time_ratio", 1.0)
    if isinstance(r, bool) or not isinstance(r, (int, float)) or not 0.0 <= float(r) <= 1.0:
        raise ValueError(f"spec_augment.time_ratio: {r!r} is not a ratio in [0, 1]")
    out["time_ratio"] = float(r)
    out["fill"] = section.get("fill", "zero")
    if out["fill"] not in FILLS:
        raise ValueError(f"spec_augment.fill: expected one of {list(FILLS)}, got {out['fill']!r}")
    _check_effect(out, "spec_augment")
    return {k: out[k] for k in SPEC_AUGMENT_KEYS}


def _check_effect(o, who):
    freq = o["freq_masks"] > 0 and o["freq_width"] > 0
    time = o["time_masks"] > 0 and o["time_width"] > 0 and o["time_ratio"] > 0.0
    if o["time_warp"] < 1 and not freq and not time:
        raise ValueError(f"{who}: nothing to apply (no warp, no frequency mask and no time mask of a width above 0); leave the "
                         "stage out instead")


class SpecAugment:
    """``time_warp``: W, the most frames the warp moves its centre by (0: no warp).  ``freq_masks`` x ``freq_width``: the number of
    frequency masks and the widest one, in features; ``time_masks`` x ``time_width``: the same along time, a mask no wider than
    ``time_ratio`` of the row (1.0: no adaptive cap beyond the row itself).  ``fill``: what a masked entry holds -- ``"zero"`` or
    ``"mean"``, the mean of the row's own input."""

    def __init__(self, time_warp: int = 0, freq_masks: int = 2, freq_width: int = 0, time_masks: int = 2, time_width: int = 0,
                 time_ratio: float = 1.0, fill: str = "zero", device="cuda"):
        o = dict(time_warp=time_warp, freq_masks=freq_masks, freq_width=freq_width, time_masks=time_masks, time_width=time_width)
        for k, v in o.items():
            hi = MAX_MASKS if k.endswith("_masks") else 2 ** 31 - 1
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) <= hi:
                raise ValueError(f"SpecAugment: {k} must be an integer in [0, {hi}], got {v!r}")
            o[k] = int(v)
        if not 0.0 <= float(time_ratio) <= 1.0:
            raise ValueError(f"SpecAugment: time_ratio {time_ratio!r} is not a ratio in [0, 1]")
        if fill not in FILLS:
            raise ValueError(f"SpecAugment: fill must be one of {list(FILLS)}, got {fill!r}")
        o.update(time_ratio=float(time_ratio), fill=fill)
        _check_effect(o, "SpecAugment")
        self.__dict__.update(o)
        self.device = torch.device(device)

    def draw(self, B: int, rng: np.random.Generator) -> Dict[str, np.ndarray]:
        """The random choices of one batch, host only and free of any length: ``draws`` int32 [B, DLIP_SPECAUG_DRAWS], every word
        uniform over [0, 2^31)."""
        return {"draws": rng.integers(0, 2 ** 31, size=(int(B), DRAWS), dtype=np.int64).astype(np.int32)}

    def __call__(self, x: torch.Tensor, lengths=None, params=None, rng: Optional[np.random.Generator] = None) -> torch.Tensor:
        """x [B, C, NF] or [B, 1, F, T] float32 (cuda) -> the augmented batch of the same shape (a new tensor; frames past a row's
        length are zeros).  ``lengths``: as ``AudioFrontend``'s, in frames (host values are validated, an int32 device tensor is
        clamped by the kernel and never read on the host).  ``params``: what ``draw`` returned -- a numpy array (copied in without
        synchronising) or an int32 device tensor (a recorded step plan's input); None draws them here from ``rng``.  Launches only:
        nothing below synchronises or allocates outside ``ops._empty``, so the call records into a step plan."""
        ops._req(x, "SpecAugment: x")
        if x.dim() == 4 and x.shape[1] == 1:
            B, _, C, NF = x.shape
        elif x.dim() == 3:
            B, C, NF = x.shape
        else:
            raise ValueError(f"SpecAugment: expected x [B, C, NF] or [B, 1, F, T], got {tuple(x.shape)}")
        dev = x.device
        lens = ops.lengths_i32(lengths, dev, n=B, lo=1, hi=NF)
        if params is None:
            params = self.draw(B, rng if rng is not None else np.random.default_rng())
        if sorted(params) != ["draws"]:
            raise ValueError(f"SpecAugment: params must hold exactly 'draws' (pass params=draw(B, rng)), got {sorted(params)}")
        v = params["draws"]
        if not isinstance(v, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(v))
        if not v.is_cuda:
            v = v.to(dev, non_blocking=True)
        if v.dtype != torch.int32 or tuple(v.shape) != (B, DRAWS):
            raise TypeError(f"SpecAugment: params['draws'] must be torch.int32 [{B}, {DRAWS}], got {v.dtype} {tuple(v.shape)}")
        v = v.contiguous()
        nbytes = int(lib().dlip_spec_augment_workspace_bytes(B, C, NF))
        if nbytes <= 0:
            raise _lib.DeepLipHipError(f"dlip_spec_augment_workspace_bytes refused B = {B}, C = {C}, NF = {NF}")
        ws = ops._empty((nbytes // 8,), dev, torch.float64)
        y = ops._empty(tuple(x.shape), dev)
        call("dlip_spec_augment_f32", x, lens, v, y, ws, nbytes, B, C, NF, self.time_warp, self.freq_masks, self.freq_width, self.time_masks,
             self.time_width, self.time_ratio, FILLS.index(self.fill))
        return y
