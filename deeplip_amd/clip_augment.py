"""Lip-clip augmentation on the device, between the loader's frames and the stem (ABI 67, added).

Time masks filled with the clip's mean, cutout, and mixup of clip pairs -- the augmentations lip-reading models are trained with beyond
the reference's RandomCrop + HorizontalFlip.  Nothing upstream defines the stage: include/deeplip_hip.h with DESIGN.md 4m is the
definition, tests/clip_augment_ref.py restates it in numpy.  ``ClipAugment`` draws LENGTH-FREE 31-bit integers on the host (``draw``)
and the ``dlip_clip_augment_u8`` / ``dlip_clip_augment_f32`` kernels resolve them against each clip's own length
(``pick(r, m) = (r m) >> 31``), straight from the uint8 frames (crop + flip + gray + normalisation as ``dlip_crop_normalize_u8``) or from
normalised float clips.  Training only: evaluation, extraction, ``embed()`` and bench.py never apply it.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, lib

FILLS = ("zero", "mean")            # exact zeros | the mean of the clip's own valid pixels before masking
MAX_MASKS = _lib.HEADER["DLIP_CLIPAUG_MAX_MASKS"]
DRAWS = _lib.HEADER["DLIP_CLIPAUG_DRAWS"]     # words per clip: (width, start) per time mask, then (height, width, top, left) per cutout
MAX_CUT = 2 ** 30


class ClipAugment:
    """``time_masks`` x ``time_width``: the number of time masks and the widest one, in frames, a mask no wider than ``time_ratio`` of
    the clip.  ``cutouts`` x ``cut_size``: the number of rectangles and their largest side, in pixels of the output, the same rectangle
    in every frame of a clip.  ``fill``: what a masked pixel holds -- ``"zero"`` or ``"mean"``, the mean of the clip's own pixels.
    ``mixup_alpha`` > 0: every batch is blended with a permutation of itself, ``lam ~ Beta(alpha, alpha)`` per batch (``mix_targets``
    gives the criterion's side).  ``crop``: the side of the output for uint8 frames (a multiple of 4)."""

    def __init__(self, time_masks: int = 0, time_width: int = 0, time_ratio: float = 1.0, cutouts: int = 0, cut_size: int = 0,
                 fill: str = "mean", mixup_alpha: float = 0.0, crop: int = 88):
        o = dict(time_masks=time_masks, time_width=time_width, cutouts=cutouts, cut_size=cut_size, crop=crop)
        for k, v in o.items():
            hi = MAX_MASKS if k in ("time_masks", "cutouts") else (MAX_CUT if k == "cut_size" else 2 ** 31 - 1)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= hi:
                raise ValueError(f"ClipAugment: {k} must be an integer in [0, {hi}], got {v!r}")
            o[k] = int(v)
        if o["crop"] < 4 or o["crop"] % 4:
            raise ValueError(f"ClipAugment: crop must be a multiple of 4 (the kernel writes four pixels per lane), got {crop!r}")
        if isinstance(time_ratio, bool) or not isinstance(time_ratio, (int, float)) or not 0.0 <= float(time_ratio) <= 1.0:
            raise ValueError(f"ClipAugment: time_ratio {time_ratio!r} is not a ratio in [0, 1]")
        if fill not in FILLS:
            raise ValueError(f"ClipAugment: fill must be one of {list(FILLS)}, got {fill!r}")
        if isinstance(mixup_alpha, bool) or not isinstance(mixup_alpha, (int, float)) or not (0.0 <= float(mixup_alpha) < math.inf):
            raise ValueError(f"ClipAugment: mixup_alpha must be a finite number >= 0, got {mixup_alpha!r}")
        o.update(time_ratio=float(time_ratio), fill=fill, mixup_alpha=float(mixup_alpha))
        time = o["time_masks"] > 0 and o["time_width"] > 0 and o["time_ratio"] > 0.0
        cut = o["cutouts"] > 0 and o["cut_size"] > 0
        if not time and not cut and o["mixup_alpha"] == 0.0:
            raise ValueError("ClipAugment: nothing to apply (no time mask and no cutout of a size above 0, no mixup); leave the stage "
                             "out instead")
        self.__dict__.update(o)

    @property
    def mixup(self) -> bool:
        return self.mixup_alpha > 0.0

    def draw(self, B: int, rng: np.random.Generator) -> Dict[str, np.ndarray]:
        """The random choices of one batch, host only and free of any length: ``draws`` int32 [B, DLIP_CLIPAUG_DRAWS], every word
        uniform over [0, 2^31); with mixup also ``perm`` int32 [B], a permutation of the rows, and ``lam`` float32 [1] ~
        Beta(alpha, alpha)."""
        B = int(B)
        if B < 1:
            raise ValueError(f"ClipAugment.draw: B must be >= 1, got {B}")
        out = {"draws": rng.integers(0, 2 ** 31, size=(B, DRAWS), dtype=np.int64).astype(np.int32)}
        if self.mixup:
            out["perm"] = rng.permutation(B).astype(np.int32)
            out["lam"] = np.array([rng.beta(self.mixup_alpha, self.mixup_alpha)], dtype=np.float32)
        return out

    # ---- params: host values are validated here, device tensors are a recorded step plan's inputs (the kernel guards them)
    def _keys(self):
        return ["draws", "lam", "perm"] if self.mixup else ["draws"]

    def _check_params(self, params, B: int) -> None:
        if not isinstance(params, dict) or sorted(params) != self._keys():
            got = sorted(params) if isinstance(params, dict) else type(params).__name__
            raise ValueError(f"ClipAugment: params must hold exactly {self._keys()} (pass params=draw(B, rng)), got {got}")
        for k, dtype, shape in (("draws", "int32", (B, DRAWS)), ("perm", "int32", (B,)), ("lam", "float32", (1,))):
            if k not in params:
                continue
            v = params[k]
            if isinstance(v, torch.Tensor):
                if v.dtype != getattr(torch, dtype) or tuple(v.shape) != shape:
                    raise TypeError(f"ClipAugment: params[{k!r}] must be torch.{dtype} {list(shape)}, got {v.dtype} {list(v.shape)}")
                if v.is_cuda:
                    continue
                v = v.numpy()
            else:
                v = np.asarray(v)
                if v.dtype != np.dtype(dtype) or v.shape != shape:
                    raise TypeError(f"ClipAugment: params[{k!r}] must be {dtype} {list(shape)}, got {v.dtype} {list(v.shape)}")
            if k == "perm" and sorted(v.tolist()) != list(range(B)):
                raise ValueError(f"ClipAugment: params['perm'] is not a permutation of the {B} rows")
            if k == "lam" and not 0.0 <= float(v[0]) <= 1.0:
                raise ValueError(f"ClipAugment: params['lam'] = {float(v[0])!r} is not in [0, 1]")

    def to_device(self, params, device) -> Dict[str, torch.Tensor]:
        """``params`` (what ``draw`` returned) validated and on ``device``: copies that do not synchronise.  Device tensors pass."""
        self._check_params(params, len(params["draws"]) if isinstance(params, dict) and "draws" in params else 0)
        return self._move(params, device)

    @staticmethod
    def _move(params, device) -> Dict[str, torch.Tensor]:
        out = {}
        for k, v in params.items():
            if not isinstance(v, torch.Tensor):
                v = torch.from_numpy(np.ascontiguousarray(v))
            out[k] = (v if v.is_cuda else v.to(device, non_blocking=True)).contiguous()
        return out

    def __call__(self, src: torch.Tensor, clip_params: Optional[torch.Tensor] = None, lengths=None, params=None,
                 rng: Optional[np.random.Generator] = None) -> torch.Tensor:
        """``src``: uint8 frames [B,T,Hs,Ws] (gray) or [B,T,3,Hs,Ws] (RGB) with ``clip_params`` (int32 cuda [B,4] = (oy, ox, flip, 0),
        None: the centre crop) as ``VideoFrontend`` takes them, or a float32 clip [B,1,T,H,W] (no crop, no flip) -> the augmented
        clip [B,1,T,crop,crop] float32 (a new tensor; frames past a clip's length are zeros).  ``lengths``: host values are validated,
        an int32 device tensor is clamped by the kernel and never read on the host.  ``params``: what ``draw`` returned -- numpy
        arrays (validated, copied in without synchronising) or device tensors (a recorded step plan's inputs); None draws them here
        from ``rng``.  Launches only: nothing below synchronises or allocates outside ``ops._empty``."""
        if not isinstance(src, torch.Tensor):
            raise TypeError(f"ClipAugment: expected a tensor, got {type(src).__name__}")
        if src.dtype == torch.uint8 and src.dim() in (4, 5):
            ch = 1 if src.dim() == 4 else int(src.shape[2])
            B, T, Hs, Ws = int(src.shape[0]), int(src.shape[1]), int(src.shape[-2]), int(src.shape[-1])
            if ch not in (1, 3):
                raise ValueError(f"ClipAugment: frames must be [B,T,H,W] or [B,T,3,H,W], got {tuple(src.shape)}")
            if self.crop > Hs or self.crop > Ws:
                raise ValueError(f"ClipAugment: crop {self.crop} exceeds the {Hs} x {Ws} frames")
            OH = OW = self.crop
        elif src.dtype == torch.float32 and src.dim() == 5 and src.shape[1] == 1:
            ch = 0
            B, _, T, OH, OW = (int(s) for s in src.shape)
            if OW < 4 or OW % 4:
                raise ValueError(f"ClipAugment: the clip's width must be a multiple of 4, got {tuple(src.shape)}")
            if clip_params is not None:
                raise ValueError("ClipAugment: clip_params go with uint8 frames; a float clip is already cropped")
        else:
            raise TypeError("ClipAugment: expected uint8 frames [B,T,H,W] / [B,T,3,H,W] or a float32 clip [B,1,T,H,W], got "
                            f"{src.dtype} {tuple(src.shape)}")
        if B < 1 or T < 1 or B > 65535 or T > 65535:
            raise ValueError(f"ClipAugment: B and T must lie in [1, 65535], got {B}, {T}")
        if clip_params is not None and (not isinstance(clip_params, torch.Tensor) or tuple(clip_params.shape) != (B, 4)):
            raise ValueError("ClipAugment: clip_params must be an int32 tensor [B,4] = (oy, ox, flip, 0)")
        if params is None:
            params = self.draw(B, rng if rng is not None else np.random.default_rng())
        self._check_params(params, B)
        if lengths is not None and not (isinstance(lengths, torch.Tensor) and lengths.is_cuda):
            vals = [int(l) for l in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
            if len(vals) != B or min(vals) < 1 or max(vals) > T:
                raise ValueError(f"ClipAugment: lengths must be {B} values in [1, {T}], got {vals}")
        # ---- everything host-side is in order: from here on the device
        ops._req(src, "ClipAugment: src", src.dtype)
        ops._req(clip_params, "ClipAugment: clip_params", torch.int32)
        dev = src.device
        lens = ops.lengths_i32(lengths, dev, n=B, lo=1, hi=T)
        p = self._move(params, dev)
        nbytes = int(lib().dlip_clip_augment_workspace_bytes(B, T))
        if nbytes <= 0:
            raise _lib.DeepLipHipError(f"dlip_clip_augment_workspace_bytes refused B = {B}, T = {T}")
        ws = ops._empty((nbytes // 8,), dev, torch.float64)
        y = ops._empty((B, 1, T, OH, OW), dev)
        tail = (self.time_masks, self.time_width, self.time_ratio, self.cutouts, self.cut_size, FILLS.index(self.fill))
        if ch:
            call("dlip_clip_augment_u8", src, clip_params, lens, p["draws"], p.get("perm"), p.get("lam"), y, ws, nbytes, B, T, ch, Hs, Ws,
                 self.crop, *tail)
        else:
            call("dlip_clip_augment_f32", src, lens, p["draws"], p.get("perm"), p.get("lam"), y, ws, nbytes, B, T, OH, OW, *tail)
        return y

    def mix_targets(self, labels: torch.Tensor, params):
        """The criterion's side of mixup: ``(labels, labels[perm], lam)`` on the device -- the loss is ``lam CE(logits, labels) +
        (1 - lam) CE(logits, labels[perm])``.  ``params``: what the clips were mixed with (device tensors pass as they are)."""
        if not self.mixup:
            raise ValueError("ClipAugment.mix_targets: mixup is off (mixup_alpha = 0)")
        self._check_params(params, int(labels.shape[0]))
        ops._req(labels, "ClipAugment.mix_targets: labels", labels.dtype)
        p = self._move(params, labels.device)
        return labels, labels[p["perm"].long()], p["lam"]
