"""Waveform augmentation on the device, in front of ``AudioFrontend``.

What an x-vector recipe does to a training utterance before the features are taken: the reference's
``AddNoise`` / ``NormalizeUtterance`` (models/video_models/preprocess.py:141-179) and the four augmentation kinds its training
lists carry (train_audio.py:454: 'reverb', 'music', 'babble', 'noise' -- one convolution with a room impulse response, three additive
mixtures at an SNR).  ``WaveAugment`` keeps the noise bank and the room responses on the device, draws the random choices on the
host (``draw``) and applies them with the ``dlip_wave_*`` kernels (``__call__``: launches only) in Kaldi's order -- reverberation,
additive noise, utterance normalisation -- on a batch ``wave [B, S]`` (+ ``lengths``), each row as if it were alone.

Two deliberate differences from the reference, which divides by zero in both places: a noise slice of zero power leaves the row
untouched, and a row of zero standard deviation normalises to zeros.
"""
from __future__ import annotations

import warnings
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, lib

SNR_PASS = 9999                     # preprocess.py:168: the level that means "leave the signal alone"
AUGMENT_KEYS = ("snr_levels", "p_reverb", "keep_power", "normalize", "max_taps", "reverb")
REVERB_ROUTES = ("fir", "fft")      # the direct FIR kernel | the partitioned overlap-save transform route (4i)


def reverb_cap(route: str) -> int:
    """The longest room response the reverberation route takes; an unknown route raises ValueError."""
    if route not in REVERB_ROUTES:
        raise ValueError(f"reverb: expected one of {list(REVERB_ROUTES)}, got {route!r}")
    return _lib.DLIP_FIR_MAX_TAPS if route == "fir" else _lib.DLIP_OLS_MAX_TAPS


def parse_augment_section(section) -> Optional[dict]:
    """The keyword arguments of ``WaveAugment`` an ``augment:`` config section names (``data.augment`` of conf/audio_config.yaml), or
    None for an absent / empty one.  Unknown keys, a ``p_reverb`` outside [0, 1], an empty ``snr_levels``, a ``reverb`` other than
    ``fir`` / ``fft`` and a ``max_taps`` outside [1, the cap of the chosen route] raise ValueError.  ``reverb`` appears in the result
    only when the section names it."""
    if section is None or section is False:
        return None
    if not isinstance(section, dict):
        raise ValueError(f"augment: expected a mapping of {list(AUGMENT_KEYS)}, got {type(section).__name__}")
    unknown = sorted(set(section) - set(AUGMENT_KEYS))
    if unknown:
        raise ValueError(f"augment: unknown key(s) {unknown}; expected {list(AUGMENT_KEYS)}")
    out = {}
    if "snr_levels" in section:
        levels = section["snr_levels"]
        if not isinstance(levels, (list, tuple)) or len(levels) == 0:
            raise ValueError("augment.snr_levels: expected a non-empty list of SNR levels in dB (9999 = no noise)")
        out["snr_levels"] = tuple(float(v) for v in levels)
    p = float(section.get("p_reverb", 0.0))
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"augment.p_reverb: {p} is not a probability")
    out["p_reverb"] = p
    out["keep_power"] = bool(section.get("keep_power", True))
    out["normalize"] = bool(section.get("normalize", False))
    route = section.get("reverb", "fir")
    if route not in REVERB_ROUTES:
        raise ValueError(f"augment.reverb: expected one of {list(REVERB_ROUTES)}, got {route!r}")
    cap = reverb_cap(route)
    taps = int(section.get("max_taps", cap))
    if not 1 <= taps <= cap:
        raise ValueError(f"augment.max_taps: {taps} is outside [1, {cap}] (the cap of reverb: {route})")
    out["max_taps"] = taps
    if "reverb" in section:
        out["reverb"] = route
    return out


class WaveAugment:
    """``noise``: a 1-D float array (the bank additive noise is cut from), uploaded once.  ``rirs``: a sequence of 1-D room impulse
    responses of differing length, packed to ``[R, Lmax]`` + ``rir_len`` + ``rir_peak`` (the tap of the direct path, argmax |h|);
    responses longer than ``max_taps`` are truncated (with a warning) and their peak is taken inside the kept part; ``rir_peaks``
    names the direct-path taps explicitly.
    ``snr_levels``: the levels (dB) one is drawn from per row, 9999 = no noise.  ``p_reverb``: the probability a row is reverberated.
    ``keep_power``: the reverberated row is rescaled to the power it had.  ``normalize``: (x - mean) / std per row at the end.
    ``reverb``: the route that convolves -- ``"fir"``, the direct kernel (responses up to DLIP_FIR_MAX_TAPS, cost linear in their
    length), or ``"fft"``, the partitioned overlap-save route (up to DLIP_OLS_MAX_TAPS; DESIGN.md section 4i says from which length
    on it is the faster one).  The two agree to fp32 rounding, not bit for bit, so the choice is the caller's and never depends on
    a response's length.  ``max_taps`` defaults to the cap of the chosen route."""

    def __init__(self, noise=None, snr_levels: Sequence[float] = (-5, 0, 5, 10, 15, 20, SNR_PASS), rirs=None, p_reverb: float = 0.0,
                 keep_power: bool = True, normalize: bool = False, max_taps: Optional[int] = None, device="cuda", rir_peaks=None,
                 reverb: str = "fir"):
        if len(snr_levels) == 0:
            raise ValueError("WaveAugment: snr_levels is empty")
        if not 0.0 <= float(p_reverb) <= 1.0:
            raise ValueError(f"WaveAugment: p_reverb {p_reverb} is not a probability")
        cap = reverb_cap(reverb)
        if max_taps is None:
            max_taps = cap
        if not 1 <= int(max_taps) <= cap:
            raise ValueError(f"WaveAugment: max_taps must lie in [1, {cap}] (the cap of reverb={reverb!r}), got {max_taps}")
        self.reverb = reverb
        self.snr_levels = tuple(float(v) for v in snr_levels)
        self.p_reverb, self.keep_power, self.normalize, self.max_taps = float(p_reverb), bool(keep_power), bool(normalize), int(max_taps)
        self.device = torch.device(device)
        self.noise = None
        if noise is not None:
            self.noise = np.array(noise, dtype=np.float32)             # (a copy: the caller's array may be read-only)
            if self.noise.ndim != 1 or self.noise.size == 0:
                raise ValueError("WaveAugment: noise must be a non-empty 1-D array")
        self.rir = self.rir_len = self.rir_peak = None
        self.truncated = []                                            # indices of the responses cut to max_taps
        if rirs is not None and len(rirs) > 0:
            hs = []
            for i, h in enumerate(rirs):
                h = np.asarray(h, dtype=np.float32)
                if h.ndim != 1 or h.size == 0:
                    raise ValueError(f"WaveAugment: room response {i} must be a non-empty 1-D array")
                if h.size > self.max_taps:
                    self.truncated.append(i)
                    h = h[:self.max_taps]
                hs.append(h)
            if self.truncated:
                warnings.warn(f"WaveAugment: room response(s) {self.truncated} are longer than max_taps = {self.max_taps} and were "
                              "truncated to it (their direct-path tap is taken inside the kept part)")
            self.rir_len = np.array([h.size for h in hs], dtype=np.int32)
            self.rir_peak = np.array([int(np.argmax(np.abs(h))) for h in hs], dtype=np.int32)
            if rir_peaks is not None:                                  # the direct-path taps, where they are not the largest ones
                self.rir_peak = np.asarray(rir_peaks, dtype=np.int32).reshape(-1)
                if self.rir_peak.size != len(hs) or (self.rir_peak < 0).any() or (self.rir_peak >= self.rir_len).any():
                    raise ValueError("WaveAugment: rir_peaks must hold one tap index inside each (kept) response")
            self.rir = np.zeros((len(hs), int(self.rir_len.max())), dtype=np.float32)
            for i, h in enumerate(hs):
                self.rir[i, :h.size] = h
        if self.p_reverb > 0.0 and self.rir is None:
            raise ValueError("WaveAugment: p_reverb > 0 needs rirs")
        self._dev = None                                               # the device copies, made on the first call
        if torch.cuda.is_available() and self.device.type == "cuda":
            self._upload()

    def _upload(self):
        if self._dev is None:
            up = lambda a: None if a is None else torch.from_numpy(a).to(self.device)
            self._dev = {k: up(getattr(self, k)) for k in ("noise", "rir", "rir_len", "rir_peak")}
            self._dev["spectra"] = None
            if self.reverb == "fft" and self.rir is not None:      # the responses' partition spectra: one launch, once per bank
                R, Lmax = self.rir.shape
                nbytes = int(lib().dlip_wave_rir_spectra_bytes(R, Lmax))
                if nbytes <= 0:
                    raise _lib.DeepLipHipError(f"dlip_wave_rir_spectra_bytes refused R = {R}, Lmax = {Lmax}")
                sp = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)
                with torch.cuda.device(self.device):
                    call("dlip_wave_rir_spectra_f32", self._dev["rir"], self._dev["rir_len"], sp, nbytes, R, Lmax)
                    torch.cuda.current_stream().synchronize()      # as the copies above: whichever stream calls later finds them made
                self._dev["spectra"] = sp
        return self._dev

    # ------------------------------------------------------------------------------------------------------------ host: the draws
    def draw(self, lengths, rng: np.random.Generator) -> Dict[str, np.ndarray]:
        """The random choices of one batch, host only: ``snr_db`` float32 [B] (uniform over ``snr_levels``; all 9999 without a bank),
        ``noise_start`` int64 [B] (uniform over [0, len(noise) - n], preprocess.py:172; 0 for rows at 9999) and ``rir_idx`` int32 [B]
        (with probability ``p_reverb`` a response drawn uniformly, else -1).  A bank shorter than a row raises ValueError."""
        lens = np.asarray(lengths.tolist() if hasattr(lengths, "tolist") else list(lengths), dtype=np.int64).reshape(-1)
        B = lens.size
        if self.noise is None:
            snr = np.full(B, SNR_PASS, dtype=np.float32)
        else:
            snr = np.asarray(self.snr_levels, dtype=np.float32)[rng.integers(0, len(self.snr_levels), size=B)]
        start = np.zeros(B, dtype=np.int64)
        for b in np.nonzero(snr < SNR_PASS)[0]:
            room = self.noise.size - int(lens[b])
            if room < 0:
                raise ValueError(f"WaveAugment.draw: row {int(b)} holds {int(lens[b])} samples, the noise bank only {self.noise.size}")
            start[b] = rng.integers(0, room + 1)
        ridx = np.full(B, -1, dtype=np.int32)
        if self.rir is not None and self.p_reverb > 0.0:
            hit = rng.random(B) < self.p_reverb
            ridx = np.where(hit, rng.integers(0, self.rir.shape[0], size=B), -1).astype(np.int32)
        return {"snr_db": snr, "noise_start": start, "rir_idx": ridx}

    # ---------------------------------------------------------------------------------------------------------- device: the stages
    def __call__(self, wave: torch.Tensor, lengths=None, params=None, rng: Optional[np.random.Generator] = None) -> torch.Tensor:
        """wave [B, S] float32 (cuda) -> the augmented batch [B, S] (a new tensor; samples past a row's length are zeros).

        ``lengths``: as ``AudioFrontend``'s (host values are validated, an int32 device tensor is clamped by the kernels and never
        read on the host).  ``params``: what ``draw`` returned -- numpy arrays (copied in without synchronising) or device tensors of
        the same dtypes (a recorded step plan's inputs); None draws them here from ``rng``, which needs host lengths.  Launches only:
        nothing below synchronises or allocates outside ``ops._empty``, so the call records into a step plan."""
        ops._req(wave, "WaveAugment: wave")
        if wave.dim() != 2:
            raise ValueError(f"WaveAugment: expected wave [B, S], got {tuple(wave.shape)}")
        B, S = wave.shape
        dev = wave.device
        lens = ops.lengths_i32(lengths, dev, n=B, lo=1, hi=S)
        if params is None:
            if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
                raise ValueError("WaveAugment: lengths on the device are never read on the host; pass params=draw(host_lengths, rng)")
            params = self.draw([S] * B if lengths is None else lengths, rng if rng is not None else np.random.default_rng())
        unknown = sorted(set(params) - {"snr_db", "noise_start", "rir_idx"})
        if unknown:
            raise ValueError(f"WaveAugment: unknown params {unknown}")
        d = self._upload()
        nbytes = int(lib().dlip_wave_reverb_workspace_bytes(B, S))
        if nbytes <= 0:
            raise _lib.DeepLipHipError(f"dlip_wave_reverb_workspace_bytes refused B = {B}, S = {S}")
        if self.reverb == "fft" and d["rir"] is not None:              # the power partials and, behind them, the input spectra
            nbytes_fft = int(lib().dlip_wave_reverb_fft_workspace_bytes(B, S, d["rir"].shape[1]))
            if nbytes_fft < nbytes:
                raise _lib.DeepLipHipError(f"dlip_wave_reverb_fft_workspace_bytes refused B = {B}, S = {S}, Lmax = {d['rir'].shape[1]}")
            ws_fft = ops._empty((nbytes_fft // 8,), dev, torch.float64)
            ws = ws_fft[:nbytes // 8]
        else:
            ws = ops._empty((nbytes // 8,), dev, torch.float64)
        cur = wave
        if d["rir"] is None and isinstance(params.get("rir_idx"), np.ndarray) and (params["rir_idx"] >= 0).any():
            raise ValueError("WaveAugment: params ask for reverberation but no rirs were given")
        ridx = self._param(params, "rir_idx", torch.int32, B, dev) if d["rir"] is not None else None
        if ridx is not None:
            y = ops._empty((B, S), dev)
            R, Lmax = d["rir"].shape
            if self.reverb == "fft":
                call("dlip_wave_reverb_fft_f32", cur, lens, d["spectra"], d["rir_len"], d["rir_peak"], ridx, y, ws_fft, nbytes_fft, B, S, R, Lmax,
                     int(self.keep_power))
            else:
                call("dlip_wave_reverb_f32", cur, lens, d["rir"], d["rir_len"], d["rir_peak"], ridx, y, ws, nbytes, B, S, R, Lmax,
                     int(self.keep_power))
            cur = y
        snr = self._param(params, "snr_db", torch.float32, B, dev)
        if snr is not None and d["noise"] is not None:
            start = self._param(params, "noise_start", torch.int64, B, dev)
            if start is None:
                raise ValueError("WaveAugment: params carry snr_db but no noise_start")
            z = ops._empty((B, S), dev)
            call("dlip_wave_add_noise_f32", cur, lens, d["noise"], d["noise"].numel(), start, snr, z, ws, nbytes, B, S)
            cur = z
        if self.normalize:
            out = ops._empty((B, S), dev)
            call("dlip_wave_normalize_f32", cur, lens, out, ws, nbytes, B, S)
            cur = out
        if cur is wave:
            raise ValueError("WaveAugment: nothing to apply (no noise bank, no room responses, normalize off)")
        return cur

    @staticmethod
    def _param(params, name, dtype, B, dev):
        v = params.get(name)
        if v is None:
            return None
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                v = v.to(dev, non_blocking=True)
        else:
            v = torch.from_numpy(np.ascontiguousarray(v)).to(dev, non_blocking=True)
        if v.dtype != dtype or v.numel() != B:
            raise TypeError(f"WaveAugment: params[{name!r}] must hold {B} values of {dtype}, got {v.numel()} of {v.dtype}")
        return v.contiguous()
