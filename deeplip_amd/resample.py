"""Waveform resampling on the device, in front of ``AudioFrontend`` (ABI 63): rate conversion and speed
perturbation.

The reference's test loader resamples a file whose rate differs from the configured one (models/audio_models/datasets.py:459-463,
``librosa.resample(data, rate, self.rate)``), and an x-vector recipe perturbs the speed of a training utterance (sox ``speed 0.9 /
1.0 / 1.1``) beside reverberation and additive noise (deeplip_amd/augment.py).  Both are one operation, a rational polyphase FIR
resampler: for a row of ``n`` samples, a ratio ``up / down`` in lowest terms and a prototype ``h[0 .. L)`` with centre
``c = (L - 1) // 2``

    n_out = ceil(n up / down),    y[m] = sum_i x[i] h[c + m down - i up],   0 <= m < n_out   (x, h zero outside their supports)

which is ``scipy.signal.resample_poly(x, up, down)`` when ``h`` is scipy's default design (``design`` below: a Kaiser-windowed sinc,
beta 5, 2 * 10 * max(up, down) + 1 taps).  Parity with librosa's own filter (resampy's ``kaiser_best``) is UNPINNED: neither package is a
dependency and nothing upstream pins the result; include/deeplip_hip.h with DESIGN.md 4g is the definition.  ``Resample`` (one ratio)
and ``SpeedPerturb`` (a bank of ratios, one drawn per row) run the ``dlip_wave_resample_f32`` kernel on a batch ``wave [B, S]``
(+ ``lengths``) and hand back a NEW length vector that lives on the device, as ``VoicedFrames`` does: a row leaves with a different
length the host never reads.
"""
from __future__ import annotations

from fractions import Fraction
from math import gcd
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import call, lib

SPEED_KEYS = ("speeds",)
SPEED_RANGE = (0.5, 2.0)


def _reduced(up, down) -> Tuple[int, int]:
    if isinstance(up, bool) or isinstance(down, bool) or int(up) != up or int(down) != down or int(up) < 1 or int(down) < 1:
        raise ValueError(f"resample: up / down must be positive integers, got {up!r} / {down!r}")
    up, down = int(up), int(down)
    g = gcd(up, down)
    return up // g, down // g


def design(up: int, down: int, half_width: int = 10, beta: float = 5.0) -> Tuple[int, int, np.ndarray]:
    """(up, down, h float64): the ratio in lowest terms and scipy's default prototype for it -- ``L = 2 half_width max(up, down) + 1``
    taps of a sinc low-pass with cutoff ``1 / max(up, down)`` of Nyquist under a Kaiser window, normalised to unit DC gain and
    multiplied by ``up`` (``up * firwin(L, 1 / max, window=('kaiser', beta))``).  ``up = down = 1`` gives ``h = [1.0]``."""
    up, down = _reduced(up, down)
    if up == 1 and down == 1:
        return 1, 1, np.ones(1, dtype=np.float64)
    mx = max(up, down)
    L = 2 * int(half_width) * mx + 1
    m = np.arange(L, dtype=np.float64) - (L - 1) / 2.0
    fc = 1.0 / mx
    h = fc * np.sinc(fc * m) * np.kaiser(L, float(beta))
    h /= h.sum()
    return up, down, h * up


def out_len(n: int, up: int, down: int) -> int:
    """ceil(n up / down): the samples an n-sample row leaves with."""
    return -((-int(n) * int(up)) // int(down))


def in_len(m: int, up: int, down: int) -> int:
    """The shortest row that leaves with at least m samples: out_len(n) >= m  <=>  n >= ((m - 1) down) // up + 1."""
    return ((int(m) - 1) * int(down)) // int(up) + 1 if m > 0 else 0


def pack_table(h: np.ndarray, up: int) -> Tuple[np.ndarray, int]:
    """(tab float32 [up, Kp], K): the polyphase table ``tab[r][j] = h[r + j up]`` of the kernel, K = ceil(L / up) taps per phase in
    rows of Kp = K | 1 words (an odd stride; the pad word is zero and never read)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    K = -(-h.size // up)
    full = np.zeros(K * up, dtype=np.float64)
    full[:h.size] = h
    tab = np.zeros((up, K | 1), dtype=np.float32)
    tab[:, :K] = full.reshape(K, up).T
    return tab, K


def parse_speed_perturb_section(section) -> Optional[dict]:
    """The keyword arguments of ``SpeedPerturb`` a ``speed_perturb:`` config section names (``data.speed_perturb`` of
    conf/audio_config.yaml), or None for an absent one.  The section holds exactly the key ``speeds``, a non-empty list of values in
    [0.5, 2.0]; unknown keys and bad values raise ValueError."""
    if section is None or section is False:
        return None
    if not isinstance(section, dict):
        raise ValueError(f"speed_perturb: expected a mapping of {list(SPEED_KEYS)}, got {type(section).__name__}")
    unknown = sorted(set(section) - set(SPEED_KEYS))
    if unknown:
        raise ValueError(f"speed_perturb: unknown key(s) {unknown}; expected {list(SPEED_KEYS)}")
    if "speeds" not in section:
        raise ValueError("speed_perturb: the section needs the key 'speeds'")
    return {"speeds": _check_speeds(section["speeds"], "speed_perturb.speeds")}


def _check_speeds(speeds, what) -> Tuple[float, ...]:
    if not isinstance(speeds, (list, tuple)) or len(speeds) == 0:
        raise ValueError(f"{what}: expected a non-empty list of speed factors in [{SPEED_RANGE[0]}, {SPEED_RANGE[1]}]")
    out = []
    for s in speeds:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not SPEED_RANGE[0] <= float(s) <= SPEED_RANGE[1]:
            raise ValueError(f"{what}: {s!r} is not a speed factor in [{SPEED_RANGE[0]}, {SPEED_RANGE[1]}]")
        out.append(float(s))
    return tuple(out)


def speed_ratio(speed: float) -> Tuple[int, int]:
    """(up, down) of a speed factor: speed s makes the row 1 / s as long, s taken as ``Fraction(s).limit_denominator(100)`` --
    0.9 -> 10/9, 1.1 -> 10/11, 1.0 -> 1/1."""
    f = Fraction(float(speed)).limit_denominator(100)
    return f.denominator, f.numerator


class _Bank:
    """Q ratios with their prototypes, packed for ``dlip_wave_resample_f32``: ``bank`` int32 [Q, 4] = (up, down, c, K), ``tabs`` float32
    [Q, tab_stride], the tile every ratio of the bank fits at and the widest input span of a tile.  A ratio the kernel's LDS budget
    cannot hold raises ValueError here, at construction."""

    def __init__(self, filters: Sequence[Tuple[int, int, np.ndarray]], device, who: str):
        self.device = torch.device(device)
        self.ratios, tabs, rows, tiles = [], [], [], []
        cap = _lib.DLIP_RESAMPLE_MAX_FACTOR
        for up, down, h in filters:
            h = np.asarray(h, dtype=np.float64)
            if h.ndim != 1 or h.size == 0:
                raise ValueError(f"{who}: the prototype filter must be a non-empty 1-D array")
            if gcd(up, down) != 1 or not (1 <= up <= cap and 1 <= down <= cap):
                raise ValueError(f"{who}: the ratio {up}/{down} must be in lowest terms with both factors in [1, {cap}]")
            tile = int(lib().dlip_wave_resample_fits(up, down, h.size))
            if tile <= 0:
                raise ValueError(f"{who}: the ratio {up}/{down} with {h.size} taps does not fit the kernel's LDS budget "
                                 f"({_lib.DLIP_RESAMPLE_LDS_WORDS} words for the polyphase table and a tile's input span)")
            tab, K = pack_table(h, up)
            tabs.append(tab.reshape(-1))
            rows.append((up, down, (h.size - 1) // 2, K))
            tiles.append(tile)
            self.ratios.append((up, down))
        self.filters = [np.asarray(h, dtype=np.float64) for _, _, h in filters]
        self.tile = min(tiles)
        self.tab_stride = max(t.size for t in tabs)
        self.span_words = max(int(lib().dlip_wave_resample_span_words(up, down, K, self.tile)) for up, down, _, K in rows)
        if self.tab_stride + self.span_words > _lib.DLIP_RESAMPLE_LDS_WORDS:
            raise ValueError(f"{who}: the ratios {self.ratios} do not fit the kernel's LDS budget together (the largest table beside "
                             "the widest input span)")
        self.bank = np.asarray(rows, dtype=np.int32)
        self.tabs = np.zeros((len(tabs), self.tab_stride), dtype=np.float32)
        for q, t in enumerate(tabs):
            self.tabs[q, :t.size] = t
        self._dev = None
        if torch.cuda.is_available() and self.device.type == "cuda":
            self._upload()

    def _upload(self):
        if self._dev is None:
            self._dev = (torch.from_numpy(self.tabs).to(self.device), torch.from_numpy(self.bank).to(self.device))
        return self._dev

    def launch(self, wave: torch.Tensor, lens, ridx: torch.Tensor, S_out: int, who: str):
        B, S = wave.shape
        tabs, bank = self._upload()
        out = ops._empty((B, S_out), wave.device)
        out_lengths = ops._empty((B,), wave.device, torch.int32)
        call("dlip_wave_resample_f32", wave, lens, tabs, bank, ridx, out, out_lengths, B, S, S_out, len(self.ratios), self.tab_stride,
             self.span_words, self.tile, what=f"{who}: dlip_wave_resample_f32")
        return out, out_lengths


def _wave_arg(wave, lengths, who):
    ops._req(wave, f"{who}: wave")
    if wave.dim() != 2:
        raise ValueError(f"{who}: expected wave [B, S], got {tuple(wave.shape)}")
    B, S = wave.shape
    return B, S, ops.lengths_i32(lengths, wave.device, n=B, lo=1, hi=S)


class Resample:
    """One ratio: ``orig_rate`` -> ``new_rate`` (integers; the ratio is reduced by their gcd).  ``filter``: a caller's prototype ``h``
    (centre ``(L - 1) // 2``) instead of ``design``'s.  Equal rates raise ValueError: there is nothing to do."""

    def __init__(self, orig_rate: int, new_rate: int, device="cuda", filter=None):
        up, down = _reduced(new_rate, orig_rate)
        if up == down:
            raise ValueError(f"Resample: orig_rate == new_rate == {orig_rate}: nothing to apply (leave the stage out instead)")
        self.orig_rate, self.new_rate = int(orig_rate), int(new_rate)
        self.up, self.down = up, down
        h = design(up, down)[2] if filter is None else np.asarray(filter, dtype=np.float64)
        self._bank = _Bank([(up, down, h)], device, "Resample")
        self.h, self.tile = self._bank.filters[0], self._bank.tile

    def out_len(self, n: int) -> int:
        return out_len(n, self.up, self.down)

    def __call__(self, wave: torch.Tensor, lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """wave [B, S] float32 (cuda) -> ``(wave' [B, out_len(S)], lengths' int32 device [B])``: row b's first lengths'[b] =
        out_len(lengths[b]) samples, exact zeros behind them.  ``lengths``: as ``AudioFrontend``'s (host values are validated, an
        int32 device tensor is clamped by the kernel and never read on the host).  Launches only, buffers from ``ops._empty``: the
        call records into a step plan and replays with new data and lengths."""
        B, S, lens = _wave_arg(wave, lengths, "Resample")
        ridx = ops._empty((B,), wave.device, torch.int32)
        ridx.zero_()
        return self._bank.launch(wave, lens, ridx, self.out_len(S), "Resample")


class SpeedPerturb:
    """``speeds``: the factors one is drawn from per row (sox ``speed``); speed s resamples the row by ``speed_ratio(s)`` -- 0.9 makes
    it 10/9 as long (slower, lower), 1.1 makes it 10/11 as long, 1.0 leaves the samples as they are (the ratio 1/1, h = [1.0])."""

    def __init__(self, speeds: Sequence[float] = (0.9, 1.0, 1.1), device="cuda"):
        self.speeds = _check_speeds(list(speeds), "SpeedPerturb: speeds")
        self.ratios = [speed_ratio(s) for s in self.speeds]
        self._bank = _Bank([design(up, down) for up, down in self.ratios], device, "SpeedPerturb")
        self.tile = self._bank.tile

    def draw(self, B: int, rng: np.random.Generator) -> Dict[str, np.ndarray]:
        """The random choices of one batch, host only: ``speed_idx`` int32 [B], uniform over ``speeds``."""
        return {"speed_idx": rng.integers(0, len(self.speeds), size=int(B)).astype(np.int32)}

    def out_samples(self, S: int) -> int:
        """out_len(S) of the slowest speed: the width that holds every row of an S-sample batch."""
        return max(out_len(S, up, down) for up, down in self.ratios)

    def in_samples(self, out_samples: int) -> int:
        """The input width that yields at least ``out_samples`` outputs at every speed."""
        return max(in_len(out_samples, up, down) for up, down in self.ratios)

    def __call__(self, wave: torch.Tensor, lengths=None, params=None, out_samples: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """wave [B, S] float32 (cuda) -> ``(wave' [B, S_out], lengths' int32 device [B])``, row b resampled at the speed
        ``params["speed_idx"][b]`` names (a negative index: the row passes through) and cut at ``S_out`` = ``out_samples`` (default:
        ``self.out_samples(S)``).  ``params``: what ``draw`` returned -- a numpy array (copied in without synchronising) or an int32
        device tensor (a recorded step plan's input).  Launches only."""
        B, S, lens = _wave_arg(wave, lengths, "SpeedPerturb")
        if params is None or sorted(params) != ["speed_idx"]:
            raise ValueError(f"SpeedPerturb: params must hold exactly 'speed_idx' (pass params=draw(B, rng)), got "
                             f"{None if params is None else sorted(params)}")
        v = params["speed_idx"]
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                v = v.to(wave.device, non_blocking=True)
        else:
            v = np.ascontiguousarray(v)
            if v.dtype == np.int32 and v.size and int(v.max()) >= len(self.speeds):
                raise ValueError(f"SpeedPerturb: speed_idx holds {int(v.max())}, there are {len(self.speeds)} speeds")
            v = torch.from_numpy(v).to(wave.device, non_blocking=True)
        if v.dtype != torch.int32 or v.numel() != B:
            raise TypeError(f"SpeedPerturb: params['speed_idx'] must hold {B} values of torch.int32, got {v.numel()} of {v.dtype}")
        S_out = self.out_samples(S) if out_samples is None else int(out_samples)
        if S_out < 1:
            raise ValueError(f"SpeedPerturb: out_samples must be >= 1, got {S_out}")
        return self._bank.launch(wave, lens, v.contiguous(), S_out, "SpeedPerturb")


class ResampledGeometry:
    """The ``wave_geometry`` of a ``RaggedExtractor`` whose ``audio_fn`` resamples in front of its front-end: every answer is in
    SOURCE-rate samples.  ``frontend``: the ``AudioFrontend`` (or any object with its geometry methods) at the target rate;
    ``resample``: the ``Resample`` in front of it (``up``, ``down``)."""

    def __init__(self, frontend, resample):
        self.frontend, self.up, self.down = frontend, int(resample.up), int(resample.down)
        # the front-end's frame at the source rate: what a "recording" at that rate is cut on
        self.frame_len = max(1, int(round(frontend.frame_len * self.down / self.up)))
        self.frame_step = max(1, int(round(frontend.frame_step * self.down / self.up)))

    @property
    def min_samples(self) -> int:
        return max(1, in_len(int(getattr(self.frontend, "min_samples", 1)), self.up, self.down))

    def frames_for_samples(self, n: int) -> int:
        return int(self.frontend.frames_for_samples(out_len(n, self.up, self.down)))

    def samples_for_frames(self, T: int) -> int:
        """The longest source length that still frames into T: out_len(n) <= M  <=>  n <= (M down) // up, M the front-end's longest
        T-frame signal."""
        return max(1, (int(self.frontend.samples_for_frames(T)) * self.down) // self.up)
