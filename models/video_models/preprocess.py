"""Drop-in module path of the reference's waveform transforms (models/video_models/preprocess.py:141-179): ``NormalizeUtterance``
and ``AddNoise`` with the reference's constructor signatures, applied to CUDA tensors by the ``dlip_wave_*`` kernels
(deeplip_amd/augment.py).  The image transforms of that file (RandomCrop, HorizontalFlip, ...) live in
deeplip_amd.frontend.VideoFrontend.

A signal is a CUDA float32 tensor ``[n]`` (one utterance, as the reference's loaders pass it) or a batch ``[B, S]`` with optional
``lengths=``; the result has the same shape.  Two deliberate differences, both where the reference divides by zero: ``AddNoise``
leaves a row untouched when its noise slice has no power, and ``NormalizeUtterance`` returns zeros for a row of zero deviation."""
from __future__ import annotations

import random

import numpy as np

from deeplip_amd.augment import SNR_PASS, WaveAugment


def _rows(signal):
    if signal.dim() not in (1, 2):
        raise ValueError(f"expected a signal [n] or a batch [B, S], got {tuple(signal.shape)}")
    return signal.reshape(1, -1) if signal.dim() == 1 else signal


class NormalizeUtterance():
    """Normalize per raw audio by removing the mean and divided by the standard deviation (preprocess.py:141-147)."""

    def __init__(self):
        self._aug = WaveAugment(normalize=True)

    def __call__(self, signal, lengths=None):
        return self._aug(_rows(signal), lengths, params={}).reshape(signal.shape)


class AddNoise(object):
    """Add SNR noise [-1, 1] (preprocess.py:150-179).  The draws come from Python's ``random`` module in the reference's order --
    ``random.choice(snr_levels)``, then ``random.randint(0, len(noise) - len(signal))`` unless the level is 9999 -- once per row, so
    a run seeded like the reference's makes the reference's choices."""

    def __init__(self, noise, snr_levels=[-5, 0, 5, 10, 15, 20, 9999]):
        noise = noise.detach().cpu().numpy() if hasattr(noise, "detach") else np.asarray(noise)
        assert noise.dtype in [np.float32, np.float64], "noise only supports float data type"
        self.noise = noise
        self.snr_levels = snr_levels
        self._aug = WaveAugment(noise=noise, snr_levels=snr_levels)

    def draw(self, lengths):
        """(snr_db, noise_start) of the rows, from ``random`` as AddNoise.__call__ of the reference consumes it."""
        snr, start = [], []
        for n in lengths:
            snr_target = random.choice(self.snr_levels)                              # preprocess.py:167
            snr.append(snr_target)
            start.append(0 if snr_target == SNR_PASS else random.randint(0, len(self.noise) - int(n)))   # :172
        return np.asarray(snr, dtype=np.float32), np.asarray(start, dtype=np.int64)

    def __call__(self, signal, lengths=None):
        x = _rows(signal)
        if lengths is None:
            host = [x.shape[1]] * x.shape[0]
        elif hasattr(lengths, "is_cuda") and lengths.is_cuda:
            raise ValueError("AddNoise: the draw needs the lengths on the host (a list, an array or a CPU tensor)")
        else:
            host = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        snr, start = self.draw(host)
        return self._aug(x, lengths, params={"snr_db": snr, "noise_start": start}).reshape(signal.shape)
