"""The fp64 restatement of DESIGN.md section 4f (sliding-window CMN, energy VAD, frame selection) in plain numpy, one utterance at a
time, sequential sums -- what tests/test_voiced_frames_gpu.py holds the kernels to.  Kaldi is not a dependency and the reference
ships no source for apply-cmvn-sliding / select-voiced-frames (conf/audio_config.yaml:21,25): this file restates the definition, it is
not a recording of either."""
import numpy as np

from deeplip_amd.voiced_frames import VAD_DEFAULTS, window_bounds


def _seq_sum(a):
    """Sum over the last axis, front to back in fp64 (np.cumsum accumulates sequentially; np.sum adds pairwise)."""
    return np.cumsum(a, axis=-1)[..., -1]


def cmn(x, window, center=True, min_window=100, norm_vars=False):
    """x [C, n] float32 (one utterance) -> float32 [C, n]."""
    x64 = np.asarray(x, dtype=np.float64)
    C, n = x64.shape
    out = np.empty((C, n), dtype=np.float32)
    for t in range(n):
        b, e = window_bounds(t, n, window, center, min_window)
        w = e - b
        mean = _seq_sum(x64[:, b:e]) / w
        d = x64[:, t] - mean
        if norm_vars:
            if w == 1:
                d = np.zeros(C)
            else:
                var = np.maximum(_seq_sum(x64[:, b:e] * x64[:, b:e]) / w - mean * mean, 1e-10)
                d = d * (1.0 / np.sqrt(var))
        out[:, t] = d.astype(np.float32)
    return out


def vad(e, energy_threshold=VAD_DEFAULTS["energy_threshold"], energy_mean_scale=VAD_DEFAULTS["energy_mean_scale"],
        frames_context=VAD_DEFAULTS["frames_context"], proportion_threshold=VAD_DEFAULTS["proportion_threshold"]):
    """e [n] float32 (one utterance's log-energy) -> (voiced bool [n], thr float32, the smallest |e[t] - thr|)."""
    e = np.asarray(e, dtype=np.float32)
    n = e.shape[0]
    thr = np.float32(energy_threshold)
    if energy_mean_scale != 0.0:
        thr = np.float32(np.float64(energy_threshold) + np.float64(energy_mean_scale) * (_seq_sum(e.astype(np.float64)) / n))
    above = e > thr
    voiced = np.zeros(n, dtype=bool)
    p = np.float32(proportion_threshold)
    for t in range(n):
        lo, hi = max(0, t - frames_context), min(n - 1, t + frames_context)
        num, den = int(above[lo:hi + 1].sum()), hi - lo + 1
        voiced[t] = np.float32(num) >= np.float32(den) * p            # the product in fp32, Kaldi's BaseFloat
    return voiced, thr, float(np.abs(e.astype(np.float64) - np.float64(thr)).min())


def select(y, voiced, min_keep=1):
    """y [C, n], voiced bool [n] -> (packed [C, n] with the kept frames in front and zeros behind, out_len, fallback)."""
    n = y.shape[1]
    V = int(voiced.sum())
    fallback = V < min_keep
    keep = np.ones(n, dtype=bool) if fallback else voiced
    out = np.zeros_like(y)
    k = int(keep.sum())
    out[:, :k] = y[:, keep]
    return out, k, int(fallback)
