"""SpecAugment (include/deeplip_hip.h) in numpy: the definition the device kernel is held to.  The integers are
exactly the header's; the warp's interpolation is taken in fp64 on the fp32 inputs (the device rounds to fp32: tests bound the gap)."""
import numpy as np

MAX_MASKS = 8
DRAWS = 2 + 4 * MAX_MASKS
TOP = 2 ** 31 - 1                   # the largest draw


def pick(r, m):
    """(int64(r) m) >> 31 in [0, m); a negative draw counts as 0."""
    return (max(int(r), 0) * int(m)) >> 31


def row_len(length, NF):
    return int(NF) if length is None else min(max(int(length), 1), int(NF))


def warp_params(n, W, r0, r1):
    """(c, c') of a row of n frames, or None where the row is not warped at all (We < 1); c == c' means d == 0."""
    We = min(int(W), (n - 3) // 2) if n >= 3 else 0
    if We < 1:
        return None
    c = We + 1 + pick(r0, n - 2 - 2 * We)
    return c, c + pick(r1, 2 * We + 1) - We


def warp_positions(n, c, cp):
    """s[t], t < n, in fp64: 64-bit integer products, one fp64 division."""
    t = np.arange(n, dtype=np.int64)
    left = t <= cp
    num = np.where(left, t * c, (t - cp) * (n - 1 - c)).astype(np.float64)
    den = np.where(left, cp, n - 1 - cp).astype(np.float64)
    return np.where(left, 0.0, float(c)) + num / den


def freq_masks(C, row, n_freq, freq_width):
    out = []
    for j in range(n_freq):
        w = pick(row[2 + 2 * j], min(freq_width, C) + 1)
        f0 = pick(row[3 + 2 * j], C - w + 1)
        out.append((f0, w))
    return out


def time_cap(n, time_width, time_ratio):
    return min(int(time_width), int(np.floor(np.float64(time_ratio) * np.float64(n))))


def time_masks(n, row, n_time, time_width, time_ratio):
    cap = time_cap(n, time_width, time_ratio)
    out = []
    for j in range(n_time):
        w = pick(row[2 + 2 * MAX_MASKS + 2 * j], cap + 1)
        t0 = pick(row[3 + 2 * MAX_MASKS + 2 * j], n - w + 1)
        out.append((t0, w))
    return out


def spec_augment(x, lengths, draws, warp=0, n_freq=0, freq_width=0, n_time=0, time_width=0, time_ratio=1.0, fill=0):
    """x float32 [B, C, NF] -> dict: ``y`` float64 [B, C, NF] (exact fp32 values wherever no interpolation took place), ``mask`` bool
    (the masked entries), ``interp`` bool (entries the warp interpolated, i.e. not a plain copy), ``scale`` float64 (max(|x[f, i]|,
    |x[f, i + 1]|) of an interpolated entry, 0 elsewhere), ``mean`` float64 [B] (the fill value of fill = 1 before its one rounding)."""
    x = np.asarray(x, dtype=np.float32)
    B, C, NF = x.shape
    y = np.zeros((B, C, NF), dtype=np.float64)
    mask = np.zeros((B, C, NF), dtype=bool)
    interp = np.zeros((B, C, NF), dtype=bool)
    scale = np.zeros((B, C, NF), dtype=np.float64)
    mean = np.zeros(B, dtype=np.float64)
    for b in range(B):
        n = row_len(None if lengths is None else lengths[b], NF)
        row = [int(v) for v in draws[b]]
        xb = x[b, :, :n].astype(np.float64)
        mean[b] = xb.sum() / (C * n)
        v = xb.copy()
        wp = warp_params(n, warp, row[0], row[1])
        if wp is not None and wp[0] != wp[1]:
            s = warp_positions(n, *wp)
            i = np.minimum(np.floor(s).astype(np.int64), n - 2)
            a = s - i
            x0, x1 = xb[:, i], xb[:, i + 1]
            v = x0 + a[None, :] * (x1 - x0)
            a32 = a.astype(np.float32)
            v[:, a32 == 0] = x0[:, a32 == 0]            # a == 0 and a == 1 take the sample itself
            v[:, a32 == 1] = x1[:, a32 == 1]
            moved = (a32 != 0) & (a32 != 1)
            interp[b, :, :n] = moved[None, :]
            scale[b, :, :n] = np.where(moved[None, :], np.maximum(np.abs(x0), np.abs(x1)), 0.0)
        m = np.zeros((C, n), dtype=bool)
        for f0, w in freq_masks(C, row, n_freq, freq_width):
            m[f0:f0 + w, :] = True
        for t0, w in time_masks(n, row, n_time, time_width, time_ratio):
            m[:, t0:t0 + w] = True
        fillv = float(np.float32(mean[b])) if fill == 1 else 0.0
        y[b, :, :n] = np.where(m, fillv, v)
        mask[b, :, :n] = m
    interp &= ~mask
    scale[mask] = 0.0
    return {"y": y, "mask": mask, "interp": interp, "scale": scale, "mean": mean}
