"""Lip-clip augmentation (include/deeplip_hip.h) in numpy: the definition the device kernels are held to.  The
integers are exactly the header's; the base pixel is the oracle's ingest arithmetic (numpy float32, the order of
``oracle.deeplip_oracle.video_preprocess_train_u8``); the blend is numpy float32, two products and one sum."""
import numpy as np

MAX_MASKS = 4
DRAWS = 6 * MAX_MASKS
TOP = 2 ** 31 - 1                   # the largest draw


def pick(r, m):
    """(int64(r) m) >> 31 in [0, m); a negative draw counts as 0."""
    return (max(int(r), 0) * int(m)) >> 31


def row_len(length, T):
    return int(T) if length is None else min(max(int(length), 1), int(T))


def base_clip(frames_u8, crop, cp=None):
    """[T,H,W] gray or [T,3,H,W] RGB uint8 -> [T,crop,crop] float32: Normalize(0,255) -> crop at (oy, ox) (clamped into the frame;
    None: CenterCrop, the margin halved and rounded down) -> flip -> Normalize(0.421, 0.165), in the oracle's order."""
    x = frames_u8.astype(np.float32)
    if x.ndim == 4:
        x = np.float32(0.299) * x[:, 0] + np.float32(0.587) * x[:, 1] + np.float32(0.114) * x[:, 2]
    x = x / np.float32(255.0)
    h, w = x.shape[-2:]
    oy, ox, flip = (h - crop) // 2, (w - crop) // 2, 0
    if cp is not None:
        oy, ox, flip = min(max(int(cp[0]), 0), h - crop), min(max(int(cp[1]), 0), w - crop), int(cp[2])
    x = x[:, oy:oy + crop, ox:ox + crop]
    if flip:
        x = x[:, :, ::-1]
    return ((x - np.float32(0.421)) / np.float32(0.165)).astype(np.float32)


def time_cap(n, time_width, time_ratio):
    return min(int(time_width), int(np.floor(np.float64(time_ratio) * np.float64(n))))


def time_masks(n, row, n_time, time_width, time_ratio):
    """[(t0, w)] of a clip of n frames."""
    cap = time_cap(n, time_width, time_ratio)
    out = []
    for i in range(n_time):
        w = pick(row[2 * i], cap + 1)
        out.append((pick(row[2 * i + 1], n - w + 1), w))
    return out


def cutouts(OH, OW, row, n_cut, cut_size):
    """[(y0, x0, h, w)] in output coordinates."""
    out = []
    for j in range(n_cut):
        d = row[2 * MAX_MASKS + 4 * j:2 * MAX_MASKS + 4 * j + 4]
        h, w = min(pick(d[0], cut_size + 1), OH), min(pick(d[1], cut_size + 1), OW)
        out.append((pick(d[2], OH - h + 1), pick(d[3], OW - w + 1), h, w))
    return out


def masked(A, n, row, n_time=0, time_width=0, time_ratio=1.0, n_cut=0, cut_size=0, fill=0):
    """Steps 1-3 on one clip.  A float32 [T, OH, OW] (frames t >= n are never looked at) -> (A' float32 [T, OH, OW] with zeros from n
    on, mask bool [T, OH, OW], the mean in fp64 before its one rounding)."""
    T, OH, OW = A.shape
    row = [int(v) for v in row]
    mean = A[:n].astype(np.float64).sum() / (n * OH * OW)
    fillv = np.float32(mean) if fill == 1 else np.float32(0.0)
    m = np.zeros((T, OH, OW), dtype=bool)
    for t0, w in time_masks(n, row, n_time, time_width, time_ratio):
        m[t0:t0 + w] = True
    for y0, x0, h, w in cutouts(OH, OW, row, n_cut, cut_size):
        m[:n, y0:y0 + h, x0:x0 + w] = True
    out = np.zeros((T, OH, OW), dtype=np.float32)
    out[:n] = np.where(m[:n], fillv, A[:n])
    return out, m, mean


def clip_augment(src, lengths, draws, crop=None, clip_params=None, perm=None, lam=None, **kw):
    """src: uint8 [B,T,Hs,Ws] / [B,T,3,Hs,Ws] (with ``crop``, ``clip_params`` [B,4] or None) or float32 [B,1,T,H,W] -> dict: ``y``
    float32 [B,1,T,OH,OW], ``mask`` bool (pixels of y that hold a fill value of either operand), ``mean`` float64 [B]."""
    src = np.asarray(src)
    B = src.shape[0]
    if src.dtype == np.uint8:
        clips = [base_clip(src[b], crop, None if clip_params is None else clip_params[b]) for b in range(B)]
    else:
        clips = [np.where(np.arange(src.shape[2])[:, None, None] < row_len(None if lengths is None else lengths[b], src.shape[2]),
                          src[b, 0], np.float32(0.0)).astype(np.float32) for b in range(B)]
    T = clips[0].shape[0]
    ns = [row_len(None if lengths is None else lengths[b], T) for b in range(B)]
    done = [masked(clips[b], ns[b], draws[b], **kw) for b in range(B)]
    y = np.zeros((B, 1) + clips[0].shape, dtype=np.float32)
    mask = np.zeros(y.shape, dtype=bool)
    for b in range(B):
        a, m, _ = done[b]
        p = int(perm[b]) if perm is not None else b
        if perm is None or p == b or not 0 <= p < B:
            y[b, 0], mask[b, 0] = a, m
            continue
        l32 = np.float32(lam)
        mu = np.float32(1.0) - l32
        u, mp, _ = done[p]                                              # zeros from n_p on
        y[b, 0, :ns[b]] = (l32 * a[:ns[b]]) + (mu * u[:ns[b]])
        mask[b, 0, :ns[b]] = m[:ns[b]] | mp[:ns[b]]
    return {"y": y, "mask": mask, "mean": np.array([d[2] for d in done])}
