"""fp64 restatement of the resampler's definition (include/deeplip_hip.h, ABI 63), vectorised numpy, for the tests:

    n_out = ceil(n up / down),   y[m] = sum_i x[i] h[c + m down - i up],   c = (L - 1) // 2,   x = 0 outside [0, n), h = 0 outside [0, L)

For output m the products that can be non-zero are those with 0 <= k = c + m down - i up < L: i = q // up - j, k = q % up + j up for
j = 0 .. ceil(L / up) - 1, q = c + m down.  Written from the definition, not from the package's code.
"""
import numpy as np


def n_out(n, up, down):
    return -((-int(n) * int(up)) // int(down))


def resample(x, up, down, h, m=None, with_abs=False):
    """y[m] in fp64 for the outputs ``m`` (default: all n_out of them); ``with_abs``: also sum_i |x[i]| |h[...]| per output, the scale
    of the forward error bound of an fma chain."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    n, L = x.size, h.size
    c = (L - 1) // 2
    m = np.arange(n_out(n, up, down), dtype=np.int64) if m is None else np.asarray(m, dtype=np.int64)
    K = -(-L // up)
    q = c + m * np.int64(down)
    y = np.zeros(m.size, dtype=np.float64)
    a = np.zeros(m.size, dtype=np.float64)
    for j in range(K):                                   # one term of every output per turn: memory stays O(outputs)
        i = q // up - j
        k = q % up + j * up
        ok = (i >= 0) & (i < n) & (k < L)
        p = np.where(ok, x[np.clip(i, 0, n - 1)] * h[np.clip(k, 0, L - 1)], 0.0)
        y += p
        a += np.abs(p)
    return (y, a) if with_abs else y
