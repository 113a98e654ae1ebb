"""The yardstick of ``arch: sincnet``: an fp64 torch restatement of the definition -- the taps, the frame-level log band
energies of a ragged batch, and the encoder behind them.  Everything is differentiable by torch's autograd; it imports nothing from
the code under test.

Layouts: waveforms [B, S], taps g [F, L], features [B, F, NF] (frames at or past a row's count are zeros)."""
import math

import numpy as np
import torch
import torch.nn.functional as F


def num_frames(n, frame_len, frame_step):
    """sigproc.framesig's count."""
    return 1 if n <= frame_len else 1 + int(math.ceil((1.0 * n - frame_len) / frame_step))


def mel_edges(n_filters, rate, min_low_hz=50.0, min_band_hz=50.0):
    """(low_hz_, band_hz_) of the widely used layer's initialisation: mel-spaced edges between 30 Hz and rate / 2 - (min_low + min_band)."""
    to_mel = lambda hz: 2595.0 * np.log10(1.0 + hz / 700.0)
    to_hz = lambda mel: 700.0 * (10.0 ** (mel / 2595.0) - 1.0)
    hz = to_hz(np.linspace(to_mel(30.0), to_mel(rate / 2.0 - (min_low_hz + min_band_hz)), n_filters + 1))
    return hz[:-1], np.diff(hz)


def taps(low_hz, band_hz, L, rate, min_low_hz=50.0, min_band_hz=50.0):
    """low_hz, band_hz fp64 [F] or [F, 1] -> g [F, L], even in m = l - (L - 1) / 2 (the half m >= 1 is computed and mirrored)."""
    low, band = low_hz.reshape(-1, 1).double(), band_hz.reshape(-1, 1).double()
    H = (L - 1) // 2
    f1 = min_low_hz + low.abs()
    f2 = torch.clamp(f1 + min_band_hz + band.abs(), min_low_hz, rate / 2.0)
    m = torch.arange(1, H + 1, dtype=torch.float64, device=low.device).view(1, -1)
    n = m / rate
    w = 0.54 - 0.46 * torch.cos(2.0 * math.pi * (H + m) / (L - 1))
    right = w * (torch.sin(2.0 * math.pi * f2 * n) - torch.sin(2.0 * math.pi * f1 * n)) / ((math.pi * n) * 2.0 * (f2 - f1))
    return torch.cat([right.flip(1), torch.ones_like(low), right], dim=1)


def features(wave, lengths, g, frame_len, frame_step, eps=1e-6):
    """wave fp64 [B, S], lengths (ints or None) -> y [B, F, NF], the definition term by term: each row on its own samples (zero outside
    [0, len)), z by an explicit shift-and-add over the taps, e the mean over the frame of z^2 at positions inside the row."""
    B, S = wave.shape
    Fn, L = g.shape
    H = (L - 1) // 2
    NF = num_frames(S, frame_len, frame_step)
    rows = []
    for b in range(B):
        n = S if lengths is None else int(lengths[b])
        x = F.pad(wave[b, :n], (H, H))                                         # x~ on [-H, n + H)
        z = sum(g[:, l:l + 1] * x[l:l + n].view(1, n) for l in range(L))       # [F, n]
        z2 = F.pad(z * z, (0, max(0, (NF - 1) * frame_step + frame_len - n)))
        y = torch.zeros(Fn, NF, dtype=torch.float64)
        cols = [torch.log(z2[:, t * frame_step:t * frame_step + frame_len].sum(dim=1) / frame_len + eps)
                for t in range(num_frames(n, frame_len, frame_step))]
        rows.append(torch.cat([torch.stack(cols, dim=1), y[:, len(cols):]], dim=1))
    return torch.stack(rows)


def features_conv1d(wave, g, frame_len, frame_step, eps=1e-6):
    """The same for a rectangular batch in plain torch: conv1d, square, framing by avg_pool1d-style unfolding, log.  This is also the
    formulation the benchmark times against (it writes, and keeps for its backward, the stride-1 tensor z [B, F, S])."""
    B, S = wave.shape
    L = g.shape[1]
    z = F.conv1d(wave.unsqueeze(1), g.unsqueeze(1), padding=(L - 1) // 2)      # g is even: correlation = convolution
    NF = num_frames(S, frame_len, frame_step)
    z2 = F.pad(z * z, (0, max(0, (NF - 1) * frame_step + frame_len - S)))
    e = z2.unfold(2, frame_len, frame_step).sum(dim=3) / frame_len
    return torch.log(e + eps)


def white_noise(B, S, seed):
    """Unit-variance white noise: every band's energy is far above eps, so the log does not amplify rounding."""
    return torch.randn(B, S, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def encoder(wave, lengths, p, contexts, bn_first, training, sinc):
    """(xv, x_a) of ``arch: sincnet``: the sinc features, then the TDNN with `pooling: statistic` (tests/ftdnn_ref.py's encoder without
    factorized layers).  ``sinc``: dict(L, rate, min_low_hz, min_band_hz, eps, frame_len, frame_step).  A ragged batch is run row by row
    at each row's own frame count, as the reference's test loop does."""
    import ftdnn_ref
    g = taps(p["sinc.low_hz_"], p["sinc.band_hz_"], sinc["L"], sinc["rate"], sinc["min_low_hz"], sinc["min_band_hz"])
    y = features(wave, lengths, g, sinc["frame_len"], sinc["frame_step"], sinc["eps"])
    if lengths is None:
        return ftdnn_ref.encoder(y, p, contexts, set(), 0.0, bn_first, training)
    outs = [ftdnn_ref.encoder(y[b:b + 1, :, :num_frames(int(n), sinc["frame_len"], sinc["frame_step"])], p, contexts, set(), 0.0, bn_first,
                              training) for b, n in enumerate(lengths)]
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
