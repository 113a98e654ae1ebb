"""The definition of `pooling: multi_head_attention` restated in plain torch, differentiable by autograd, for the tests
of deeplip_amd.audio.MultiHeadAttention (test_mh_attn_pool_cpu.py, test_mh_attn_pool_gpu.py).  Run it on fp64 tensors."""
import torch

EPS = 1e-5          # deeplip_amd.audio_resnet.POOL_EPS


def single_head(x, W, b, v, k, eps=EPS):
    """One attentive statistics pooling with the floored standard deviation: x [B,T,C], W [Hd,C], b [1,Hd], v [Hd,1], k [1,1] -> [B,2C]."""
    e = torch.relu(x.matmul(W.t()) + b).matmul(v) + k               # [B,T,1]
    alpha = torch.softmax(e, dim=1)
    m = (alpha * x).sum(dim=1)
    q = (alpha * x * x).sum(dim=1)
    return torch.cat([m, torch.sqrt(torch.clamp(q - m * m, min=0.0) + eps)], dim=1)


def multi_head(x, W, b, v, k, widths, lengths=None, eps=EPS):
    """x [B,T,C]; W [S,C], b [1,S], v [S,1], k [1,n] stacked over the heads of ``widths`` -> y [B, n 2C] = cat_h [m_h | s_h], written
    out as the issue states it: ONE hidden product for all heads, per-head segmented scores, softmax over each row's valid frames."""
    B, T, _ = x.shape
    hidden = x.matmul(W.t()) + b                                    # [B,T,S]
    rows = []
    for i in range(B):
        L = T if lengths is None else int(lengths[i])
        xi, off, parts = x[i, :L], 0, []
        for h, w in enumerate(widths):
            e = torch.relu(hidden[i, :L, off:off + w]).matmul(v[off:off + w, 0]) + k[0, h]     # [L]
            alpha = torch.softmax(e, dim=0)[:, None]
            m = (alpha * xi).sum(dim=0)
            q = (alpha * xi * xi).sum(dim=0)
            parts += [m, torch.sqrt(torch.clamp(q - m * m, min=0.0) + eps)]
            off += w
        rows.append(torch.cat(parts))
    return torch.stack(rows)


def case_tensors(B, T, C, widths, seed=5):
    """The inputs of the existing attentive pooling test, stacked over heads: x = 0.8 randn + 0.3 [B,T,C], W ~ randn / sqrt(C), b and k ~
    0.1 randn, v ~ 0.5 randn, dy ~ randn (all fp32, CPU)."""
    g = torch.Generator().manual_seed(seed)
    S, n = sum(widths), len(widths)
    return {"W": torch.randn(S, C, generator=g) / C ** 0.5, "b": torch.randn(1, S, generator=g) * 0.1,
            "v": torch.randn(S, 1, generator=g) * 0.5, "k": torch.randn(1, n, generator=g) * 0.1,
            "x": torch.randn(B, T, C, generator=g) * 0.8 + 0.3, "dy": torch.randn(B, n * 2 * C, generator=g)}
