"""The yardstick of ``arch: ftdnn`` (conf/audio_config.yaml:84-92): an fp64 numpy / torch restatement of the definition --
the factorized block, the encoder built from it, and the semi-orthogonal step.  It imports nothing from the code under test.

Layouts are the reference's: activations [B, C, T], Conv1d weights [K, C, taps], state-dict keys as the model's."""
import numpy as np
import torch
import torch.nn.functional as F

LRELU = 0.2
BN_EPS = 1e-5


# ---- the semi-orthogonal step --------------------------------------------------------------------------------------------------
def semi_orth_quantities(M):
    """(P, tp, tpp, alpha2, ratio, nu) of a matrix M [rows, cols] in fp64."""
    M = np.asarray(M, dtype=np.float64)
    P = M @ M.T
    tp = float(np.trace(P))
    tpp = float((P * P).sum())
    alpha2 = tpp / tp
    ratio = tpp * M.shape[0] / (tp * tp)
    nu = 0.125
    if ratio > 1.02:
        nu *= 0.5
    if ratio > 1.1:
        nu *= 0.5
    return P, tp, tpp, alpha2, ratio, nu


def semi_orth_step(M):
    """M <- M - (4 nu / alpha2) (P - alpha2 I) M   (Kaldi's ConstrainOrthonormalInternal with a floating scale)."""
    M = np.asarray(M, dtype=np.float64)
    P, tp, tpp, alpha2, ratio, nu = semi_orth_quantities(M)
    return M - (4.0 * nu / alpha2) * ((P - alpha2 * np.eye(M.shape[0])) @ M)


def semi_orth_defect(M):
    """||P / alpha2 - I||_F: zero when the rows of M are orthogonal and of one length."""
    P, tp, tpp, alpha2, ratio, nu = semi_orth_quantities(M)
    return float(np.linalg.norm(P / alpha2 - np.eye(P.shape[0])))


def semi_orth_due(n, every):
    """Is the step due on optimizer step n (counted from 1)?"""
    return every > 0 and n % every == 0


def uniform_matrix(rows, cols, seed):
    """rows x cols drawn uniform(+-1 / sqrt(cols)) (nn.Conv1d's default init of a factor weight)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(-1.0, 1.0, (rows, cols)) / np.sqrt(cols)


def converged_matrix(rows, cols, seed, steps=40):
    M = uniform_matrix(rows, cols, seed)
    for _ in range(steps):
        M = semi_orth_step(M)
    return M


# ---- the block and the encoder -------------------------------------------------------------------------------------------------
def dilation_of(context):
    return (context[-1] - context[0]) // (len(context) - 1) if len(context) > 1 else 1


def _bn(y, p, prefix, training):
    return F.batch_norm(y, p[prefix + "running_mean"].clone(), p[prefix + "running_var"].clone(), p[prefix + "weight"], p[prefix + "bias"],
                        training, 0.1, BN_EPS)


def _bn_act(y, p, prefix, bn_first, training):
    if bn_first:
        return F.leaky_relu(_bn(y, p, prefix, training), LRELU)
    return _bn(F.leaky_relu(y, LRELU), p, prefix, training)


def tdnn_block(x, p, prefix, context, bn_first, training):
    y = F.conv1d(x, p[prefix + "context_layer.weight"], p[prefix + "context_layer.bias"], dilation=dilation_of(context))
    return _bn_act(y, p, prefix + "bn.", bn_first, training)


def ftdnn_block(x, p, prefix, context, bypass_scale, bn_first, training):
    """x [B, Cin, T] fp64 -> [B, Cout, T'].  p: {prefix + 'factor.weight', 'context_layer.weight' / '.bias', 'bn.*'} fp64 tensors."""
    z = F.conv1d(x, p[prefix + "factor.weight"], None, dilation=dilation_of(context))
    y = F.conv1d(z, p[prefix + "context_layer.weight"], p[prefix + "context_layer.bias"])
    y = _bn_act(y, p, prefix + "bn.", bn_first, training)
    if x.shape[1] == y.shape[1] and bypass_scale != 0.0:
        assert context[0] <= 0 <= context[-1]
        y = y + bypass_scale * x[:, :, -context[0]: -context[0] + y.shape[2]]
    return y


def encoder(x, p, contexts, factorized, bypass_scale, bn_first, training):
    """(xv, x_a) of the TDNN-family encoder with `pooling: statistic` (tdnn.py:89-101): x [B, F, T] fp64."""
    h = x
    for i, c in enumerate(contexts):
        if i in factorized:
            h = ftdnn_block(h, p, f"tdnn.{i}.", c, bypass_scale, bn_first, training)
        else:
            h = tdnn_block(h, p, f"tdnn.{i}.", c, bn_first, training)
    pooled = torch.cat([h.mean(dim=2), h.std(dim=2, unbiased=True)], dim=1)
    x_a = F.linear(pooled, p["fc1.weight"], p["fc1.bias"])
    xv = F.linear(_bn_act(x_a, p, "bn1.", bn_first, training), p["fc2.weight"], p["fc2.bias"])
    return xv, x_a


def to64(sd, grad=False):
    """A state dict as detached fp64 CPU tensors (floating parameters optionally requiring grad)."""
    out = {}
    for k, v in sd.items():
        t = v.detach().cpu()
        if t.is_floating_point():
            t = t.double().clone()
            if grad and not k.endswith(("running_mean", "running_var")):
                t.requires_grad_()
        out[k] = t
    return out
