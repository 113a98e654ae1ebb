"""Train-mode BatchNorm backward on ILL-CONDITIONED channels (-m gpu).  Every other BatchNorm test draws its channels from one
distribution; real training also produces an exactly constant channel (a dead filter: bias only), a channel whose variance sits below
eps, channel scales over six decades, gradient channels that are zero or tiny, gamma of zero or below zero, a large offset and an
outlier row.  One seeded generator builds all of them -- the degenerate channels inside the same 64-channel block as live ones -- and
the BatchNorm backward paths are held to fp64 torch autograd ELEMENT by element (conftest.assert_close_rel), dgamma / dbeta / dslope
per channel against the size of their own fp64 sums, and the lift of the dz that the speech encoder never stores (ABI 47, formed on
load by the convolution's operand producers) to within 2^-10 of its target."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_close_rel, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-5


@pytest.fixture(autouse=True)
def _collect_cycles():
    """Collect what a test leaves in reference cycles (autograd graphs, retained gradients) while nothing is being recorded: a GPU
    tensor freed by a collection that happens to run inside a later test's graph capture aborts that capture."""
    yield
    gc.collect()


# the degenerate channels, all inside the first 64-channel block
C_CONST, C_GAMMA0, C_EPS, C_DY0, C_OFF, C_OUT = 5, 11, 17, 23, 29, 41


def gen(seed):
    return np.random.default_rng(seed)


def channel_params(C, seed, zero_gamma=True):
    """gamma over 1e-3 .. 1e2 with random signs (one exact zero), a beta that is never zero (the constant and gamma = 0 channels' output
    is beta), dy channel scales over 1e-6 .. 1 (one channel all zero)."""
    r = gen(seed)
    gamma = 10.0 ** r.uniform(-3, 2, C) * np.where(r.random(C) < 0.3, -1.0, 1.0)
    if zero_gamma:
        gamma[C_GAMMA0] = 0.0
    beta = (0.3 * r.standard_normal(C) + 0.5 * np.sign(r.standard_normal(C))) * np.maximum(np.abs(gamma), 0.05)
    gamma[C_OFF] = abs(gamma[C_OFF])
    beta[C_OFF] = 6.0 * gamma[C_OFF]              # (bn > 0 on the whole offset channel: nothing there is moved off a kink)
    dscale = 10.0 ** r.uniform(-6, 0, C)
    dscale[C_DY0] = 0.0
    return gamma.astype(np.float32), beta.astype(np.float32), dscale


def conditioned_rows(M, C, seed, outlier=False, near_eps=True):
    """z [M, C] fp32: channel std over 1e-3 .. 1e3; C_CONST exactly constant; C_EPS variance ~ eps / 10; C_OFF |mean| / std = 1e4 (rows
    in +-d pairs around a centre that fp32 holds exactly, so the batch mean is exact in both arithmetics); C_OUT (outlier) one row at
    |xhat| ~ sqrt(M) / 2."""
    assert M % 2 == 0
    r = gen(seed)
    std = 10.0 ** r.uniform(-3, 3, C)
    z = r.standard_normal((M, C)) * std + r.standard_normal(C) * std
    z[:, C_CONST] = 0.37
    if near_eps:
        z[:, C_EPS] = 0.01 + np.sqrt(EPS / 10) * r.standard_normal(M)
    sd, centre = 0.5, 5000.0                      # ulp(5000) = 2^-11: the pairs' offsets on that grid
    d = np.round(sd * r.standard_normal(M // 2) * 2048.0) / 2048.0
    z[0::2, C_OFF], z[1::2, C_OFF] = centre + d, centre - d
    if outlier:
        s = std[C_OUT]
        z[:, C_OUT] = s * r.standard_normal(M)
        z[M // 3, C_OUT] = s * np.sqrt(M / 3.0)
    return z.astype(np.float32)


def clear_kinks(z, gamma, beta, act_first, keep=(C_CONST, C_OFF)):
    """Move every value whose fp64 pre-activation lies within 1e-5 of its channel's scale from zero out to 2e-5 of it (the LeakyReLU /
    PReLU kink must not decide a result: flipped kinks are a separate, known effect).  The constant and offset channels are left as
    they are (their pre-activation is beta / positive by construction)."""
    z = z.astype(np.float64)
    for _ in range(4):
        if act_first:
            pre, scale, step = z, np.abs(z).max(0) + 1e-30, np.ones(z.shape[1])
        else:
            mu, var = z.mean(0), z.var(0)
            inv = 1.0 / np.sqrt(var + EPS)
            xh = (z - mu) * inv
            pre = xh * gamma + beta
            scale = np.abs(gamma) * np.abs(xh).max(0) + np.abs(beta)
            step = np.sign(gamma) / np.maximum(np.abs(gamma) * inv, 1e-30)          # (the move in z that raises pre by one)
        near = np.abs(pre) < 1e-5 * scale
        near[:, list(keep)] = False
        if not near.any():
            return z.astype(np.float32)
        sgn = np.where(pre >= 0, 1.0, -1.0)
        z = np.where(near, z + sgn * (2e-5 * scale - np.abs(pre)) * step, z)
        z = z.astype(np.float32).astype(np.float64)
    raise AssertionError("values left at a kink")


def bn_act_ref(z, gamma, beta, dy, act, slope, act_first=False, res=None):
    """fp64 torch autograd of act(bn_train(z) [+ res]) (or bn_train(act(z))): outputs, gradients, the gradient g at the BatchNorm's output,
    xhat, and the running statistics after one update from (0, 1)."""
    zd = torch.from_numpy(np.asarray(z, np.float64)).requires_grad_()
    gd = torch.from_numpy(np.asarray(gamma, np.float64)).requires_grad_()
    bd = torch.from_numpy(np.asarray(beta, np.float64)).requires_grad_()
    sd = torch.as_tensor(np.asarray(slope, np.float64)).requires_grad_()
    rd = torch.from_numpy(np.asarray(res, np.float64)).requires_grad_() if res is not None else None
    C = zd.shape[-1]
    z2 = zd.reshape(-1, C)
    a = F.leaky_relu(z2, float(slope)) if act_first else z2
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    bn = F.batch_norm(a, rm, rv, gd, bd, training=True, momentum=0.1, eps=EPS)
    bn.retain_grad()
    t = bn if rd is None else bn + rd.reshape(-1, C)
    if act_first:
        y = t
    elif act == "prelu":
        y = F.prelu(t, sd)
    else:
        y = F.leaky_relu(t, float(slope))
    y = y.reshape(zd.shape)
    y.backward(torch.from_numpy(np.asarray(dy, np.float64)))
    ad = a.detach()
    xh = (ad - ad.mean(0)) / torch.sqrt(ad.var(0, unbiased=False) + EPS)
    out = {"y": y.detach().numpy(), "dz": zd.grad.numpy(), "dgamma": gd.grad.numpy(), "dbeta": bd.grad.numpy(), "g": bn.grad.numpy(),
           "xhat": xh.numpy(), "rm": rm.numpy(), "rv": rv.numpy(), "pre": t.detach().numpy()}
    if act == "prelu":
        out["dslope"] = sd.grad.numpy()
    if rd is not None:
        out["dres"] = rd.grad.numpy()
    return out


def assert_channel_sums(got, want, mag, rtol, what):
    """Per channel: |a - b| <= rtol |b| + 1e-6 mag, mag = the channel's sum of |terms| (the sums are fp64 in the kernels)."""
    got, want, mag = (np.asarray(t, np.float64) for t in (got, want, mag))
    bad = np.abs(got - want) > rtol * np.abs(want) + 1e-6 * mag
    if bad.any():
        c = int(np.argmax(np.abs(got - want) - rtol * np.abs(want) - 1e-6 * mag))
        raise AssertionError(f"{what}: {int(bad.sum())} channels off; worst {c}: got {got[c]!r}, want {want[c]!r}, sum|terms| {mag[c]!r}")


def assert_bn_grads(got_dg, got_db, ref, rtol=1e-4):
    g, xh = ref["g"].reshape(-1, ref["g"].shape[-1]), ref["xhat"]
    assert_channel_sums(got_dg, ref["dgamma"], np.abs(g * xh).sum(0), rtol, "dgamma")
    assert_channel_sums(got_db, ref["dbeta"], np.abs(g).sum(0), rtol, "dbeta")


def assert_running(rm, rv, ref):
    assert_close_rel(rm, ref["rm"], 1e-5, 1e-7, "running_mean")
    assert_close_rel(rv, ref["rv"], 1e-5, 1e-7, "running_var")


def assert_lift(dx, lift):
    lift = lift.cpu()
    e, inv, amax = float(lift[0]), float(lift[1]), float(dx.abs().max())
    assert e * inv == 1.0 and 512.0 <= amax * e <= 1024.0 and bool((lift[2:2050] == inv).all()), (e, inv, amax)


def cuda(*ts):
    return [torch.as_tensor(np.ascontiguousarray(t), dtype=torch.float32).to(DEV) for t in ts]


# ------------------------------------------------------------------------------------------------------------------------------
# the lift of the dz that is formed on load: dlip_bn_rows_train_bwd_sums_f32 against the true max|dz| (fp64, from the same fp32 inputs)

def true_dz(z, dy, gamma, beta, mean, invstd, slope, act_first):
    z, dy = z.astype(np.float64), dy.astype(np.float64)
    gamma, beta, mean, invstd = (np.asarray(t, np.float64) for t in (gamma, beta, mean, invstd))
    M = z.shape[0]
    a = np.where(z >= 0, z, slope * z) if act_first else z
    xh = (a - mean) * invstd
    g = dy if act_first else dy * np.where(xh * gamma + beta >= 0, 1.0, slope)
    dz = gamma * invstd * (g - g.sum(0) / M - xh * (g * xh).sum(0) / M)
    return dz * np.where(z >= 0, 1.0, slope) if act_first else dz


def concrete_rows(M, C, seed):
    """The ADVICE case: live channels with z std ~ 100 and dy ~ 1e-4, one dead filter (constant: invstd ~ 316) whose dy ~ 1e-10."""
    r = gen(seed)
    z = (100.0 * r.standard_normal((M, C))).astype(np.float32)
    z[:, C_CONST] = 0.37
    gamma = (1.0 + 0.2 * r.standard_normal(C)).astype(np.float32)
    beta = (0.2 * r.standard_normal(C)).astype(np.float32)
    dscale = np.full(C, 1e-4)
    dscale[C_CONST] = 1e-10
    return z, gamma, beta, dscale


@pytest.mark.parametrize("M,C,act_first,outlier,src", [(5120, 128, False, None, "dy"), (5120, 128, True, None, "dy"), (5100, 64, False, None, "ms"),
                                                       (5120, 128, False, False, "dy"), (5120, 128, True, False, "dy"),
                                                       (6000, 64, False, True, "dy"), (6000, 192, True, True, "dy"),
                                                       (5100, 128, False, False, "ms"), (6000, 100, False, True, "ms")])
def test_lift_of_the_gradient_formed_on_load_sits_at_its_target(M, C, act_first, outlier, src):
    """The power-of-two lift the sums pass sets for a dz it never sees: 1 <= max|dz| lift <= 1024 (the upper end is the overflow side a
    bound must keep, the lower end 2^-10 of the target) -- with dy given and with dy formed on load from a statistics pooling's
    coefficients (ms = (coef, T), computed as MeanStdPoolFn's hand-over backward computes them); and the word layout.  outlier None:
    the concrete case of concrete_rows."""
    from deeplip_amd import autograd as ag
    slope = 0.2
    if outlier is None:
        z, gamma, beta, dscale = concrete_rows(M, C, seed=100 + C)
    else:
        z = conditioned_rows(M, C, seed=101 + C, outlier=outlier)
        gamma, beta, dscale = channel_params(C, seed=102 + C)
    z = clear_kinks(z, gamma, beta, act_first)
    zg, gg, bg = cuda(z, gamma, beta)
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    _, mean, invstd = ag._bn_rows_fwd(zg, gg, bg, rm, rv, 0.1, EPS, slope, act_first, stats_only=True)
    if src == "dy":
        dy = (gen(103 + C).standard_normal((M, C)) * dscale).astype(np.float32)
        dg, db, lift = ag._bn_rows_bwd_sums(cuda(dy)[0], zg, gg, bg, mean, invstd, slope, act_first)
    else:
        T = 100 if M % 100 == 0 else 60
        B = M // T
        # the activated values and their pooled statistics, then the pooling's gradient over decades per channel (one channel zero)
        ya = F.leaky_relu((zg - mean) * invstd * gg + bg, slope).view(B, T, C)
        y_pool = torch.cat([ya.mean(1), ya.std(1)], 1).contiguous()
        gp = gen(104 + C).standard_normal((B, 2 * C)) * np.concatenate([dscale, dscale[::-1]])
        coef = torch.empty_like(y_pool)
        ag.check(ag.lib().dlip_meanstd_bwd_coef_f32(ag.ptr(y_pool), ag.ptr(cuda(gp)[0]), ag.ptr(coef), B, C, T, ag.stream_handle()),
                 "dlip_meanstd_bwd_coef_f32")
        dg, db, lift = ag._bn_rows_bwd_sums(None, zg, gg, bg, mean, invstd, slope, act_first, ms=(coef, T))
        co = coef.double().cpu().numpy()
        yv = ya.double().cpu().numpy()
        dy = (co[:, None, :C] + co[:, None, C:] * yv).reshape(M, C)
    torch.cuda.synchronize()
    lift = lift.cpu()
    assert float(lift[0]) * float(lift[1]) == 1.0 and bool((lift[2:2050] == lift[1]).all())
    dz = true_dz(z, dy, gamma, beta, mean.cpu().numpy(), invstd.cpu().numpy(), slope, act_first)
    amax = float(np.abs(dz).max())
    assert amax > 0.0
    at = amax * float(lift[0])
    assert 1.0 <= at <= 1024.0, f"max|dz| lift = {at:.6g} (max|dz| {amax:.3e}, lift 2^{np.log2(float(lift[0])):.0f})"


# ------------------------------------------------------------------------------------------------------------------------------
# the speech encoder's block: conv -> BatchNorm -> LeakyReLU with dz formed on load, against fp64 autograd and against the stored route

def tdnn_case(B, T, C, K, S, dil, profile, seed):
    r = gen(seed)
    x = r.standard_normal((B, C, T)).astype(np.float32)
    w = r.standard_normal((K, C, S)) / np.sqrt(C * S)
    if profile == "concrete":                  # the ADVICE case: live channels z std ~ 100, dy ~ 1e-4; one dead filter with dy ~ 1e-10
        zs = np.full(K, 100.0)
        gamma = (1.0 + 0.2 * r.standard_normal(K)).astype(np.float32)
        beta = (0.2 * r.standard_normal(K)).astype(np.float32)
        dscale = np.full(K, 1e-4)
        dscale[C_CONST] = 1e-10
    else:
        zs = 10.0 ** r.uniform(-3, 3, K)
        zs[C_EPS] = np.sqrt(EPS / 10)
        gamma, beta, _ = channel_params(K, seed + 1)
        # dy per channel ~ 1e-4 z std / |gamma| (within a decade): dz -- what the data and weight gradients' operands hold under ONE
        # lift -- then spans about two decades over the channels; per-channel lifts (dz channels 1e-6 below the largest held to their own
        # scale) are a separate matter.  One gradient channel all zero, the dead filter's ~1e-10.
        dscale = 1e-4 * zs / np.maximum(np.abs(gamma), 1e-3) * 10.0 ** r.uniform(-1, 1, K)
        dscale[C_DY0] = 0.0
        dscale[C_CONST] = 1e-10
    w = w * zs[:, None, None]
    w[C_CONST] = 0.0                            # a dead filter: the channel is its bias, exactly
    b = (0.1 * zs * r.standard_normal(K)).astype(np.float32)
    b[C_CONST] = 0.37
    dy = r.standard_normal((B, K, T - dil * (S - 1))) * dscale[None, :, None]
    return x, w.astype(np.float32), b, gamma, beta, dy.astype(np.float32)


def run_tdnn(x, w, b, gamma, beta, dy, slope, dil, act_first):
    from deeplip_amd import autograd as ag
    K = w.shape[0]
    xg = torch.from_numpy(x).permute(0, 2, 1).contiguous().to(DEV).requires_grad_()
    wg_, bg, gg, beg = (t.requires_grad_() for t in cuda(w, b, gamma, beta))
    rm, rv = torch.zeros(K, device=DEV), torch.ones(K, device=DEV)
    y = ag.TDNNBlockTrainFn.apply(xg, wg_, bg, gg, beg, rm, rv, 0.1, EPS, slope, dil, act_first)
    y.backward(torch.from_numpy(dy).permute(0, 2, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    return {"dx": xg.grad.cpu().permute(0, 2, 1).numpy(), "dw": wg_.grad.cpu().numpy(), "db": bg.grad.cpu().numpy(),
            "dgamma": gg.grad.cpu().numpy(), "dbeta": beg.grad.cpu().numpy(), "rm": rm.cpu().numpy(), "rv": rv.cpu().numpy(),
            "y": y.detach().cpu().permute(0, 2, 1).numpy()}


@pytest.mark.parametrize("B,T,C,K,S,dil,act_first,profile", [
    (40, 120, 64, 128, 1, 1, False, "concrete"),
    (40, 120, 64, 128, 1, 1, False, "spread"), (40, 120, 64, 128, 1, 1, True, "spread"),
    (40, 120, 64, 100, 1, 1, False, "spread"), (20, 250, 128, 1500, 1, 1, False, "spread"),
    (40, 120, 64, 128, 3, 2, False, "spread"), (40, 120, 64, 128, 3, 2, True, "spread"), (40, 120, 64, 128, 3, 2, False, "concrete")])
def test_tdnn_block_backward_on_ill_conditioned_channels(B, T, C, K, S, dil, act_first, profile, monkeypatch):
    """TDNNBlockTrainFn at more than BN_SMALL_ROWS rows, dz formed on load (k = 1: dlip_wgrad_operand_split_bnbwd_f32, also K = 100 and
    1 500; k = 3 dilated: the chwn route) and stored (BN_BWD_ON_LOAD off).  Slope 1.0: no kink decides anything.  Against fp64 autograd
    element by element (dx, dW, dbias: 1e-4 + 1e-6 max; dgamma / dbeta per channel against their own sums), and the two routes against
    each other (the same forward bits: a lift's exponent moves the last bit of a split at most)."""
    from deeplip_amd import autograd as ag
    x, w, b, gamma, beta, dy = tdnn_case(B, T, C, K, S, dil, profile, seed=200 + K + S + int(act_first))
    assert B * (T - dil * (S - 1)) > ag.BN_SMALL_ROWS
    xd, wd, bd, gd, betad = (torch.from_numpy(t.astype(np.float64)).requires_grad_() for t in (x, w, b, gamma, beta))
    z = F.conv1d(xd, wd, bd, dilation=dil)
    bn = F.batch_norm(z, None, None, gd, betad, training=True, eps=EPS)
    bn.retain_grad()
    bn.backward(torch.from_numpy(dy.astype(np.float64)))
    zz = z.detach().permute(0, 2, 1).reshape(-1, K)
    xh = ((zz - zz.mean(0)) / torch.sqrt(zz.var(0, unbiased=False) + EPS)).numpy()
    g = bn.grad.permute(0, 2, 1).reshape(-1, K).numpy()
    out = {}
    for on in (True, False):
        monkeypatch.setattr(ag, "BN_BWD_ON_LOAD", on)
        out[on] = run_tdnn(x, w, b, gamma, beta, dy, 1.0, dil, act_first)
    # dbias: sum over rows of dz, which the batch statistics make ~0 -- per channel against sum |dz|
    zr = z.detach().requires_grad_()
    torch.autograd.backward(F.batch_norm(zr, None, None, gd.detach(), betad.detach(), training=True, eps=EPS), torch.from_numpy(dy.astype(np.float64)))
    dz_abs = zr.grad.abs().sum((0, 2)).numpy()
    for on, got in out.items():
        tag = f"[on-load {on}]"
        assert_close_rel(got["dx"], xd.grad.numpy(), 1e-4, 1e-6, f"{tag} dx")
        assert_close_rel(got["dw"], wd.grad.numpy(), 1e-4, 1e-6, f"{tag} dW")
        assert_channel_sums(got["db"], bd.grad.numpy(), dz_abs, 1e-4, f"{tag} dbias")
        assert_channel_sums(got["dgamma"], gd.grad.numpy(), np.abs(g * xh).sum(0), 1e-4, f"{tag} dgamma")
        assert_channel_sums(got["dbeta"], betad.grad.numpy(), np.abs(g).sum(0), 1e-4, f"{tag} dbeta")
    assert np.array_equal(out[True]["y"], out[False]["y"])
    for k in ("dx", "dw", "dgamma", "dbeta", "db"):
        assert_close_rel(out[True][k], out[False][k], 1e-5, 1e-7, f"on-load vs stored {k}")
    for k in ("rm", "rv"):
        assert np.array_equal(out[True][k], out[False][k]), k
    from deeplip_amd import _lib
    _lib.check_range(sync=True)


@pytest.mark.parametrize("act_first", [False, True])
def test_tdnn_block_routes_agree_with_a_kinked_slope(act_first, monkeypatch):
    """The same conditioned block at slope 0.2: the routes' forward bits are identical, so their comparison does not depend on which
    side of a kink a value falls."""
    from deeplip_amd import autograd as ag
    x, w, b, gamma, beta, dy = tdnn_case(40, 120, 64, 128, 1, 1, "spread", seed=333 + int(act_first))
    out = {}
    for on in (True, False):
        monkeypatch.setattr(ag, "BN_BWD_ON_LOAD", on)
        out[on] = run_tdnn(x, w, b, gamma, beta, dy, 0.2, 1, act_first)
    assert np.array_equal(out[True]["y"], out[False]["y"])
    for k in ("dx", "dw", "dgamma", "dbeta", "db"):
        assert_close_rel(out[True][k], out[False][k], 1e-5, 1e-7, f"on-load vs stored {k}")


def test_speech_encoder_on_ill_conditioned_channels_routes_agree(monkeypatch):
    """The whole small speech encoder (SpeakerEmbNet, statistics pooling, B = 64: more than 4 096 rows per block) with one dead hidden
    filter, the last block's weight rows scaled over six decades and unnormalised input (per-band gains 1e-2 .. 1e2): BN_BWD_ON_LOAD and
    POOL_BWD_ON_LOAD each on and off give the same loss and running statistics.  BN_BWD_ON_LOAD moves nothing but the exponent of the lift
    of dz (the same expression per value): every parameter gradient element-wise to 1e-5 + 1e-6 max.  POOL_BWD_ON_LOAD forms the pooling's
    gradient as A + K y instead of the pooling backward's own expression (other roundings, carried through four blocks' backward into
    elements far below their tensor's largest): 1e-6 of each tensor's largest, as test_meanstd_pooling_with_the_batchnorm_in_front_applied_on_load."""
    from deeplip_amd import autograd as ag, weightgen as wg
    from models.audio_models.loss import LMCL
    from models.audio_models.tdnn import SpeakerEmbNet
    from oracle import deeplip_oracle as O
    B = 64
    opts = {"arch": "tdnn", "tdnn": {"input_dim": 24, "hidden_dim": [512] * 4 + [1500], "context": O.TDNN_CONTEXT, "tdnn_layers": 5,
                                      "embedding_dim": 512, "pooling": "statistic", "attention_hidden_size": 64, "bn_first": True}}
    x = wg.audio_input(B, 24, 90, key="bn.conditioning")
    ax = [i for i, n in enumerate(x.shape) if n == 24][0]
    gains = 10.0 ** np.linspace(-2, 2, 24)
    x = torch.from_numpy((x * gains.reshape([-1 if i == ax else 1 for i in range(x.ndim)])).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(wg.labels(B, 19)).to(DEV)
    net0 = SpeakerEmbNet(opts)
    sd = wg.fill_state_dict({k: tuple(v.shape) for k, v in net0.state_dict().items()}, prefix="audio_tdnn.")
    sd["tdnn.2.context_layer.weight"][7] = 0.0                                   # a dead hidden filter
    w4 = sd["tdnn.4.context_layer.weight"]
    w4 *= (10.0 ** np.random.default_rng(5).uniform(-3, 3, w4.shape[0])).reshape(-1, 1, 1).astype(w4.dtype)
    cw = wg.fill_state_dict({"w": tuple(LMCL(512, 19, 30, 0.2).weights.shape)}, prefix="bn.conditioning.crit.")["w"]
    res = {}
    for bwd_on in (True, False):
        for pool_on in (True, False):
            monkeypatch.setattr(ag, "BN_BWD_ON_LOAD", bwd_on)
            monkeypatch.setattr(ag, "POOL_BWD_ON_LOAD", pool_on)
            net = SpeakerEmbNet(opts)
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
            net.to(DEV).train()
            crit = LMCL(512, 19, 30, 0.2).to(DEV)
            with torch.no_grad():
                crit.weights.copy_(torch.from_numpy(cw))
            loss, _ = crit(net(x), lab)
            loss.backward()
            torch.cuda.synchronize()
            res[(bwd_on, pool_on)] = (float(loss.detach()), {k: v.grad.detach().cpu().numpy() for k, v in net.named_parameters()},
                                      {k: v.detach().cpu().numpy() for k, v in net.named_buffers()})
    ref = res[(False, False)]
    for key, got in res.items():
        assert got[0] == ref[0], key
        for k in ref[2]:
            assert np.array_equal(got[2][k], ref[2][k]), (key, k)
        for k in ref[1]:
            assert rel_err(got[1][k], ref[1][k]) < 1e-6, (key, k)
    bad = []
    for pool_on in (True, False):
        on, off = res[(True, pool_on)], res[(False, pool_on)]
        for k in off[1]:
            try:
                assert_close_rel(on[1][k], off[1][k], 1e-5, 1e-6, f"pool on-load {pool_on}: {k}")
            except AssertionError as e:
                bad.append(str(e))
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------------------------------------
# the lip-clip encoder's BatchNorm Functions (dx stored, its lift from the exact max): regression guards on the same channels

def lip_case(M, C, seed, outlier, act_first=False, near_eps=True):
    z = conditioned_rows(M, C, seed, outlier=outlier, near_eps=near_eps)
    gamma, beta, dscale = channel_params(C, seed + 1)
    z = clear_kinks(z, gamma, beta, act_first)
    dy = (gen(seed + 2).standard_normal((M, C)) * dscale).astype(np.float32)
    return z, gamma, beta, dy


def check_bn_fn(got, ref, what):
    assert_close_rel(got["y"], ref["y"], 1e-5, 1e-6, f"{what} y")
    assert_close_rel(got["dx"], ref["dz"], 1e-4, 1e-6, f"{what} dx")
    assert_bn_grads(got["dgamma"], got["dbeta"], ref)
    assert_running(got["rm"], got["rv"], ref)


@pytest.mark.parametrize("M,C,outlier", [(5000, 64, False), (5000, 128, True), (1200, 64, False)])
def test_bn_prelu_on_ill_conditioned_channels(M, C, outlier):
    from deeplip_amd import autograd_video as av
    z, gamma, beta, dy = lip_case(M, C, 400 + M + C, outlier)
    slope = (gen(7).random(C) * 0.5 - 0.05).astype(np.float32)
    ref = bn_act_ref(z, gamma, beta, dy, "prelu", slope)
    zg, gg, bg, sg = (t.requires_grad_() for t in cuda(z, gamma, beta, slope))
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = av.BNPReLUFn.apply(zg, gg, bg, sg, rm, rv, 0.1, EPS)
    y.backward(cuda(dy)[0])
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu().numpy(), "dx": zg.grad.cpu().numpy(), "dgamma": gg.grad.cpu().numpy(), "dbeta": bg.grad.cpu().numpy(),
           "rm": rm.cpu().numpy(), "rv": rv.cpu().numpy()}
    check_bn_fn(got, ref, "BNPReLUFn")
    assert_channel_sums(sg.grad.cpu().numpy(), ref["dslope"], np.abs(dy * np.minimum(ref["pre"], 0)).sum(0), 1e-5, "dslope")
    # the lift the backward leaves on dx: the exact max puts it at 512 .. 1024
    zg2, gg2, bg2, sg2 = cuda(z, gamma, beta, slope)
    zg2.requires_grad_()
    y2 = av.BNPReLUFn.apply(zg2, gg2, bg2, sg2, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), 0.1, EPS)
    dx = av.BNPReLUFn.backward(y2.grad_fn, cuda(dy)[0])[0]
    torch.cuda.synchronize()
    assert_lift(dx, dx._dlip_lift)


@pytest.mark.parametrize("act_first", [False, True])
@pytest.mark.parametrize("M,C,outlier", [(5000, 64, False), (6000, 128, True), (2000, 64, False)])
def test_bn_rows_act_on_ill_conditioned_channels(M, C, outlier, act_first):
    from deeplip_amd import autograd as ag
    z, gamma, beta, dy = lip_case(M, C, 500 + M + C, outlier, act_first)
    ref = bn_act_ref(z, gamma, beta, dy, "lrelu", 0.2, act_first=act_first)
    zg, gg, bg = (t.requires_grad_() for t in cuda(z, gamma, beta))
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = ag.BNRowsActFn.apply(zg, gg, bg, rm, rv, 0.1, EPS, 0.2, act_first)
    y.backward(cuda(dy)[0])
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu().numpy(), "dx": zg.grad.cpu().numpy(), "dgamma": gg.grad.cpu().numpy(), "dbeta": bg.grad.cpu().numpy(),
           "rm": rm.cpu().numpy(), "rv": rv.cpu().numpy()}
    check_bn_fn(got, ref, f"BNRowsActFn act_first={act_first}")
    _, mean, invstd = ag._bn_rows_fwd(cuda(z)[0], gg.detach(), bg.detach(), torch.zeros(C, device=DEV), torch.ones(C, device=DEV), 0.1, EPS,
                                      0.2, act_first)
    dx, _, _ = ag._bn_rows_bwd(cuda(dy)[0], cuda(z)[0], gg.detach(), bg.detach(), mean, invstd, 0.2, act_first)
    torch.cuda.synchronize()
    assert_lift(dx, dx._dlip_lift)


@pytest.mark.parametrize("M,C,fork", [(5000, 64, False), (5000, 64, True), (6000, 128, True)])
def test_bn_add_prelu_on_ill_conditioned_channels(M, C, fork):
    from deeplip_amd import autograd_video as av
    z, gamma, beta, dy = lip_case(M, C, 600 + M + C, outlier=C == 128)
    r = gen(601)
    res = (r.standard_normal((M, C)) * np.abs(gamma) * 0.1).astype(np.float32)
    slope = (r.random(C) * 0.5 - 0.05).astype(np.float32)
    # the kink of prelu(bn + res): move the residual, not z (the statistics stay as they are)
    ref0 = bn_act_ref(z, gamma, beta, dy, "prelu", slope, res=res)
    pre = ref0["pre"]
    scale = np.abs(pre).max(0) + 1e-30
    near = np.abs(pre) < 1e-5 * scale
    res = np.where(near, res + np.where(pre >= 0, 1.0, -1.0) * 2e-5 * scale, res).astype(np.float32)
    ref = bn_act_ref(z, gamma, beta, dy, "prelu", slope, res=res)
    assert not (np.abs(ref["pre"]) < 0.5e-5 * scale).any()
    d1 = (0.25 * dy).astype(np.float32)
    d2 = (dy - d1).astype(np.float32)
    zg, rg, gg, bg, sg = (t.requires_grad_() for t in cuda(z, res, gamma, beta, slope))
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    if fork:
        y, y2 = av.BNAddPReLUFn.apply(zg, rg, gg, bg, sg, rm, rv, 0.1, EPS, None, True)
        torch.autograd.backward([y, y2], cuda(d1, d2))
        ref = bn_act_ref(z, gamma, beta, d1.astype(np.float64) + d2.astype(np.float64), "prelu", slope, res=res)
    else:
        y = av.BNAddPReLUFn.apply(zg, rg, gg, bg, sg, rm, rv, 0.1, EPS, None, False)
        y.backward(cuda(dy)[0])
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu().numpy(), "dx": zg.grad.cpu().numpy(), "dgamma": gg.grad.cpu().numpy(), "dbeta": bg.grad.cpu().numpy(),
           "rm": rm.cpu().numpy(), "rv": rv.cpu().numpy()}
    check_bn_fn(got, ref, f"BNAddPReLUFn fork={fork}")
    assert_close_rel(rg.grad.cpu().numpy(), ref["dres"], 1e-4, 1e-6, "dres")
    pre = ref["pre"]
    assert_channel_sums(sg.grad.cpu().numpy(), ref["dslope"], np.abs(dy * np.minimum(pre, 0)).sum(0), 1e-5, "dslope")


@pytest.mark.parametrize("N,H,W,C", [(24, 18, 18, 64), (12, 21, 19, 128)])
def test_bn_prelu_maxpool_on_ill_conditioned_channels(N, H, W, C):
    """maxpool(prelu(bn_train(x))) of the stem: the exactly constant channel (and gamma = 0) make every window a tie -- torch gives the
    gradient to the FIRST maximum in row-major order, and so must the kernel's argmax code.  The near-eps channel is left out (its
    argmax is decided by rounding, not by the kernel)."""
    from deeplip_amd import autograd_video as av
    M = N * H * W
    z, gamma, beta, _ = lip_case(M, C, 700 + C, outlier=False, near_eps=False)
    r = gen(701 + C)
    slope = (r.random(C) * 0.5).astype(np.float32)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    _, _, dscale = channel_params(C, 700 + C + 1)
    dy = (r.standard_normal((N, Ho, Wo, C)) * dscale).astype(np.float32)
    zd = torch.from_numpy(z.astype(np.float64)).view(N, H, W, C).permute(0, 3, 1, 2).contiguous().requires_grad_()
    gd, bd = (torch.from_numpy(t.astype(np.float64)).requires_grad_() for t in (gamma, beta))
    sd = torch.from_numpy(slope.astype(np.float64)).requires_grad_()
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    bn = F.batch_norm(zd, rm, rv, gd, bd, training=True, momentum=0.1, eps=EPS)
    bn.retain_grad()
    act = F.prelu(bn, sd)
    act.retain_grad()
    ref_y = F.max_pool2d(act, 3, 2, 1)
    ref_y.backward(torch.from_numpy(dy.astype(np.float64)).permute(0, 3, 1, 2))
    zz = z.astype(np.float64)
    xh = (zz - zz.mean(0)) / np.sqrt(zz.var(0) + EPS)
    g = bn.grad.permute(0, 2, 3, 1).reshape(-1, C).numpy()
    ref = {"y": ref_y.detach().permute(0, 2, 3, 1).numpy(), "dz": zd.grad.permute(0, 2, 3, 1).numpy(), "dgamma": gd.grad.numpy(),
           "dbeta": bd.grad.numpy(), "g": g, "xhat": xh, "rm": rm.numpy(), "rv": rv.numpy()}
    zg, gg, bg, sg = (t.requires_grad_() for t in cuda(z.reshape(N, H, W, C), gamma, beta, slope))
    rmg, rvg = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    y = av.BNPReLUMaxPoolFn.apply(zg, gg, bg, sg, rmg, rvg, 0.1, EPS, None)
    y.backward(cuda(dy)[0])
    torch.cuda.synchronize()
    got = {"y": y.detach().cpu().numpy(), "dx": zg.grad.cpu().numpy(), "dgamma": gg.grad.cpu().numpy(), "dbeta": bg.grad.cpu().numpy(),
           "rm": rmg.cpu().numpy(), "rv": rvg.cpu().numpy()}
    check_bn_fn(got, ref, "BNPReLUMaxPoolFn")
    # (dx of the constant channel is gamma invstd (g - mean g), g the pooled gradient routed to each window's argmax: its element-wise
    # check above holds the kernel's tie rule -- the first maximum in row-major order -- to torch's)
    pre = bn.detach().permute(0, 2, 3, 1).reshape(-1, C).numpy()
    routed = act.grad.permute(0, 2, 3, 1).reshape(-1, C).numpy()
    assert_channel_sums(sg.grad.cpu().numpy(), sd.grad.numpy(), np.abs(routed * np.minimum(pre, 0)).sum(0), 1e-5, "dslope")
    zg2, gg2, bg2, sg2 = cuda(z.reshape(N, H, W, C), gamma, beta, slope)
    zg2.requires_grad_()
    y2 = av.BNPReLUMaxPoolFn.apply(zg2, gg2, bg2, sg2, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), 0.1, EPS, None)
    dx = av.BNPReLUMaxPoolFn.backward(y2.grad_fn, cuda(dy)[0])[0]
    torch.cuda.synchronize()
    assert_lift(dx, dx._dlip_lift)
