"""What the training entry points of encoder_train_ops.hip and video_train_ops.hip refuse, pinned down without a GPU.

DLIP_CHECK_ARG returns DLIP_EINVAL (-1) before any HIP call, so a refusal can be observed on a machine with no device: the
entry points are called through the ctypes binding with made-up integer addresses (no tensor is allocated).  Every case of the
table breaks exactly ONE condition of an otherwise acceptable call and must come back as -1; the acceptable calls themselves
(and the variants that drop a nullable pointer) must come back as anything BUT -1 -- with no device that is a HIP error code
from the launch that could not happen, which is also what a refusal lost in a refactor would turn into.

The module skips itself where a GPU is visible: there an accepted call would launch a kernel on the made-up addresses.
"""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

if torch.cuda.device_count() > 0:
    pytest.skip("a GPU is visible: an accepted call would launch on made-up addresses", allow_module_level=True)

EINVAL = -1


def P(i):
    """The i-th made-up device address: 4 KiB apart, so every one is 128-byte aligned."""
    return 0x10000 + 0x1000 * i


def ptrs(*names):
    return {n: P(i) for i, n in enumerate(names)}


def i32s(*v):
    return (ctypes.c_int32 * len(v))(*v)


def addrs(*v):
    return (ctypes.c_void_p * len(v))(*v)


class E:
    """One entry point: its acceptable call (name -> value, in ABI order), the refused variants, the accepted variants and
    the pointers its alignment conditions name (a16: 16-byte rules, a128: 128-byte rules; an item is a name, or
    (name, overrides) where the pointer only counts together with other arguments)."""

    def __init__(self, name, args, bad, a16=(), a128=(), ok=(), probe=True):
        self.name, self.args, self.bad, self.a16, self.a128, self.ok, self.probe = name, args, list(bad), a16, a128, list(ok), probe

    def call_args(self, over):
        assert set(over) <= set(self.args), (self.name, over)
        a = dict(self.args)
        a.update(over)
        return tuple(a.values())

    def refused(self):
        for label, over in self.bad:
            yield label, over
        for off, names in ((4, self.a16), (16, self.a128)):
            for item in names:
                n, extra = item if isinstance(item, tuple) else (item, {})
                base = extra.get(n, self.args[n])
                assert base is not None and base % 128 == 0, (self.name, n)
                yield f"{n} + {off}", {**extra, n: base + off}

    def accepted(self):
        if not self.probe:
            return
        yield "as is", {}
        for label, over in self.ok:
            yield label, over
        for item in tuple(self.a16) + tuple(self.a128):        # the aligned pointer alone (with what it needs) is acceptable
            if isinstance(item, tuple):
                yield f"{item[0]} aligned", item[1]


BN = dict(M=64, C=8)
ROWS_FWD_TAIL = dict(momentum=0.1, eps=1e-5)
RUNNING_PAIR = [("running_mean without running_var", dict(running_mean=P(40))), ("running_var without running_mean", dict(running_var=P(41)))]
RUNNING_OK = [("running pair given", dict(running_mean=P(40), running_var=P(41)))]
MS = dict(ms_coef=P(50), ms_T=4)       # dy formed on load from a MeanStdPooling's coefficients

ENCODER = [
    E("dlip_bn_rows_train_fwd_f32",
      dict(**ptrs("x", "gamma", "beta", "y", "save_mean", "save_invstd"), running_mean=None, running_var=None, workspace=P(8), **BN,
           **ROWS_FWD_TAIL, slope=0.01, act_first=0, ready_chunks=0, num_batches_tracked=None, stream=None),
      [("x null", dict(x=None)), ("C % 4", dict(C=6)), ("M = 0", dict(M=0)), *RUNNING_PAIR,
       ("ready_chunks < 0", dict(ready_chunks=-1)), ("ready_chunks > 0 with act_first", dict(ready_chunks=2, act_first=1))],
      a16=["x", "y"],
      ok=[("y null: statistics only", dict(y=None)), ("ready_chunks alone", dict(ready_chunks=2)), ("act_first alone", dict(act_first=1)),
          *RUNNING_OK]),
    E("dlip_bn_rows_train_bwd_f32",
      dict(**ptrs("dy", "x", "gamma", "beta", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "workspace"), **BN, slope=0.01,
           act_first=0, dx_lift2=None, stream=None),
      [("dy null", dict(dy=None)), ("workspace null", dict(workspace=None)), ("C % 4", dict(C=6))],
      a16=["x", "dy", "dx"], ok=[("dx_lift2 given", dict(dx_lift2=P(30)))]),
    E("dlip_meanstd_bwd_coef_f32", dict(**ptrs("y_pool", "g_pool", "coef"), B=2, C=8, T=4, stream=None),
      [("coef null", dict(coef=None)), ("T <= 1", dict(T=1)), ("B = 0", dict(B=0))]),
    E("dlip_bn_rows_train_bwd_ms_f32",
      dict(ms_coef=P(0), T=4, **{k: P(i) for i, k in enumerate(("x", "gamma", "beta", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "workspace"), 1)},
           M=8192, C=8, slope=0.01, dx_lift2=None, stream=None),
      [("ms_coef null", dict(ms_coef=None)), ("C % 4", dict(C=6)), ("T <= 1", dict(T=1)), ("M % T", dict(T=3)),
       ("M <= 4096: the small-row kernels take no coefficients", dict(M=4096))],
      a16=["x", "dx", "ms_coef"]),
    E("dlip_bn_rows_train_bwd_sums_f32",
      dict(**ptrs("dy", "x", "gamma", "beta", "save_mean", "save_invstd", "dgamma", "dbeta", "workspace", "amax_parts"), **BN, slope=0.01,
           act_first=0, dx_lift2=P(10), ms_coef=None, ms_T=0, stream=None),
      [("x null", dict(x=None)), ("dx_lift2 null", dict(dx_lift2=None)), ("C % 4", dict(C=6)), ("neither dy nor ms_coef", dict(dy=None)),
       ("ms_coef with act_first", dict(**MS, act_first=1)), ("ms_coef with ms_T <= 1", dict(ms_coef=P(50), ms_T=1)),
       ("ms_coef with M % ms_T", dict(ms_coef=P(50), ms_T=5))],
      a16=["x", "dy", ("ms_coef", MS)], ok=[("dy null with ms_coef", dict(dy=None, **MS)), ("act_first alone", dict(act_first=1))]),
    E("dlip_bn_prelu_rows_train_fwd_f32",
      dict(**ptrs("x", "gamma", "beta", "slope", "y", "save_mean", "save_invstd"), running_mean=None, running_var=None, workspace=P(9), **BN,
           **ROWS_FWD_TAIL, num_batches_tracked=None, stream=None),
      [("slope null", dict(slope=None)), ("C % 4", dict(C=6)), *RUNNING_PAIR], a16=["x", "y"],
      ok=[("y null: statistics only", dict(y=None)), *RUNNING_OK]),
    E("dlip_bn_prelu_rows_train_bwd_f32",
      dict(**ptrs("dy", "x", "gamma", "beta", "slope", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "dslope", "workspace"), **BN,
           dx_lift2=None, stream=None),
      [("dslope null", dict(dslope=None)), ("C % 4", dict(C=6))], a16=["x", "dy", "dx"]),
    E("dlip_bn_prelu_maxpool_train_fwd_f32",
      dict(**ptrs("x", "gamma", "beta", "slope", "y", "idx", "save_mean", "save_invstd"), running_mean=None, running_var=None, workspace=P(10),
           N=1, H=5, W=7, C=8, **ROWS_FWD_TAIL, num_batches_tracked=None, stream=None),
      [("idx null", dict(idx=None)), ("C % 4", dict(C=6)), *RUNNING_PAIR, ("N H W >= 2^31 - 1", dict(N=1 << 20, H=64, W=32))],
      a16=["x", "y"], ok=RUNNING_OK),
    E("dlip_bn_prelu_maxpool_train_bwd_f32",
      dict(**ptrs("dy_pooled", "dy_pooled2", "idx", "x", "gamma", "beta", "slope", "save_mean", "save_invstd", "dx", "dgamma", "dbeta", "dslope",
                  "workspace"), N=1, H=5, W=7, C=8, dx_lift2=None, stream=None),
      [("idx null", dict(idx=None)), ("C % 4", dict(C=6)), ("N H W >= 2^31 - 1", dict(N=1 << 20, H=64, W=32))],
      a16=["x", "dy_pooled", "dy_pooled2", "dx"], ok=[("dy_pooled2 null", dict(dy_pooled2=None)), ("dx_lift2 given", dict(dx_lift2=P(30)))]),
    E("dlip_bn_add_prelu_rows_train_fwd_f32",
      dict(**ptrs("x", "residual", "gamma", "beta", "slope", "sum", "y", "save_mean", "save_invstd"), running_mean=None, running_var=None,
           workspace=P(11), **BN, **ROWS_FWD_TAIL, num_batches_tracked=None, stream=None),
      [("residual null", dict(residual=None)), ("C % 4", dict(C=6)), *RUNNING_PAIR], a16=["x", "residual", "sum", "y"], ok=RUNNING_OK),
    E("dlip_bn_add_prelu_rows_train_bwd_f32",
      dict(**ptrs("dy", "dy2", "sum", "x", "gamma", "beta", "slope", "save_mean", "save_invstd", "dresidual", "dx", "dgamma", "dbeta", "dslope",
                  "workspace"), **BN, dx_lift2=None, stream=None),
      [("sum null", dict(sum=None)), ("C % 4", dict(C=6))], a16=["dy", "dy2", "sum", "x", "dresidual", "dx"],
      ok=[("dy2 null", dict(dy2=None))]),
    E("dlip_bn_apply_rows_f32",
      dict(**ptrs("x", "mean", "invstd", "gamma", "beta", "slope_vec"), slope=0.01, y=P(7), **BN, stream=None),
      [("y null", dict(y=None)), ("C % 4", dict(C=6))], a16=["x", "y"], ok=[("slope_vec null", dict(slope_vec=None))]),
    E("dlip_colsum_rows_f32", dict(**ptrs("x", "y", "workspace"), **BN, stream=None),
      [("workspace null", dict(workspace=None)), ("C % 4", dict(C=6))], a16=["x"]),
    E("dlip_meanstd_pool_bwd_f32", dict(**ptrs("x", "y", "dy", "dx"), B=2, T=4, C=8, stream=None),
      [("dy null", dict(dy=None)), ("T <= 1", dict(T=1)), ("C % 4", dict(C=6)), ("B > 65535", dict(B=65536))], a16=["x", "dx"]),
    E("dlip_meanstd_pool_bwd_bn_f32",
      dict(**ptrs("z", "mean", "invstd", "gamma", "beta"), slope=0.01, y=P(6), dy=P(7), dx=P(8), B=2, T=4, C=8, stream=None),
      [("gamma null", dict(gamma=None)), ("T <= 1", dict(T=1)), ("C % 4", dict(C=6)), ("B > 65535", dict(B=65536))], a16=["z", "dx"]),
    E("dlip_permute3_f32", dict(**ptrs("x", "y"), d0=2, d1=3, d2=4, p0=2, p1=0, p2=1, flip_axis=-1, stream=None),
      [("y null", dict(y=None)), ("d1 = 0", dict(d1=0)), ("not a permutation", dict(p0=0)), ("p2 out of range", dict(p2=3)),
       ("flip_axis out of range", dict(flip_axis=3))]),
    # (probe=False: these two answer a failed hipMemsetAsync with DLIP_EINVAL as well, so without a device their acceptable call
    # cannot be told from a refused one)
    E("dlip_pow2_scale_f32", dict(**ptrs("x", "scale2"), n=64, target=1024.0, stream=None),
      [("scale2 null", dict(scale2=None)), ("n = 0", dict(n=0)), ("target = 0", dict(target=0.0))], a16=["x"], probe=False),
    E("dlip_pow2_lift_f32", dict(**ptrs("x", "lift"), n=64, target=1024.0, stream=None),
      [("lift null", dict(lift=None)), ("n = 0", dict(n=0)), ("target = 0", dict(target=0.0))], a16=["x"], probe=False),
    E("dlip_split_pack_scaled_f32", dict(**ptrs("x", "y", "scale"), rows=4, C=32, stream=None),
      [("scale null", dict(scale=None)), ("C % 32", dict(C=16))]),
    E("dlip_split_pack_scaled_pad_f32", dict(**ptrs("x", "y", "scale"), rows=4, C=8, C_pad=32, stream=None),
      [("y null", dict(y=None)), ("C % 4", dict(C=6)), ("C_pad < C", dict(C=64)), ("C_pad % 32", dict(C_pad=48))], a16=["x"]),
    E("dlip_split_weights_rows_f32", dict(**ptrs("w", "w_split", "w_scale"), K=4, L=32, stream=None),
      [("w_scale null", dict(w_scale=None)), ("L % 32", dict(L=16))]),
    E("dlip_split_weights_perm_f32", dict(**ptrs("w_kct", "w_split", "w_scale"), K=4, C=32, T=3, mode=0, C_pad=0, stream=None),
      [("w_split null", dict(w_split=None)), ("mode = 2", dict(mode=2)), ("C_pad % 32", dict(C_pad=48)), ("C_pad < C", dict(C=64, C_pad=32)),
       ("default C_pad = C, C % 32", dict(C=16))], ok=[("mode 1: the inner extent is K", dict(mode=1, K=32, C=8))]),
    E("dlip_split_weights_multi_f32", dict(**ptrs("descs", "block_desc"), n_blocks=2, max_row_floats=64, stream=None),
      [("block_desc null", dict(block_desc=None)), ("n_blocks = 0", dict(n_blocks=0)), ("max_row_floats < 0", dict(max_row_floats=-1)),
       ("descs + 4 (8-byte rule)", dict(descs=P(0) + 4))]),
    E("dlip_fill_from_scalar_f32", dict(**ptrs("src", "y"), n=8, stream=None), [("src null", dict(src=None)), ("n = 0", dict(n=0))]),
]

BNV = ptrs("mean", "invstd", "gamma", "beta", "slope_vec")          # addresses P(0) .. P(4); the tensors follow from P(8)
BWDV = ptrs("mean", "invstd", "gamma", "beta", "dgamma", "dbeta")
ONE_TAP = dict(stride_h=1, stride_w=1, R=3, S=3, dil_h=1, dil_w=1, pad_h=1, pad_w=1)
UPS = dict(N=1, Ho=2, Wo=2, Hu=4, Wu=4, C=32, stride_h=2, stride_w=2)
POOL = dict(N=1, H=5, W=7, C=8)

VIDEO = [
    E("dlip_tap_gather_f32",
      dict(x=P(0), out=P(1), N=1, H=4, W=4, C=8, ldx=8, Ho=4, Wo=4, stride_h=1, stride_w=1, off_h=0, off_w=0, ldo=8, stream=None),
      [("x null", dict(x=None)), ("C % 4", dict(C=6)), ("ldx % 4", dict(ldx=10)), ("ldx < C", dict(ldx=4)), ("ldo < C", dict(ldo=4)),
       ("ldo % 4", dict(ldo=10))], a16=["out"]),
    E("dlip_wgrad_operand_f32",
      dict(x=P(0), out=P(1), ld_out=32, N=2, H=4, W=4, C=8, ldx=8, Ho=4, Wo=4, **ONE_TAP, scale=None, stream=None),
      [("out null", dict(out=None)), ("ld_out < J", dict(N=3)), ("ld_out % 32", dict(ld_out=48)), ("ldx < C", dict(ldx=4)), ("R = 0", dict(R=0))],
      a128=["out"], ok=[("x + 4: the generic tile", dict(x=P(0) + 4)), ("scale given", dict(scale=P(2))), ("C = 128", dict(C=128, ldx=128)),
                        ("C = 64", dict(C=64, ldx=64))]),
    E("dlip_wgrad_operand_split_f32", dict(x=P(0), out=P(1), ld_out=32, J=32, C=64, scale=P(2), nhwc_split_out=P(3), stream=None),
      [("nhwc_split_out null", dict(nhwc_split_out=None)), ("C % 64", dict(C=32)), ("ld_out < J", dict(J=33)), ("ld_out % 32", dict(ld_out=48))],
      a16=["x"], a128=["out", "nhwc_split_out"], ok=[("scale null", dict(scale=None)), ("C = 128", dict(C=128))]),
    E("dlip_wgrad_chwn_f32",
      dict(x=P(0), out=P(1), N=4, H=2, W=2, C=32, ldx=32, N32=32, scale=None, slice_major=1, nhwc_split_out=P(2), stream=None),
      [("out null", dict(out=None)), ("N32 < N", dict(N=33)), ("N32 % 32", dict(N32=48)), ("ldx < C", dict(ldx=16)),
       ("H W > 65535", dict(H=256, W=256)), ("nhwc_split_out with C % 32", dict(C=8, ldx=8))],
      a128=["out", "nhwc_split_out"],
      ok=[("nhwc_split_out null, C % 32 != 0", dict(nhwc_split_out=None, C=8, ldx=8)), ("x + 4: the generic tile", dict(x=P(0) + 4)),
          ("C = 128", dict(C=128, ldx=128)), ("C = 64", dict(C=64, ldx=64))]),
    E("dlip_wgrad_operand_split_bn_f32",
      dict(x=P(8), out=P(9), ld_out=32, J=32, C=64, **BNV, slope=0.01, nhwc_split_out=P(10), stream=None),
      [("mean null", dict(mean=None)), ("nhwc_split_out null", dict(nhwc_split_out=None)), ("C % 64", dict(C=32)), ("ld_out < J", dict(J=33)),
       ("ld_out % 32", dict(ld_out=48))],
      a16=["x"], a128=["out", "nhwc_split_out"], ok=[("slope_vec null", dict(slope_vec=None)), ("C = 128", dict(C=128))]),
    E("dlip_wgrad_chwn_bn_f32",
      dict(x=P(8), out=P(9), N=4, H=2, W=2, C=64, N32=32, **BNV, slope=0.01, nhwc_split_out=P(10), stream=None),
      [("beta null", dict(beta=None)), ("C % 64", dict(C=32)), ("N32 < N", dict(N=33)), ("N32 % 32", dict(N32=48)),
       ("H W > 65535", dict(H=256, W=256))],
      a16=["x"], a128=["out", "nhwc_split_out"], ok=[("slope_vec null", dict(slope_vec=None)), ("C = 128", dict(C=128))]),
    E("dlip_wgrad_operand_split_bnbwd_f32",
      dict(dy=P(8), z=P(9), out=P(10), ld_out=32, J=32, C=64, **BWDV, M=32, slope=0.01, act_first=0, lift=P(11), nhwc_split_out=P(12),
           ld_nhwc=0, ms_coef=None, ms_T=0, stream=None),
      [("z null", dict(z=None)), ("lift null", dict(lift=None)), ("C % 4", dict(C=62, ld_nhwc=64)), ("ld_out < J", dict(J=33)), ("M = 0", dict(M=0)),
       ("neither dy nor ms_coef", dict(dy=None)), ("ms_coef with act_first", dict(**MS, act_first=1)),
       ("ms_coef with ms_T <= 1", dict(ms_coef=P(50), ms_T=1)), ("ms_coef with J % ms_T", dict(ms_coef=P(50), ms_T=5)),
       ("ld_nhwc = 0, nhwc_split_out with C % 32", dict(C=8)), ("ld_nhwc < C", dict(ld_nhwc=32)), ("ld_nhwc % 32", dict(ld_nhwc=80))],
      a16=["dy", "z", ("ms_coef", MS)], a128=["out", "nhwc_split_out"],
      ok=[("dy null with ms_coef", dict(dy=None, **MS)), ("nhwc_split_out null, C % 32 != 0", dict(nhwc_split_out=None, C=8)),
          ("ld_nhwc given, C % 32 != 0", dict(C=40, ld_nhwc=64)), ("act_first alone", dict(act_first=1)), ("C = 128", dict(C=128)),
          ("C > 512, ragged", dict(C=520, ld_nhwc=544))]),
    E("dlip_wgrad_chwn_bnbwd_f32",
      dict(dy=P(8), z=P(9), out=P(10), N=4, H=2, W=2, C=64, N32=32, **BWDV, M=16, slope=0.01, act_first=0, lift=P(11), nhwc_split_out=P(12),
           stream=None),
      [("dy null", dict(dy=None)), ("dbeta null", dict(dbeta=None)), ("C % 64", dict(C=32)), ("N32 < N", dict(N=33)), ("M = 0", dict(M=0)),
       ("H W > 65535", dict(H=256, W=256))],
      a16=["dy", "z"], a128=["out", "nhwc_split_out"], ok=[("nhwc_split_out null", dict(nhwc_split_out=None)), ("C = 128", dict(C=128))]),
    E("dlip_stem_wgrad_chwn_f32", dict(x=P(0), out=P(1), B=1, T=4, H=4, W=4, N32=32, slice_major=1, stream=None),
      [("x null", dict(x=None)), ("N32 < B T", dict(T=33)), ("N32 % 32", dict(N32=48))], a128=["out"]),
    E("dlip_upsample_zero_f32", dict(dz=P(0), out=P(1), **UPS, stream=None),
      [("out null", dict(out=None)), ("C % 4", dict(C=6)), ("stride_w = 0", dict(stride_w=0))]),
    E("dlip_upsample_zero_split_f32", dict(dz=P(0), out_split=P(1), scale=P(2), **UPS, stream=None),
      [("scale null", dict(scale=None)), ("C % 32", dict(C=16))], a16=["dz"], a128=["out_split"]),
    E("dlip_prelu_rows_fwd_f32", dict(**ptrs("x", "slope", "y"), **BN, stream=None), [("slope null", dict(slope=None)), ("C % 4", dict(C=6))]),
    E("dlip_prelu_rows_bwd_f32", dict(**ptrs("dy", "x", "slope", "dx", "dslope_terms"), **BN, stream=None),
      [("dslope_terms null", dict(dslope_terms=None)), ("C % 4", dict(C=6))]),
    E("dlip_add_prelu_rows_fwd_f32", dict(**ptrs("a", "b", "slope", "sum", "y"), **BN, stream=None),
      [("b null", dict(b=None)), ("C % 4", dict(C=6))]),
    E("dlip_maxpool3x3s2_bwd_f32", dict(**ptrs("x", "dy", "dx"), **POOL, stream=None), [("dy null", dict(dy=None)), ("C % 4", dict(C=6))]),
    E("dlip_maxpool3x3s2_idx_f32", dict(**ptrs("x", "y", "idx"), **POOL, stream=None), [("idx null", dict(idx=None)), ("C % 4", dict(C=6))]),
    E("dlip_maxpool3x3s2_bwd_idx_f32", dict(**ptrs("idx", "dy", "dx"), **POOL, stream=None), [("idx null", dict(idx=None)), ("C % 4", dict(C=6))]),
    E("dlip_row_broadcast_f32", dict(**ptrs("dy", "lengths", "dx"), N=2, P=3, C=8, scale=1.0, stream=None),
      [("dx null", dict(dx=None)), ("C % 4", dict(C=6)), ("P = 0", dict(P=0))], ok=[("lengths null", dict(lengths=None))]),
    E("dlip_stem_im2col_f32", dict(**ptrs("x", "col"), B=1, T=2, H=8, W=8, stream=None),
      [("col null", dict(col=None)), ("H odd", dict(H=7)), ("W = 1", dict(W=1))]),
    E("dlip_stem_wgrad_operand_f32", dict(x=P(0), out=P(1), ld_out=32, B=1, T=2, H=8, W=8, stream=None),
      [("x null", dict(x=None)), ("W odd", dict(W=7)), ("ld_out < J", dict(T=3)), ("ld_out % 32", dict(ld_out=48))], a128=["out"]),
    E("dlip_split_stem_weights_f32", dict(**ptrs("w", "w_img", "w_scale"), K=4, stream=None), [("w_img null", dict(w_img=None)), ("K = 0", dict(K=0))]),
    E("dlip_dropout_keep_f32", dict(**ptrs("x", "u", "y"), n=8, p=0.5, scale=2.0, stream=None),
      [("u null", dict(u=None)), ("n = 0", dict(n=0)), ("p = 1", dict(p=1.0)), ("p < 0", dict(p=-0.5))]),
    # (the three arrays are read on the host: real ones, of made-up device addresses)
    E("dlip_chomp_concat_f32",
      dict(branches=addrs(P(0), P(1)), lengths=i32s(6, 8), widths=i32s(8, 4), n_branches=2, cat=P(2), B=1, T=4, backward=0, stream=None),
      [("cat null", dict(cat=None)), ("widths null", dict(widths=None)), ("n_branches = 5", dict(n_branches=5)), ("T = 0", dict(T=0)),
       ("a branch null", dict(branches=addrs(P(0), None))), ("a width % 4", dict(widths=i32s(8, 6))), ("a length < T", dict(lengths=i32s(6, 2))),
       ("length - T odd", dict(lengths=i32s(7, 8))), ("branches[0] + 4", dict(branches=addrs(P(0) + 4, P(1)))),
       ("branches[1] + 4", dict(branches=addrs(P(0), P(1) + 4))), ("cat + 4", dict(cat=P(2) + 4))],
      ok=[("backward", dict(backward=1))]),
    E("dlip_mul_mask_f32", dict(**ptrs("x", "mask", "y"), n=8, scale=1.0, stream=None), [("mask null", dict(mask=None)), ("n = 0", dict(n=0))]),
]

TABLE = ENCODER + VIDEO
REFUSED = [pytest.param(e, over, id=f"{e.name}: {label}") for e in TABLE for label, over in e.refused()]
ACCEPTED = [pytest.param(e, over, id=f"{e.name}: {label}") for e in TABLE for label, over in e.accepted()]


def checked_entry_points(source):
    """The extern "C" entry points of a translation unit whose body has a DLIP_CHECK_ARG."""
    text = open(os.path.join(ROOT, "deeplip_amd", "csrc", source)).read()
    parts = re.split(r'extern "C" int(?:32_t)? (dlip_[a-z0-9_]+)\(', text)
    return [name for name, body in zip(parts[1::2], parts[2::2]) if "DLIP_CHECK_ARG" in body]


def test_table_covers_every_checked_entry_point():
    assert [e.name for e in ENCODER] == checked_entry_points("encoder_train_ops.hip")
    assert [e.name for e in VIDEO] == checked_entry_points("video_train_ops.hip")
    from deeplip_amd import _lib
    for e in TABLE:
        assert len(e.args) == len(_lib.SIGNATURES[e.name]), e.name
        assert list(e.args)[-1] == "stream"


@pytest.mark.parametrize("e, over", REFUSED)
def test_refused(e, over):
    from deeplip_amd import _lib
    assert getattr(_lib.lib(), e.name)(*e.call_args(over)) == EINVAL


@pytest.mark.parametrize("e, over", ACCEPTED)
def test_accepted_up_to_the_launch(e, over):
    """The call each refused case departs from passes every argument check (no device: the launch itself then fails, with a HIP
    error code) -- so a refused case is refused for the one condition it breaks."""
    from deeplip_amd import _lib
    assert torch.cuda.device_count() == 0
    assert getattr(_lib.lib(), e.name)(*e.call_args(over)) != EINVAL
