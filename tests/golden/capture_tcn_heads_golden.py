#!/usr/bin/env python3
"""Capture golden vectors of the REFERENCE's single-branch TCN head and depthwise-separable (dwpw) heads (models/video_models/
model.py:40-58, tcn.py:28-59,145-237); run in the build container only, like capture_shufflenet_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_tcn_heads_golden.py

Imports ``models.*`` from the reference checkout (read-only), fills every parameter / buffer with
``deeplip_amd.weightgen.fill_state_dict`` (name-keyed, seed 1, one prefix per variant; see ``fill`` for the aliased keys of a
TemporalBlock) and writes DATA only to ``tcn_heads_golden.npz``:
  manifest_<v>            key/shape manifest of each head variant (VARIANTS)
  lengths                 the consensus lengths of the features weightgen.gen("tcn_heads.x.<C>", (B, T, C)) (channels-last)
  logits_<v>, block<i>_<v>  eval logits and every block's output [B,T,C] of each variant
  model_logits_resnet_k3, model_logits_shufflenet0p5_k3_dwpw (+ model_lengths): whole-model eval logits of
                          weightgen.video_input(2, frames=5, key="tcn_heads.video")
  train_<h>_*             one train-mode step of a small head (dropout 0): loss = sum(logits * train_G), each parameter's gradient
                          (.grad.<name>), each BatchNorm's updated running statistics (.buf.<name>); the features are
                          weightgen.gen("tcn_heads.train.x.<h>", (TRAIN_B, TRAIN_T, C))
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DEEPLIP_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deeplip_amd import weightgen as wg  # noqa: E402

sys.path = [p for p in sys.path if os.path.realpath(p or os.getcwd()) != os.path.realpath(ROOT)]
sys.path.insert(0, REF)
for m in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
    del sys.modules[m]
from models.video_models.model import TCN, Lipreading, MultiscaleMultibranchTCN  # noqa: E402
import models  # noqa: E402
assert os.path.realpath(os.path.dirname(models.__path__[0] if hasattr(models, "__path__") else models.__file__)).startswith(os.path.realpath(REF)), "reference not imported"

torch.set_num_threads(8)
torch.manual_seed(1)

NUM_CLASSES = 54
B, T = 2, 8
LENGTHS = [8, 6]
# name -> (kernel_size, dwpw, relu_type, width_mult, input channels)
VARIANTS = {
    "k3_prelu": ([3], False, "prelu", 1, 512),
    "k3_relu": ([3], False, "relu", 1, 512),
    "k3_dwpw": ([3], True, "prelu", 1, 512),
    "k357_dwpw": ([3, 5, 7], True, "prelu", 1, 512),
    "k3_wm2": ([3], False, "prelu", 2, 512),
    "k3_c1024": ([3], False, "prelu", 1, 1024),
    "k3_dwpw_c1024": ([3], True, "prelu", 1, 1024),
}
# small heads for the train step: name -> (kernel_size, dwpw, input channels, num_channels)
TRAIN = {
    "k3": ([3], False, 64, [32] * 3),
    "k3_dwpw": ([3], True, 64, [32] * 3),
    "k357_dwpw": ([3, 5, 7], True, 64, [48] * 2),
}
TRAIN_B, TRAIN_T, TRAIN_LENGTHS, TRAIN_CLASSES = 4, 10, [10, 9, 7, 10], 10

# A non-dwpw TemporalBlock holds conv1 .. relu2 under two names each (tcn.py:205-206); both name one tensor, so the filled state
# dict gives the alias the value of the ``net.<i>`` name.
ALIAS = {"conv1": "0", "batchnorm1": "1", "relu1": "3", "conv2": "5", "batchnorm2": "6", "relu2": "8"}


def fill(shapes, prefix):
    sd = wg.fill_state_dict(shapes, prefix=prefix)
    for k in list(sd):
        m = re.match(r"(.*)\.(conv1|batchnorm1|relu1|conv2|batchnorm2|relu2)\.([a-z_]+)$", k)
        if m and f"{m.group(1)}.net.{ALIAS[m.group(2)]}.{m.group(3)}" in sd:
            sd[k] = sd[f"{m.group(1)}.net.{ALIAS[m.group(2)]}.{m.group(3)}"]
    return sd


def opts(ks, dwpw, wm=1, layers=4, dropout=0.2):
    return {"num_layers": layers, "kernel_size": ks, "dropout": dropout, "dwpw": dwpw, "width_mult": wm}


def head(ks, dwpw, relu_type, wm, cin, prefix):
    o = opts(ks, dwpw, wm)
    cls = TCN if len(ks) == 1 else MultiscaleMultibranchTCN
    h = cls(input_size=cin, num_channels=[256 * len(ks) * wm] * 4, num_classes=NUM_CLASSES, tcn_options=o, dropout=0.2,
            relu_type=relu_type, dwpw=dwpw)
    shapes = {k: tuple(v.shape) for k, v in h.state_dict().items()}
    h.load_state_dict({k: torch.from_numpy(v) for k, v in fill(shapes, prefix).items()}, strict=True)
    return h.eval(), shapes


def trunk(h):
    return h.tcn_trunk.network if isinstance(h, TCN) else h.mb_ms_tcn.network


def main():
    out = {"lengths": np.array(LENGTHS, dtype=np.int32)}
    with torch.no_grad():
        for v, (ks, dwpw, relu_type, wm, cin) in VARIANTS.items():
            h, shapes = head(ks, dwpw, relu_type, wm, cin, f"tcn_heads.{v}.")
            out[f"manifest_{v}"] = np.array(json.dumps(sorted([k, list(s)] for k, s in shapes.items())))
            x = torch.from_numpy(wg.gen(f"tcn_heads.x.{cin}", (B, T, cin)))
            out[f"logits_{v}"] = h(x, LENGTHS, B).numpy()
            y = x.transpose(1, 2)
            for i, blk in enumerate(trunk(h)):
                y = blk(y)
                out[f"block{i}_{v}"] = y.transpose(1, 2).contiguous().numpy()

        # whole models: ResNet + [3] (dense, prelu) and ShuffleNet 0.5 + [3] dwpw
        xm = torch.from_numpy(wg.video_input(2, frames=5, key="tcn_heads.video"))
        out["model_lengths"] = np.array([5, 4], dtype=np.int32)      # (the clips: weightgen.video_input(2, frames=5, key="tcn_heads.video"))
        for name, bb, w, dwpw in (("resnet_k3", "resnet", 1.0, False), ("shufflenet0p5_k3_dwpw", "shufflenet", 0.5, True)):
            net = Lipreading(hidden_dim=256, backbone_type=bb, num_classes=NUM_CLASSES, relu_type="prelu",
                             tcn_options=opts([3], dwpw), width_mult=w)
            shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
            net.load_state_dict({k: torch.from_numpy(v) for k, v in fill(shapes, f"tcn_heads.model.{name}.").items()}, strict=True)
            out[f"model_logits_{name}"] = net.eval()(xm, [5, 4]).numpy()

    # one train-mode step of each small head (dropout 0: deterministic)
    out["train_lengths"] = np.array(TRAIN_LENGTHS, dtype=np.int32)
    out["train_G"] = wg.gen("tcn_heads.train.G", (TRAIN_B, TRAIN_CLASSES))
    for name, (ks, dwpw, cin, chans) in TRAIN.items():
        cls = TCN if len(ks) == 1 else MultiscaleMultibranchTCN
        h = cls(input_size=cin, num_channels=chans, num_classes=TRAIN_CLASSES, tcn_options=opts(ks, dwpw, layers=len(chans), dropout=0.0),
                dropout=0.0, relu_type="prelu", dwpw=dwpw)
        shapes = {k: tuple(v.shape) for k, v in h.state_dict().items()}
        h.load_state_dict({k: torch.from_numpy(v) for k, v in fill(shapes, f"tcn_heads.train.{name}.").items()}, strict=True)
        h.train()
        x = wg.gen(f"tcn_heads.train.x.{name}", (TRAIN_B, TRAIN_T, cin))
        logits = h(torch.from_numpy(x), TRAIN_LENGTHS, TRAIN_B)
        loss = (logits * torch.from_numpy(out["train_G"])).sum()
        loss.backward()
        out[f"train_{name}_loss"] = np.array(loss.item(), dtype=np.float64)
        for pn, p in h.named_parameters():
            out[f"train_{name}.grad.{pn}"] = p.grad.numpy().copy()
        for bn, b in h.named_buffers():
            if bn.endswith("running_mean") or bn.endswith("running_var"):
                out[f"train_{name}.buf.{bn}"] = b.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "tcn_heads_golden.npz"), **out)
    for k, v in out.items():
        if not k.startswith("train_") or ".grad." not in k:
            print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
