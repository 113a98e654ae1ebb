#!/usr/bin/env python3
"""Capture golden vectors of the REFERENCE's ShuffleNet lip-clip encoder (Lipreading(backbone_type='shufflenet')); run in the
build container only, like capture_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/capture_shufflenet_golden.py

Imports ``models.*`` from the reference checkout (read-only), overwrites every parameter / buffer with
``deeplip_amd.weightgen.fill_state_dict`` (name-keyed, seed 1, one prefix per model), feeds ``weightgen.video_input`` clips and
writes DATA only to ``shufflenet_golden.npz``: the key/shape manifest of every width, features, logits, per-stage tensors of one
frame and the 112 x 112 features (whose last map is 4 x 4: AvgPool2d(3) keeps the top-left 3 x 3 window).
"""
import json
import os
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
from models.video_models.model import Lipreading, threeD_to_2D_tensor  # noqa: E402
import models  # noqa: E402
assert os.path.realpath(os.path.dirname(models.__path__[0] if hasattr(models, "__path__") else models.__file__)).startswith(os.path.realpath(REF)), "reference not imported"

torch.set_num_threads(8)
torch.manual_seed(1)

TCN_OPTS = {"num_layers": 4, "kernel_size": [3, 5, 7], "dropout": 0.2, "dwpw": False, "width_mult": 1}
WIDTHS = (0.5, 1.0, 1.5, 2.0)
NUM_CLASSES = 54


def wtag(w):
    return str(w).replace(".", "p")


def build(width, relu_type="prelu", extract_feats=True, prefix=None):
    net = Lipreading(hidden_dim=256, backbone_type="shufflenet", num_classes=NUM_CLASSES, relu_type=relu_type,
                     tcn_options=TCN_OPTS, width_mult=width, extract_feats=extract_feats)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = wg.fill_state_dict(shapes, prefix=prefix if prefix is not None else f"shufflenet_{wtag(width)}_{relu_type}.")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net.eval()
    return net, shapes


def main():
    out = {}
    x = torch.from_numpy(wg.video_input(2, frames=5, key="shufflenet.video"))
    with torch.no_grad():
        for w in WIDTHS:
            net, shapes = build(w)
            out[f"manifest_w{wtag(w)}"] = np.array(json.dumps(sorted([k, list(s)] for k, s in shapes.items())))
            out[f"feats_w{wtag(w)}"] = net(x, [5, 5]).numpy()
        net, _ = build(1.0, relu_type="relu")
        out["feats_w1p0_relu"] = net(x, [5, 5]).numpy()

        # MS-TCN logits, width 1.0, B = 4, mixed lengths (the padding frames go through the net; only the consensus is masked)
        net, _ = build(1.0, extract_feats=False)
        xl = torch.from_numpy(wg.video_input(4, frames=8, key="shufflenet.video.logits"))
        lengths = [8, 6, 5, 3]
        logits = net(xl, lengths)
        out["logits_w1p0"] = logits.numpy()
        out["logits_lengths"] = np.array(lengths, dtype=np.int32)
        out["logits_argmax"] = logits.argmax(dim=1).numpy().astype(np.int64)

        # one frame's tensors after the stem and every stage (width 1.0 prelu: the net of feats_w1p0), NCHW
        net, _ = build(1.0)
        y = threeD_to_2D_tensor(net.frontend3D(x))
        out["tap_stem"] = y[0].numpy()
        feats = net.trunk[0]
        y = feats[0:4](y); out["tap_stage2"] = y[0].numpy()
        y = feats[4:12](y); out["tap_stage3"] = y[0].numpy()
        y = feats[12:16](y); out["tap_stage4"] = y[0].numpy()
        y = net.trunk[1](y); out["tap_conv_last"] = y[0].numpy()

        # 112 x 112: the last map is 4 x 4 and the reference averages its top-left 3 x 3 window
        x112 = torch.from_numpy(wg.video_input(1, frames=3, size=112, key="shufflenet.video.112"))
        out["feats_w1p0_112"] = net(x112, [3]).numpy()
    np.savez_compressed(os.path.join(HERE, "shufflenet_golden.npz"), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype)


if __name__ == "__main__":
    main()
