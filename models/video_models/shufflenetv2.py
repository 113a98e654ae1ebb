"""Drop-in for the reference's models/video_models/shufflenetv2.py."""
from deeplip_amd.shufflenet import InvertedResidual, ShuffleNetV2, channel_shuffle, conv_1x1_bn, conv_bn  # noqa: F401
