"""Drop-in for the reference's models/audio_models/tdnn.py."""
from deeplip_amd.audio import SpeakerEmbNet, TDNN_Block  # noqa: F401
from deeplip_amd.audio import FTDNN_Block  # noqa: F401  (`arch: ftdnn`: the build's own definition)
from deeplip_amd.audio import MeanStdPooling, AttentiveStatPooling  # noqa: F401  (tdnn.py:5 star-imports pooling)
from deeplip_amd.sincnet import SincConv  # noqa: F401  (`arch: sincnet`: the build's own definition)
