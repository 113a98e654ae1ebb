"""Drop-in for the reference's models/fusion_models/compact_bilinear_pooling.py (the import of its train_fusion.py:31-32)."""
from deeplip_amd.fusion import CompactBilinearPooling  # noqa: F401
