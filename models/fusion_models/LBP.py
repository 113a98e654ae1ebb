"""Drop-in for the reference's models/fusion_models/LBP.py (BNBilinear: the class its train_fusion.py:84 names)."""
from deeplip_amd.fusion import BNBilinear, LowFER  # noqa: F401
