"""models/inpaint.py: `Inpainter(model_dir)(image, mask) -> float32 [H, W, 3]`, LBAMModel(4, 3) on the GPU
(bodyfitting_amd.inpaint.Inpainter).  The training-only VGG16FeatureExtractor has no counterpart."""
from bodyfitting_amd.inpaint import Inpainter  # noqa: F401
