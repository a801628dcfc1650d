"""Registry module with the surface of `slotdiffusion.video_based` (scripts/train.py:97-100)."""
from ..evaluate import evaluate_video_segmentation  # noqa: F401
from ..extract import extract_video_slots  # noqa: F401
from ..method import SyntheticDataModule, build_method  # noqa: F401
from ..models import build_model  # noqa: F401
from ..quality import evaluate_compositional_generation, evaluate_video_reconstruction  # noqa: F401


def build_dataset(params, val_only=False):
    """Datasets are out of scope; clips of `n_sample_frames` synthetic frames."""
    return SyntheticDataModule(params, frames=getattr(params, 'n_sample_frames', 3))
