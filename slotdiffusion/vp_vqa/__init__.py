"""`slotdiffusion.vp_vqa` registry surface (build_dataset / build_model / build_method)."""
from slotdiffusion_amd.vp_vqa import build_dataset, build_method, build_model  # noqa: F401
