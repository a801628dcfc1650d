"""Registry module with the surface of `slotdiffusion.vp_vqa` (scripts/train.py:97-100): video prediction with
LDMSlotFormer, and the VQA readout on its rollouts with PhysionReadout."""
import os

from .. import models as _models
from ..method import (SlotsFileDataModule, SyntheticSlotsDataModule, SyntheticSlotsLabelDataModule,  # noqa: F401
                      build_method)


def build_model(params):
    """vp_vqa/models/__init__.py:9-22."""
    if params.model == 'LDMSlotFormer':
        return _models.LDMSlotFormer(resolution=params.resolution, clip_len=params.input_frames,
                                     slot_dict=params.slot_dict, dec_dict=params.dec_dict,
                                     rollout_dict=params.rollout_dict, loss_dict=params.loss_dict)
    return _models.build_model(params)          # PhysionReadout (needs params.readout_dict); refusals by name


def build_dataset(params, val_only=False):
    """Datasets are out of scope; synthetic slots [B, history + rollout, N, D], for the readout
    [B, video_len, N, D] with a label.  A `params.slots_root` that exists (the file extract.dump_slots writes) feeds
    LDMSlotFormer windows of the extracted slots instead."""
    if params.model == 'PhysionReadout':
        return SyntheticSlotsLabelDataModule(params)
    root = params.get('slots_root') if hasattr(params, 'get') else getattr(params, 'slots_root', None)
    if root and os.path.exists(root):
        return SlotsFileDataModule(params, root, split='val' if val_only else 'train')
    return SyntheticSlotsDataModule(params)
