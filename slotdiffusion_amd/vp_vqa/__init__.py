"""Registry module with the surface of `slotdiffusion.vp_vqa` (scripts/train.py:97-100): video prediction with
LDMSlotFormer, and the VQA readout on its rollouts with PhysionReadout."""
import os

from .. import models as _models
from ..method import (SlotsFileDataModule, SlotsLabelFileDataModule, SyntheticSlotsDataModule,  # noqa: F401
                      SyntheticSlotsLabelDataModule, build_method)
from ..quality import evaluate_video_prediction  # noqa: F401
from ..vqa import (PhysionVQATestSet, ReadoutBank, evaluate_physion_vqa, format_report, logit_cuts)  # noqa: F401

# the labels of the two Physion subsets under params.data_root (vp_vqa/datasets/physion.py:250-253)
PHYSION_LABELS = {'readout': 'PhysionTrainMP4s/readout_labels.csv', 'test': 'PhysionTestMP4s/labels.csv'}


def build_model(params):
    """vp_vqa/models/__init__.py:9-22."""
    if params.model == 'LDMSlotFormer':
        return _models.LDMSlotFormer(resolution=params.resolution, clip_len=params.input_frames,
                                     slot_dict=params.slot_dict, dec_dict=params.dec_dict,
                                     rollout_dict=params.rollout_dict, loss_dict=params.loss_dict)
    return _models.build_model(params)          # PhysionReadout (needs params.readout_dict); refusals by name


def _param(params, name):
    return params.get(name) if hasattr(params, 'get') else getattr(params, name, None)


def build_dataset(params, val_only=False):
    """The Physion readers are out of scope; synthetic slots [B, history + rollout, N, D], for the
    readout [B, video_len, N, D] with a label.  A `params.slots_root` that exists (the file extract.dump_slots writes)
    feeds LDMSlotFormer windows of the extracted slots instead; for PhysionReadout it (the file
    unroll.rollout_slots_file writes) is read together with the subset's labels CSV under `params.data_root` -- the test
    subset when `params.dataset` names it, the readout subset otherwise -- and only when both files exist."""
    root = _param(params, 'slots_root')
    if params.model == 'PhysionReadout':
        subset = 'test' if 'test' in str(_param(params, 'dataset') or '') else 'readout'
        data_root = _param(params, 'data_root')
        csv_path = os.path.join(data_root, PHYSION_LABELS[subset]) if data_root else None
        if root and os.path.exists(root) and csv_path and os.path.exists(csv_path):
            split = 'test' if subset == 'test' else ('val' if val_only else 'train')
            return SlotsLabelFileDataModule(params, root, csv_path, split=split)
        return SyntheticSlotsLabelDataModule(params)
    if root and os.path.exists(root):
        return SlotsFileDataModule(params, root, split='val' if val_only else 'train')
    return SyntheticSlotsDataModule(params)
