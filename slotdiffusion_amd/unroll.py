"""From a trained LDMSlotFormer to the slots file the VQA readout trains on (the reference's
vp_vqa/rollout_physion_slots.py:22-63): the observed frames of every video are kept, the rest is the rollouter's
prediction from the last observed frames.

    rollout_slots_file(model, 'slots.pkl', 'rollout_readout_slots.pkl', ('train', 'val'), video_len=150)
    params.slots_root = 'rollout_readout_slots.pkl'       # vp_vqa.build_dataset -> SlotsLabelFileDataModule

A model trained with `frame_offset` o sees every o-th frame, so the reference rolls o interleaved streams out one after
the other (frames obs + off, obs + off + o, ... for off < o) and interleaves the results.  Here the o streams of a batch
of videos are the sequences of ONE model.unroll call: the rollout is autoregressive, so a stream that needs fewer steps
takes a prefix of the common pred_len and the surplus steps are dropped."""
import os

import numpy as np
import torch

from .extract import dump_slots, load_slots


@torch.no_grad()
def rollout_video_slots(model, video_slots, files, video_len, obs_frames=45, frame_offset=3, batch_size=1):
    """rollout_physion_slots.py:22-63.  video_slots {basename: ndarray [T, N, C]}, files: the videos to process (looked up
    by basename) -> ndarray [len(files), video_len, N, C] fp32.  With h = model.history_len: frames [0, obs_frames) are
    the stored ones; frame f >= obs_frames, off = (f - obs_frames) % frame_offset, k = (f - obs_frames) // frame_offset,
    is step k of the rollout whose burn-in is frames obs_frames - h frame_offset + off + j frame_offset, j < h."""
    h = int(model.history_len)
    if frame_offset < 1:
        raise ValueError(f'frame_offset={frame_offset}: must be at least 1')
    if batch_size < 1:
        raise ValueError(f'batch_size={batch_size}: must be at least 1')
    if obs_frames < h * frame_offset:
        raise ValueError(f'obs_frames={obs_frames}: the burn-in needs history_len * frame_offset = {h * frame_offset} '
                         'observed frames')
    if video_len <= obs_frames:
        raise ValueError(f'video_len={video_len}: nothing to roll out behind obs_frames={obs_frames}')
    names = [os.path.basename(f) for f in files]
    for n in names:
        if n not in video_slots:
            raise KeyError(f'files: {n!r} is not in the slots file')
        if video_slots[n].shape[0] < video_len:
            raise ValueError(f'files: {n!r} has {video_slots[n].shape[0]} frames, video_len is {video_len}')
    if hasattr(model, 'eval'):
        model.eval()
    device = getattr(model, 'device', 'cpu')
    o = frame_offset
    pred_len = (video_len - obs_frames + o - 1) // o
    # burn-in frame j of stream off, [o, h]; (stream, step) of predicted frame i, [video_len - obs_frames]
    burn = obs_frames - h * o + np.arange(o)[:, None] + o * np.arange(h)[None, :]
    i = np.arange(video_len - obs_frames)
    out = []
    for start in range(0, len(names), batch_size):
        ori = np.stack([np.asarray(video_slots[n][:video_len], dtype=np.float32) for n in names[start:start + batch_size]])
        B, _, N, C = ori.shape
        past = torch.from_numpy(ori[:, burn].reshape(B * o, h, N, C)).to(device)
        pred = model.unroll(past, pred_len).float().cpu().numpy().reshape(B, o, pred_len, N, C)
        out.append(np.concatenate([ori[:, :obs_frames], pred[:, i % o, i // o]], axis=1))
    return np.concatenate(out, axis=0)


def rollout_slots_file(model, src_path, dst_path, splits, **kw):
    """The stage: the slots file at `src_path` (extract.dump_slots / the reference's pickle layout) -> the same layout at
    `dst_path` with every video of `splits` rolled out (rollout_video_slots(**kw)), videos in sorted order.  Returns what
    was written."""
    data = load_slots(src_path)
    out = {}
    for split in splits:
        if split not in data:
            raise KeyError(f'splits: {src_path} has no split {split!r}')
        files = sorted(data[split])
        out[split] = (files, rollout_video_slots(model, data[split], files, **kw))
    return dump_slots(dst_path, out)
