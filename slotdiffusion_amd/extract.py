"""From a video checkpoint to the slots file the vp_vqa task starts from (the reference's
video_based/extract_slots.py:18-62 with the long-video path of video_based/models/savi.py:402-443).

    slots = extract_video_slots(model, dataset, batch_size=4)            # [num_videos, T, N, C] numpy
    dump_slots(path, {'train': (files, slots), 'val': (val_files, val_slots)})
    params.slots_root = path                                             # vp_vqa.build_dataset -> SlotsFileDataModule

The reference bounds memory on long videos by halving the clip on out-of-memory errors; here a video is walked in
chunks of a fixed `chunk_len` frames (model.encode_stream -> engine.encode_stream), the last slots and the LSTM wrapper's
state carried from chunk to chunk, so memory is bounded by the chunk and the walk is deterministic."""
import os
import pickle

import numpy as np
import torch


@torch.no_grad()
def extract_video_slots(model, dataset, batch_size=1, chunk_len=None):
    """extract_slots.py:18-37.  dataset: `num_videos` and `get_video(i) -> {'video': [T, 3, H, W]}` (one T per batch of
    videos) -> numpy [num_videos, T, N, C].  Per batch of `batch_size` videos the clip is walked in chunks of `chunk_len`
    frames (default model.clip_len): chunk k + 1 starts from the last slots of chunk k, and only the first chunk of a
    video (prev_slots None) resets the model's PredictorState (savi.py:453-455)."""
    model.eval()
    chunk_len = int(chunk_len or model.clip_len)
    assert chunk_len >= 1 and batch_size >= 1
    device = getattr(model, 'device', 'cpu')
    all_slots = []
    for start in range(0, dataset.num_videos, batch_size):
        vids = [torch.as_tensor(dataset.get_video(i)['video']) for i in range(start, min(start + batch_size, dataset.num_videos))]
        video = torch.stack(vids).float()                                 # [B, T, 3, H, W]
        prev, parts = None, []
        for t0 in range(0, video.shape[1], chunk_len):
            chunk = video[:, t0:t0 + chunk_len].to(device)
            slots = model.encode_stream(chunk, prev)                      # [B, Tc, N, C]
            prev = slots[:, -1]
            parts.append(slots.detach().cpu())
        all_slots += list(torch.cat(parts, 1).numpy())
    return np.stack(all_slots, axis=0)


def dump_slots(path, splits):
    """extract_slots.py:50-62: {split: (files, slots [n, T, N, C])} -> the pickled dict {split: {basename(file):
    ndarray [T, N, C]}} at `path`."""
    out = {}
    for split, (files, slots) in splits.items():
        assert len(files) == len(slots), (split, len(files), len(slots))
        out[split] = {os.path.basename(f): np.asarray(s) for f, s in zip(files, slots)}
        assert len(out[split]) == len(files), f'{split}: two files share a basename'
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, 'wb') as f:
        pickle.dump(out, f)
    return out


def load_slots(path):
    """-> {split: {basename: ndarray [T, N, C]}} as dump_slots (and the reference) wrote it."""
    with open(path, 'rb') as f:
        return pickle.load(f)


class SyntheticVideoDataset:
    """`get_video` / `num_videos` stand-in (datasets are out of scope): seeded random frames in
    [-1, 1] of the configured resolution; video i depends on (seed, i) alone."""

    def __init__(self, params, num_videos=4, video_len=12, seed=1234):
        res = params.get('resolution') if hasattr(params, 'get') else params.resolution
        self.H, self.W = (res, res) if isinstance(res, int) else tuple(res)
        self.num_videos, self.video_len, self.seed = num_videos, video_len, seed
        self.files = [f'synthetic/video_{i:05d}.mp4' for i in range(num_videos)]

    def get_video(self, i):
        if not 0 <= i < self.num_videos:
            raise IndexError(i)
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        v = (torch.randn((self.video_len, 3, self.H, self.W), generator=g) * 0.5).clamp_(-1, 1)
        return {'video': v, 'data_idx': i}


class SyntheticVideoSegDataset(SyntheticVideoDataset):
    """SyntheticVideoDataset whose videos also carry ground-truth segmentation, for the evaluation stage
    (evaluate.evaluate_video_segmentation): 'masks' [T, H, W] int64, id 0 the background and ids 1 .. num_objects
    rectangles that drift one pixel per frame (later ids cover earlier ones), a function of (seed, i) alone.  The frames
    are the parent's: the masks are unrelated to them, as random frames are to any scene."""

    def __init__(self, params, num_videos=4, video_len=12, seed=1234, num_objects=4):
        super().__init__(params, num_videos, video_len, seed)
        self.num_objects = num_objects

    def get_video(self, i):
        d = super().get_video(i)
        g = torch.Generator().manual_seed(self.seed * 7919 + 31 * i + 1)
        masks = torch.zeros((self.video_len, self.H, self.W), dtype=torch.int64)
        for k in range(1, self.num_objects + 1):
            hh = int(torch.randint(max(1, self.H // 8), max(2, self.H // 2), (1,), generator=g))
            ww = int(torch.randint(max(1, self.W // 8), max(2, self.W // 2), (1,), generator=g))
            y0 = int(torch.randint(0, self.H - hh + 1, (1,), generator=g))
            x0 = int(torch.randint(0, self.W - ww + 1, (1,), generator=g))
            dy, dx = (int(v) for v in torch.randint(-1, 2, (2,), generator=g))
            for t in range(self.video_len):
                y, x = (y0 + dy * t) % self.H, (x0 + dx * t) % self.W
                masks[t, y:y + hh, x:x + ww] = k
        d['masks'] = masks
        return d
