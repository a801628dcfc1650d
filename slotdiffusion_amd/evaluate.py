"""From a checkpoint to the segmentation table: FG-ARI / mIoU / mBO as the reference's img_based/test_seg.py:19-101 and
video_based/test_seg.py:17-113 print them.

    res = evaluate_image_segmentation(model, batches)                          # batches: dicts as the val loader's
    res = evaluate_video_segmentation(model, dataset, batch_size=4)            # dataset: num_videos / get_video(i)
    for k, v in res['metrics'].items(): print(f'{k}: {v * 100.:.2f}')

Every score is a function of the per-sample contingency table alone (metrics.py), so nothing else is kept.  For the models
whose masks are Slot Attention's attention map (SADiffusion, SAViDiffusion) no mask, upsampled or not, and no id map is
written: sdmi_seg_tables turns the low-resolution map into table counts on the device (metrics.seg_tables; the composed
path outside its gate).  A video is walked in chunks like extract.extract_video_slots, slots and the LSTM wrapper's state
carried over, one table per video over all its frames: T is folded into the pixel axis (video_based/test_seg.py:25-30),
so an object must keep its slot over time.  SA and SAVi produce full-resolution masks in their decoder: those go through
argmax and sdmi_contingency inside the same drivers.

Averaging is the reference's: the metric of a batch (the float32 mean of ARI / FG-ARI over the batch, the nanmean of the
others) enters an AverageMeter with weight B (test_seg.py:91-95).  ONE DIFFERENCE: a batch whose value is NaN (every
ground truth of the batch holds the background id alone) is left out of that metric's average and counted in
`nan_batches`; the reference's meter would print NaN from that batch on.
"""
import numpy as np
import torch

from . import metrics as MT

__all__ = ['evaluate_image_segmentation', 'evaluate_video_segmentation', 'image_tables', 'stream_chunk_tables']

_KEY = {'ARI': 'ari', 'fARI': 'fari', 'miou': 'miou', 'fmiou': 'fmiou', 'mbo': 'mbo'}
REPORTED = ('fARI', 'miou', 'mbo')            # the three the paper reports (test_seg.py:31-37)


class _Meter:
    """nerv.utils.AverageMeter's update(value, n) / avg, with NaN values left out and counted."""

    def __init__(self):
        self.sum, self.count, self.nan = 0.0, 0, 0

    def update(self, val, n):
        if np.isnan(val):
            self.nan += 1
            return
        self.sum += float(val) * n
        self.count += n

    @property
    def avg(self):
        return self.sum / self.count if self.count else float('nan')


class _Results:
    def __init__(self, names):
        self.names = tuple(names)
        assert all(n in _KEY for n in self.names), f'metrics are among {sorted(_KEY)}'
        self.meters, self.per_sample, self.tables = {}, {}, []

    def add_batch(self, tables, prefix=''):
        """tables: int [B, Kg + 1, N] of one batch -> the batch's values into the meters, the per-sample values kept."""
        keys = tuple(_KEY[n] for n in self.names)
        per = MT.scores_from_tables(tables, keys)
        vals = MT.batch_scores(None, keys, per_sample=per)
        for n in self.names:
            self.meters.setdefault(prefix + n, _Meter()).update(vals[_KEY[n]], tables.shape[0])
            self.per_sample.setdefault(prefix + n, []).append(np.asarray(per[_KEY[n]], dtype=np.float64))

    def result(self):
        return {'metrics': {k: m.avg for k, m in self.meters.items()},
                'nan_batches': {k: m.nan for k, m in self.meters.items()},
                'per_sample': {k: np.concatenate(v) for k, v in self.per_sample.items()},
                'tables': self.tables}


def _decoder_masks(model):
    """SA / SAVi: the masks are the decoder's alpha masks (test_seg.py:66-69); every other model's are the attention map."""
    from . import models
    return isinstance(model, models.SA)


def _ids32(x, device):
    return torch.as_tensor(x).to(device=device, dtype=torch.int32)


@torch.no_grad()
def image_tables(model, batch, num_true):
    """One batch of the image loader -> int32 tables [B, maps, Kg + 1, N] on the device (maps: 'masks', then 'sem_masks'
    when the batch has them; row Kg: the pixels of 'inst_overlap_masks')."""
    from . import engine
    device = getattr(model, 'device', 'cpu')
    img = batch['img'].to(device)
    B, _, H, W = img.shape
    gt = _ids32(batch['masks'], device).view(B, 1, H, W)
    gt2 = _ids32(batch['sem_masks'], device).view(B, 1, H, W) if 'sem_masks' in batch else None
    ov = batch.get('inst_overlap_masks')
    ov = _ids32(ov, device).view(B, 1, H, W) if ov is not None else None
    if _decoder_masks(model):
        pm = model({'img': img})['masks']                     # [B, N, 1, H, W]
        N = pm.shape[1]
        pred = pm.squeeze(-3).argmax(dim=-3).view(B, 1, H, W)
        tabs = []
        for m in (gt, gt2):
            if m is not None:
                rows = m if ov is None else torch.where(ov != 0, torch.full_like(m, num_true), m)
                tabs.append(MT.contingency(rows, pred, num_true + 1, N))
        return torch.stack(tabs, 1)
    K = model.K()
    tok = engine.encoder_out(K, model._to_nhwc(img), model.rplan)
    _, seg = engine.slot_attention(K, tok, model.init_latents[0], model.num_iterations, model.eps)
    return MT.seg_tables(seg, gt, model.visual_resolution, num_true, gt2=gt2, overlap=ov)


@torch.no_grad()
def evaluate_image_segmentation(model, batches, metrics=REPORTED, tables_fn=None):
    """img_based/test_seg.py:45-101.  batches: an iterable of dicts {'img' [B, 3, H, W], 'masks' [B, H, W] integer ids
    (0 = background)} and optionally 'inst_overlap_masks' [B, H, W] (0 / 1) and 'sem_masks' [B, H, W] (COCO / VOC: every
    batch is then scored twice, against the instance and the semantic masks, test_seg.py:79-89, reported as 'inst/<m>'
    and 'sem/<m>'; the plain '<m>' otherwise).  metrics: names among ARI, fARI, miou, fmiou, mbo.
    -> {'metrics': {name: B-weighted average of the per-batch values}, 'nan_batches': {name: batches left out because
    their value was NaN (module docstring)}, 'per_sample': {name: float array over all images},
    'tables': [int tensor [B, maps, Kg + 1, N] per batch]}.  tables_fn(model, batch, num_true) replaces image_tables."""
    model.eval()
    res = _Results(metrics)
    fn = tables_fn or image_tables
    for batch in batches:
        two = 'sem_masks' in batch
        num_true = int(torch.as_tensor(batch['masks']).max()) + 1
        if two:
            num_true = max(num_true, int(torch.as_tensor(batch['sem_masks']).max()) + 1)
        tabs = fn(model, batch, num_true).cpu()
        res.tables.append(tabs)
        res.add_batch(tabs[:, 0], 'inst/' if two else '')
        if two:
            res.add_batch(tabs[:, 1], 'sem/')
    return res.result()


@torch.no_grad()
def stream_chunk_tables(model, chunk, prev_slots, gt, counts, num_true):
    """One chunk [B, Tc, 3, H, W] of a batch of videos -> (its last slots, counts [B, 1, Kg + 1, N] with the chunk's
    pixels added; counts None: a new table).  gt int32 [B, Tc, H, W] on the device (a slice of the whole video's)."""
    B, Tc = chunk.shape[:2]
    if _decoder_masks(model):
        slots = model.encode_stream(chunk, prev_slots)
        masks = model.decode(slots.flatten(0, 1))[2]                           # [B * Tc, N, 1, H, W]
        pred = masks.squeeze(-3).argmax(dim=-3).view(B, Tc, *masks.shape[-2:])
        add = MT.contingency(gt, pred, num_true + 1, masks.shape[1]).unsqueeze(1)
        counts = add if counts is None else counts.add_(add)
    else:
        slots, seg = model.encode_stream(chunk, prev_slots, want_seg=True)   # seg [Tc, B, h*w, N]
        counts = MT.seg_tables(seg.flatten(0, 1), gt, model.visual_resolution, num_true, time_major=True, counts=counts)
    return slots[:, -1], counts


@torch.no_grad()
def evaluate_video_segmentation(model, dataset, batch_size=1, chunk_len=None, seq_len=-1, metrics=REPORTED,
                                chunk_tables_fn=None):
    """video_based/test_seg.py:44-113 on whole videos.  dataset: `num_videos` and `get_video(i) -> {'video' [T, 3, H, W],
    'masks' [T, H, W] integer ids}` (one T per batch of videos).  Per batch of `batch_size` videos the clip is walked in
    chunks of `chunk_len` frames (default model.clip_len) as extract.extract_video_slots walks it: chunk k + 1 starts
    from the last slots of chunk k, only the first chunk of a video resets the model's PredictorState, and every chunk
    adds to the ONE table of its video, so the result does not depend on chunk_len.  seq_len > 0 evaluates the first
    seq_len frames (the reference's --seq_len).  Returns what evaluate_image_segmentation returns, tables
    [B, 1, Kg + 1, N] per batch.  chunk_tables_fn replaces stream_chunk_tables."""
    model.eval()
    chunk_len = int(chunk_len or model.clip_len)
    assert chunk_len >= 1 and batch_size >= 1
    device = getattr(model, 'device', 'cpu')
    res = _Results(metrics)
    fn = chunk_tables_fn or stream_chunk_tables
    for start in range(0, dataset.num_videos, batch_size):
        items = [dataset.get_video(i) for i in range(start, min(start + batch_size, dataset.num_videos))]
        video = torch.stack([torch.as_tensor(d['video']) for d in items]).float()          # [B, T, 3, H, W]
        masks = torch.stack([torch.as_tensor(d['masks']) for d in items])                  # [B, T, H, W]
        if seq_len > 0:
            video, masks = video[:, :seq_len], masks[:, :seq_len]
        num_true = int(masks.max()) + 1
        gt = masks.to(device=device, dtype=torch.int32).contiguous()
        prev, counts = None, None
        for t0 in range(0, video.shape[1], chunk_len):
            prev, counts = fn(model, video[:, t0:t0 + chunk_len].to(device), prev, gt[:, t0:t0 + chunk_len], counts,
                              num_true)
        tabs = counts.cpu()
        res.tables.append(tabs)
        res.add_batch(tabs[:, 0])
    return res.result()
