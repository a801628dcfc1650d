"""From a checkpoint to the reconstruction / generation / video-prediction tables: MSE, PSNR and SSIM and the saved
frames as the reference's img_based/test_recon.py:24-107, video_based/test_recon.py:24-115, both test_comp_gen.py
(19-98) and vp_vqa/test_vp.py:24-107 produce them.

    res = evaluate_image_reconstruction(model, batches, save_dir='eval')         # batches: dicts as the val loader's
    res = evaluate_video_reconstruction(model, dataset, batch_size=1)            # dataset: num_videos / get_video(i)
    res = evaluate_compositional_generation(model, batches_or_dataset, 'eval')
    res = evaluate_video_prediction(slotformer, batches, save_dir='eval')
    for k, v in res['metrics'].items(): print(f'{k}: {v:.4f}')

All four share one shape: get slots (encode, shift across the batch, or roll out), sample frames with DPM-Solver++ and
decode them, score them against the ground truth, write a per-batch metrics pickle and the frames as 8-bit PNGs for
FID / FVD.  The scoring tail is metrics.image_quality: one sdmi_img_quality launch per batch of frames reads the
decoder's NHWC-4 rows and the loader's NCHW images once and gives the per-frame squared error, SSIM and the 8-bit
frames; ONE device-to-host copy of the [F, 2] table per batch.  A video is walked in chunks as
evaluate.evaluate_video_segmentation walks it, slots and predictor state carried over.

Averaging is the reference's: the value of a batch (mse: mean over its frames of the squared error summed over a frame;
psnr: mean over frames of 10 log10(1 / (se / n)); ssim: mean over frames) enters an AverageMeter with weight B.

save_dir is the reference's layout: metrics/{data_idx[0]}_metric.pkl (a pickled dict of floats) and the frames under
recon_imgs/<idx>.png, gt_imgs/, recon_vids/<idx>/<t>.png, gt_vids/, pred_vids/, comp_imgs/, comp_vids/, by each script's
own rules (video_based/test_recon.py saves no frames: save_frames=True asks for them).  Beside the pickle the per-frame
table is kept as metrics/{data_idx[0]}_frames.npy.  A batch whose metric file exists is loaded and not recomputed: the
reference's resume.  data_idx comes from the batch ('data_idx'), otherwise it is the running sample index.

seed: the x_T of a batch is drawn on the host from a generator seeded with seed + data_idx[0], so a resumed run and a
fresh one agree; seed=None draws from torch's global generator on the device, like the reference.

LPIPS is NOT built (no VGG weights offline): lpips_fn, an optional callable (pred, gt) -> float on NCHW fp32 images in
[-1, 1], adds the 'lpips' key when given.  FID / FVD read the saved frames with their own tools.  Not built either: the
mp4 visualisation (--save_video), the STEVE / SLATE branches, DataParallel.

The dpm_* / unipc_* keywords of LDM.generate_imgs pass through every driver.
"""
import os
import pickle

import numpy as np
import torch

from . import metrics as MT
from .evaluate import _Meter

__all__ = ['evaluate_image_reconstruction', 'evaluate_video_reconstruction', 'evaluate_compositional_generation',
           'evaluate_video_prediction', 'score_frames']


def score_frames(pred, gt, pred_nhwc4=False, want_u8=(False, False)):
    """The scoring tail: (pred rows, gt NCHW) -> (device fp64 table [F, 2] of (se, ssim), pred_u8, gt_u8).  The drivers'
    quality_fn hook replaces it."""
    return MT.image_quality(pred, gt, pred_nhwc4=pred_nhwc4, want_u8=want_u8)


# ----------------------------------------------------------------------------------------------------------------------
# bookkeeping shared by the drivers
# ----------------------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, save_dir, seed, lpips_fn, quality_fn):
        self.save_dir, self.seed, self.lpips_fn = save_dir, seed, lpips_fn
        self.score = quality_fn or score_frames
        self.meters, self.per_frame, self.batches, self.seen = {}, {'se': [], 'ssim': []}, [], 0

    def data_idx(self, given, B):
        """The batch's 'data_idx' as ints, otherwise the running sample index."""
        if given is None:
            idx = list(range(self.seen, self.seen + B))
        else:
            idx = [int(i) for i in torch.as_tensor(given).reshape(-1).tolist()]
            assert len(idx) == B, 'one data_idx per sample'
        self.seen += B
        return idx

    def metric_file(self, idx0):
        return os.path.join(self.save_dir, 'metrics', f'{idx0}_metric.pkl') if self.save_dir else None

    def resumed(self, idx, B):
        """The reference's resume: a batch whose metric file exists is loaded, not recomputed."""
        fn = self.metric_file(idx[0])
        if fn is None or not os.path.exists(fn):
            return False
        with open(fn, 'rb') as f:
            vals = pickle.load(f)
        frames = fn[:-len('_metric.pkl')] + '_frames.npy'
        self.add(idx, B, vals, np.load(frames) if os.path.exists(frames) else None, write=False)
        return True

    def noise(self, idx0, shape, device):
        if self.seed is None:
            return torch.randn(shape, device=device)
        g = torch.Generator().manual_seed(int(self.seed) + int(idx0))
        return torch.randn(shape, generator=g).to(device)

    def add(self, idx, B, vals, table=None, write=True):
        vals = {k: float(v) for k, v in vals.items()}
        for k, v in vals.items():
            self.meters.setdefault(k, _Meter()).update(v, B)
        if table is not None:
            self.per_frame['se'].append(np.asarray(table[:, 0], dtype=np.float64))
            self.per_frame['ssim'].append(np.asarray(table[:, 1], dtype=np.float64))
        self.batches.append(dict(vals, data_idx=list(idx)))
        fn = self.metric_file(idx[0])
        if write and fn is not None:
            os.makedirs(os.path.dirname(fn), exist_ok=True)
            with open(fn, 'wb') as f:
                pickle.dump(vals, f)
            if table is not None:
                np.save(fn[:-len('_metric.pkl')] + '_frames.npy', np.asarray(table, dtype=np.float64))

    def values(self, table, n, pred=None, gt=None):
        """The batch's floats from the host copy of its table (+ 'lpips' through the hook)."""
        vals = MT.batch_quality(table, n)
        if self.lpips_fn is not None:
            vals['lpips'] = float(self.lpips_fn(pred, gt))
        return vals

    def result(self):
        return {'metrics': {k: m.avg for k, m in self.meters.items()},
                'per_frame': {k: (np.concatenate(v) if v else np.zeros((0,))) for k, v in self.per_frame.items()},
                'batches': self.batches}


def _image_writer():
    try:
        from PIL import Image
    except ImportError as e:                                                       # pragma: no cover
        raise RuntimeError('saving frames needs PIL (Pillow); metrics alone do not: call without save_dir / '
                           'save_frames') from e
    return Image


def _save_images(save_dir, sub, idx, u8):
    """u8 [B, H, W, 3] -> <save_dir>/<sub>/<idx>.png"""
    Image = _image_writer()
    d = os.path.join(save_dir, sub)
    os.makedirs(d, exist_ok=True)
    for i, a in zip(idx, u8.cpu().numpy()):
        Image.fromarray(a).save(os.path.join(d, f'{i}.png'))


def _save_videos(save_dir, sub, idx, u8):
    """u8 [B, T, H, W, 3] -> <save_dir>/<sub>/<idx>/<t>.png"""
    Image = _image_writer()
    for i, vid in zip(idx, u8.cpu().numpy()):
        d = os.path.join(save_dir, sub, str(i))
        os.makedirs(d, exist_ok=True)
        for t, a in enumerate(vid):
            Image.fromarray(a).save(os.path.join(d, f'{t}.png'))


def _decoder_model(model):
    """SA / SAVi decode slots with their own decoder; every other model samples from its dm_decoder."""
    from . import models
    return isinstance(model, models.SA)


def _as_nchw(rows, nhwc4):
    """The frames as the lpips_fn hook takes them (only built when the hook is given)."""
    return rows[..., :3].permute(0, 3, 1, 2).contiguous() if nhwc4 else rows


def _sample(model, slots, x_T, sampler):
    """Flattened slots [F, N, D] -> (frames, nhwc4): DPM-Solver++ from x_T, decoded, as the decoder leaves them."""
    return model.dm_decoder.sample_rows({'slots': slots}, use_dpm=True, x_T=x_T, **sampler)


def _latent_shape(model):
    h, w = model.latent_res
    return 3, int(h), int(w)


# ----------------------------------------------------------------------------------------------------------------------
# images
# ----------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def evaluate_image_reconstruction(model, batches, save_dir=None, seed=None, lpips_fn=None, quality_fn=None, **sampler):
    """img_based/test_recon.py:24-107.  batches: an iterable of dicts {'img' [B, 3, H, W] in [-1, 1]} and optionally
    'data_idx' [B].  SA: the frames are model(data)['recon_img']; SADiffusion: the slots sampled with use_dpm=True.
    save_dir: metrics/<idx0>_metric.pkl, recon_imgs/<idx>.png, gt_imgs/<idx>.png.
    -> {'metrics': {'mse', 'psnr', 'ssim' (, 'lpips')}: B-weighted averages of the per-batch values, 'per_frame':
    {'se', 'ssim'} float64 over all frames (of a resumed batch: from its _frames.npy), 'batches': the per-batch dicts}."""
    model.eval()
    device = getattr(model, 'device', 'cpu')
    run = _Run(save_dir, seed, lpips_fn, quality_fn)
    for batch in batches:
        img = torch.as_tensor(batch['img']).float()
        B, _, H, W = img.shape
        idx = run.data_idx(batch.get('data_idx'), B)
        if run.resumed(idx, B):
            continue
        img = img.to(device).contiguous()
        if _decoder_model(model):
            pred, nhwc4 = model({'img': img})['recon_img'], False
        else:
            slots = model({'img': img})['slots']
            pred, nhwc4 = _sample(model, slots, run.noise(idx[0], (B,) + _latent_shape(model), device), sampler)
        save = save_dir is not None
        table, pu8, gu8 = run.score(pred, img, nhwc4, (save, save))
        host = table.cpu()
        vals = run.values(host, 3 * H * W, *((_as_nchw(pred, nhwc4), img) if lpips_fn is not None else ()))
        run.add(idx, B, vals, host.numpy())
        if save:
            _save_images(save_dir, 'recon_imgs', idx, pu8)
            _save_images(save_dir, 'gt_imgs', idx, gu8)
    return run.result()


# ----------------------------------------------------------------------------------------------------------------------
# videos
# ----------------------------------------------------------------------------------------------------------------------
def _video_batches(dataset, batch_size, seq_len):
    for start in range(0, dataset.num_videos, batch_size):
        items = [dataset.get_video(i) for i in range(start, min(start + batch_size, dataset.num_videos))]
        video = torch.stack([torch.as_tensor(d['video']) for d in items]).float()            # [B, T, 3, H, W]
        if seq_len > 0:
            video = video[:, :seq_len]
        given = [d['data_idx'] for d in items] if all('data_idx' in d for d in items) else None
        yield video, given


@torch.no_grad()
def evaluate_video_reconstruction(model, dataset, batch_size=1, chunk_len=None, save_dir=None, seq_len=-1, seed=None,
                                  lpips_fn=None, quality_fn=None, save_frames=False, keep_frames=False, **sampler):
    """video_based/test_recon.py:24-115 on whole videos.  dataset: `num_videos` and `get_video(i) -> {'video' [T, 3, H, W]
    in [-1, 1]}` (+ 'data_idx'; one T per batch of videos).  Per batch of `batch_size` videos the clip is walked in
    chunks of `chunk_len` frames (default model.clip_len) exactly as evaluate.evaluate_video_segmentation walks it: chunk
    k + 1 starts from the last slots of chunk k, only the first chunk of a video resets the model's PredictorState.  ONE
    x_T [1, 3, h, w] per batch of videos is repeated over all of its frames and passed to every chunk: the reference's
    same_noise=True over the flattened B * T frames.  SAVi decodes with its own decoder.  The batch's values are taken
    over its B * T frames, [B][T] order, from one host copy of the table.
    save_dir: metrics/<idx0>_metric.pkl and, as in the reference, NO frames; save_frames=True also writes
    recon_vids/<idx>/<t>.png and gt_vids/<idx>/<t>.png.  keep_frames=True returns them: 'frames': [(pred_u8, gt_u8)
    uint8 [B, T, H, W, 3] on the host, per computed batch].  -> as evaluate_image_reconstruction."""
    model.eval()
    chunk_len = int(chunk_len or model.clip_len)
    assert chunk_len >= 1 and batch_size >= 1
    assert not save_frames or save_dir is not None, 'save_frames needs save_dir'
    device = getattr(model, 'device', 'cpu')
    run = _Run(save_dir, seed, lpips_fn, quality_fn)
    frames = []
    u8 = bool(save_frames or keep_frames)
    for video, given in _video_batches(dataset, batch_size, seq_len):
        B, T, _, H, W = video.shape
        idx = run.data_idx(given, B)
        if run.resumed(idx, B):
            continue
        x1 = None if _decoder_model(model) else run.noise(idx[0], (1,) + _latent_shape(model), device)
        prev, tabs, pu, gu, lp = None, [], [], [], []
        for t0 in range(0, T, chunk_len):
            chunk = video[:, t0:t0 + chunk_len].to(device)
            Tc = chunk.shape[1]
            slots = model.encode_stream(chunk, prev)                              # [B, Tc, N, D]
            prev = slots[:, -1]
            if _decoder_model(model):
                pred, nhwc4 = model.decode(slots.flatten(0, 1))[0], False
            else:
                pred, nhwc4 = _sample(model, slots.flatten(0, 1).contiguous(), x1.repeat(B * Tc, 1, 1, 1), sampler)
            gt = chunk.flatten(0, 1).contiguous()
            tab, p8, g8 = run.score(pred, gt, nhwc4, (u8, u8))
            tabs.append(tab.view(B, Tc, 2))
            if u8:
                pu.append(p8.view(B, Tc, H, W, 3))
                gu.append(g8.view(B, Tc, H, W, 3))
            if lpips_fn is not None:
                lp.append(_as_nchw(pred, nhwc4).view(B, Tc, 3, H, W))
        host = torch.cat(tabs, 1).flatten(0, 1).cpu()                              # [B * T, 2], the batch's one copy
        vals = run.values(host, 3 * H * W, *((torch.cat(lp, 1).flatten(0, 1), video.flatten(0, 1).to(device))
                                              if lpips_fn is not None else ()))
        run.add(idx, B, vals, host.numpy())
        if u8:
            pu, gu = torch.cat(pu, 1), torch.cat(gu, 1)
            if save_frames:
                _save_videos(save_dir, 'recon_vids', idx, pu)
                _save_videos(save_dir, 'gt_vids', idx, gu)
            if keep_frames:
                frames.append((pu.cpu(), gu.cpu()))
    res = run.result()
    if keep_frames:
        res['frames'] = frames
    return res


@torch.no_grad()
def evaluate_compositional_generation(model, data, save_dir, batch_size=1, chunk_len=None, seq_len=-1, seed=None,
                                      quality_fn=None, **sampler):
    """Both test_comp_gen.py (19-98): slot i of every sample is taken from the sample i places further along the batch
    (metrics.shuffle_slots), the mixed slots are decoded, and the frames are saved for FID / FVD.  No metric is
    computed: the result of a batch is the reference's {'mse': 0.} pickle.
    data: an iterable of image batches {'img' [B, 3, H, W]} -> comp_imgs/<idx>.png, gt_imgs/<idx>.png, every sample
    with its own x_T; or a video dataset (`get_video`) -> comp_vids/<idx>/<t>.png, gt_vids/<idx>/<t>.png, batches of
    `batch_size` videos encoded and decoded in chunks of `chunk_len` frames with ONE x_T for all frames of the batch
    (same_noise on the video side only, as the reference does).  SA / SAVi decode with their own decoder."""
    model.eval()
    device = getattr(model, 'device', 'cpu')
    run = _Run(save_dir, seed, None, quality_fn)
    assert save_dir is not None, 'compositional generation only produces files'
    if hasattr(data, 'get_video'):
        chunk_len = int(chunk_len or model.clip_len)
        for video, given in _video_batches(data, batch_size, seq_len):
            B, T, _, H, W = video.shape
            idx = run.data_idx(given, B)
            if run.resumed(idx, B):
                continue
            prev, slots = None, []
            for t0 in range(0, T, chunk_len):
                slots.append(model.encode_stream(video[:, t0:t0 + chunk_len].to(device), prev))
                prev = slots[-1][:, -1]
            slots = MT.shuffle_slots(torch.cat(slots, 1))                         # [B, T, N, D]
            x1 = None if _decoder_model(model) else run.noise(idx[0], (1,) + _latent_shape(model), device)
            pu, gu = [], []
            for t0 in range(0, T, chunk_len):
                s = slots[:, t0:t0 + chunk_len].flatten(0, 1).contiguous()
                Tc = s.shape[0] // B
                if _decoder_model(model):
                    pred, nhwc4 = model.decode(s)[0], False
                else:
                    pred, nhwc4 = _sample(model, s, x1.repeat(B * Tc, 1, 1, 1), sampler)
                _, p8, g8 = run.score(pred, video[:, t0:t0 + chunk_len].flatten(0, 1).to(device).contiguous(), nhwc4, (True, True))
                pu.append(p8.view(B, Tc, H, W, 3))
                gu.append(g8.view(B, Tc, H, W, 3))
            run.add(idx, B, {'mse': 0.})
            _save_videos(save_dir, 'comp_vids', idx, torch.cat(pu, 1))
            _save_videos(save_dir, 'gt_vids', idx, torch.cat(gu, 1))
        return run.result()
    for batch in data:
        img = torch.as_tensor(batch['img']).float()
        B = img.shape[0]
        idx = run.data_idx(batch.get('data_idx'), B)
        if run.resumed(idx, B):
            continue
        img = img.to(device).contiguous()
        slots = MT.shuffle_slots(model({'img': img})['slots'])
        if _decoder_model(model):
            pred, nhwc4 = model.decode(slots)[0], False
        else:
            pred, nhwc4 = _sample(model, slots, run.noise(idx[0], (B,) + _latent_shape(model), device), sampler)
        _, p8, g8 = run.score(pred, img, nhwc4, (True, True))
        run.add(idx, B, {'mse': 0.})
        _save_images(save_dir, 'comp_imgs', idx, p8)
        _save_images(save_dir, 'gt_imgs', idx, g8)
    return run.result()


@torch.no_grad()
def evaluate_video_prediction(model, batches, save_dir=None, seed=None, lpips_fn=None, quality_fn=None, **sampler):
    """vp_vqa/test_vp.py:24-107 on an LDMSlotFormer.  batches: dicts {'img' [B, T, 3, H, W], 'slots' [B, T, N, D]} (+
    'data_idx') with T = history_len + rollout_len.  The slots of the first history_len frames are rolled out
    (model.rollout(slots[:, :history_len], rollout_len)), the predicted slots are sampled with use_dpm=True, every frame
    with its own x_T (no same_noise), and scored against img[:, history_len:].
    save_dir: metrics/<idx0>_metric.pkl, pred_vids/<idx>/<t>.png, gt_vids/<idx>/<t>.png.
    -> as evaluate_image_reconstruction."""
    model.eval()
    device = getattr(model, 'device', 'cpu')
    run = _Run(save_dir, seed, lpips_fn, quality_fn)
    for batch in batches:
        img = torch.as_tensor(batch['img']).float()
        B = img.shape[0]
        idx = run.data_idx(batch.get('data_idx'), B)
        if run.resumed(idx, B):
            continue
        gt = img[:, model.history_len:].to(device)
        P, H, W = gt.shape[1], gt.shape[3], gt.shape[4]
        past = torch.as_tensor(batch['slots'])[:, :model.history_len].to(device).float()
        pred_slots = model.rollout(past, model.rollout_len)                          # [B, P, N, D]
        assert pred_slots.shape[1] == P, 'img holds history_len + rollout_len frames'
        pred, nhwc4 = _sample(model, pred_slots.flatten(0, 1).contiguous(),
                              run.noise(idx[0], (B * P,) + _latent_shape(model), device), sampler)
        gtf = gt.flatten(0, 1).contiguous()
        save = save_dir is not None
        table, pu8, gu8 = run.score(pred, gtf, nhwc4, (save, save))
        host = table.cpu()
        vals = run.values(host, 3 * H * W, *((_as_nchw(pred, nhwc4), gtf) if lpips_fn is not None else ()))
        run.add(idx, B, vals, host.numpy())
        if save:
            _save_videos(save_dir, 'pred_vids', idx, pu8.view(B, P, H, W, 3))
            _save_videos(save_dir, 'gt_vids', idx, gu8.view(B, P, H, W, 3))
    return run.result()
