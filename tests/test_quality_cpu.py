"""The image-quality stage, host side: the four drivers of slotdiffusion_amd/quality.py on a stub model with a torch
restatement of the scoring tail passed through quality_fn= -- chunk walking and that a video's result does not depend on
chunk_len (exact on the stub), B-weighted averaging, the files each script writes, resume, the seed + data_idx[0] noise,
the prediction driver's history_len slicing, compositional generation's slot shift against the oracle, the lpips_fn hook
-- and the argument refusals of sdmi_img_quality.  No GPU."""
import os
import pickle
import types

import numpy as np
import pytest
import torch

from oracle import slotdiff_oracle as O
from slotdiffusion_amd import _lib, extract, quality
from slotdiffusion_amd import metrics as MT

H = W = 12
N = 3
SHARE = (0.5, 0.3, 0.2)


def torch_quality(pred, gt, pred_nhwc4=False, want_u8=(False, False)):
    """metrics.image_quality restated on the CPU: float64 squared error of the fp32 to_rgb images, the oracle's SSIM, the
    reference's np.round frames."""
    if pred_nhwc4:
        pred = pred[..., :3].permute(0, 3, 1, 2)
    a, b = MT.to_rgb(pred.float()), MT.to_rgb(gt.float())
    se = ((a.double() - b.double()) ** 2).flatten(1).sum(1)
    ssim = torch.tensor([O.ssim_metric(a[i:i + 1], b[i:i + 1]) for i in range(a.shape[0])], dtype=torch.float64)
    u8 = [torch.from_numpy(np.round(t.numpy() * 255.).astype(np.uint8).transpose(0, 2, 3, 1).copy()) if w else None
          for t, w in zip((a, b), want_u8)]
    return torch.stack([se, ssim], 1), u8[0], u8[1]


class _Stub:
    """A 'diffusion' model whose slots are shares of the frame itself: slot i = SHARE[i] * frame, decoding adds the slots
    up and 0.1 * x_T on top, as NHWC-4 rows with a NaN padding lane.  It is its own dm_decoder."""
    clip_len = 4
    latent_res = (H, W)
    history_len, rollout_len = 2, 3

    def __init__(self):
        self.dm_decoder = self
        self.stream, self.samples, self.forwards, self.rollouts, self.evals = [], [], 0, [], 0

    def eval(self):
        self.evals += 1
        return self

    @staticmethod
    def slots_of(frames):
        flat = frames.flatten(1)
        return torch.stack([s * flat for s in SHARE], 1)                          # [F, N, 3 * H * W]

    @staticmethod
    def frames_of(slots):
        return slots.sum(1).view(-1, 3, H, W)

    def __call__(self, data):
        self.forwards += 1
        return {'slots': self.slots_of(data['img'])}

    def encode_stream(self, chunk, prev=None):
        B, Tc = chunk.shape[:2]
        self.stream.append((B, Tc, None if prev is None else prev.clone(), chunk[:, :, 0, 0, 0].clone()))
        return self.slots_of(chunk.flatten(0, 1)).view(B, Tc, N, -1)

    def sample_rows(self, batch, use_dpm=False, x_T=None, **kw):
        assert use_dpm is True
        self.samples.append((x_T.clone(), dict(kw)))
        img = self.frames_of(batch['slots']) + 0.1 * x_T
        rows = torch.cat([img.permute(0, 2, 3, 1), torch.full(img.shape[:1] + (H, W, 1), float('nan'))], -1)
        return rows.contiguous(), True

    def rollout(self, past, pred_len):
        self.rollouts.append((past.clone(), pred_len))
        return torch.stack([past[:, -1] * (0.9 ** (k + 1)) for k in range(pred_len)], 1)


def _ds(num_videos=3, video_len=7, seed=5):
    return extract.SyntheticVideoDataset(types.SimpleNamespace(resolution=(H, W)), num_videos=num_videos, video_len=video_len,
                                         seed=seed)


def _dec(frames):
    """What the stub decodes from the slots of `frames` (the shares add up to the frame only to fp32 rounding)."""
    return _Stub.frames_of(_Stub.slots_of(frames))


def _noise(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _pngs(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith('.png'))


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


# ----------------------------------------------------------------------------------------------------------------------
# videos
# ----------------------------------------------------------------------------------------------------------------------
def test_video_driver_walks_chunks_carries_slots_and_does_not_depend_on_chunk_len():
    ds = _ds()
    m = _Stub()
    res = quality.evaluate_video_reconstruction(m, ds, batch_size=2, chunk_len=3, seed=11, quality_fn=torch_quality,
                                                keep_frames=True)
    assert m.evals == 1
    assert [(B, Tc) for B, Tc, *_ in m.stream] == [(2, 3), (2, 3), (2, 1), (1, 3), (1, 3), (1, 1)]
    assert [c[2] is None for c in m.stream] == [True, False, False, True, False, False]
    v0 = torch.stack([ds.get_video(i)['video'] for i in range(2)])
    assert torch.equal(m.stream[1][2], _Stub.slots_of(v0[:, 2])), 'the last slots of a chunk start the next one'
    assert torch.equal(torch.cat([c[3] for c in m.stream[3:]], 1)[0], ds.get_video(2)['video'][:, 0, 0, 0])
    # ONE x_T per batch of videos (seed + data_idx[0]), repeated over the frames of every chunk
    x0, x2 = _noise(11 + 0, (1, 3, H, W)), _noise(11 + 2, (1, 3, H, W))
    assert [s[0].shape[0] for s in m.samples] == [6, 6, 2, 3, 3, 1]
    for s, x in zip(m.samples, (x0, x0, x0, x2, x2, x2)):
        assert torch.equal(s[0], x.expand_as(s[0]))
    # the numbers: per batch the reference's values over its B * T frames in [B][T] order, averaged with weight B
    vals = []
    for vids, x in (([0, 1], x0), ([2], x2)):
        gt = torch.stack([ds.get_video(i)['video'] for i in vids]).flatten(0, 1)
        tab, p8, g8 = torch_quality(_dec(gt) + 0.1 * x, gt, want_u8=(True, True))
        vals.append((MT.batch_quality(tab, 3 * H * W), tab, p8, g8))
    for k in ('mse', 'psnr', 'ssim'):
        assert abs(res['metrics'][k] - (2 * vals[0][0][k] + 1 * vals[1][0][k]) / 3) <= 1e-12, k
        assert res['batches'][0][k] == vals[0][0][k] and res['batches'][1][k] == vals[1][0][k]
    assert set(res['metrics']) == {'mse', 'psnr', 'ssim'}
    assert [b['data_idx'] for b in res['batches']] == [[0, 1], [2]]
    assert np.array_equal(res['per_frame']['se'], torch.cat([vals[0][1], vals[1][1]])[:, 0].numpy())
    assert res['per_frame']['ssim'].shape == (21,)
    assert torch.equal(res['frames'][0][0], vals[0][2].view(2, 7, H, W, 3)) and torch.equal(res['frames'][1][1], vals[1][3].view(1, 7, H, W, 3))
    for cl in (1, 7, 4, None):
        m2 = _Stub()
        r2 = quality.evaluate_video_reconstruction(m2, ds, batch_size=2, chunk_len=cl, seed=11, quality_fn=torch_quality)
        assert r2['metrics'] == res['metrics'] and r2['batches'] == res['batches'], cl
        assert np.array_equal(r2['per_frame']['se'], res['per_frame']['se'])
        assert 'frames' not in r2
        if cl is None:
            assert [(B, Tc) for B, Tc, *_ in m2.stream] == [(2, 4), (2, 3), (1, 4), (1, 3)]          # default: model.clip_len
    m3 = _Stub()
    r3 = quality.evaluate_video_reconstruction(m3, ds, batch_size=3, chunk_len=2, seq_len=5, seed=11, quality_fn=torch_quality)
    assert [(B, Tc) for B, Tc, *_ in m3.stream] == [(3, 2), (3, 2), (3, 1)] and r3['per_frame']['se'].shape == (15,)


def test_video_driver_files_resume_and_sampler_keywords(tmp_path):
    ds = _ds()
    m = _Stub()
    d = str(tmp_path / 'eval')
    res = quality.evaluate_video_reconstruction(m, ds, batch_size=2, chunk_len=3, save_dir=d, seed=3, quality_fn=torch_quality,
                                                dpm_steps=4, dpm_order=2)
    assert all(s[1] == {'dpm_steps': 4, 'dpm_order': 2} for s in m.samples)
    # video_based/test_recon.py saves the metrics and no frames
    assert sorted(os.listdir(d)) == ['metrics']
    assert sorted(f for f in os.listdir(os.path.join(d, 'metrics')) if f.endswith('.pkl')) == ['0_metric.pkl', '2_metric.pkl']
    with open(os.path.join(d, 'metrics', '0_metric.pkl'), 'rb') as f:
        saved = pickle.load(f)
    assert set(saved) == {'mse', 'psnr', 'ssim'} and all(type(v) is float for v in saved.values())
    assert saved['ssim'] == res['batches'][0]['ssim']
    # resume: nothing is computed, the result is the same
    m2 = _Stub()
    again = quality.evaluate_video_reconstruction(m2, ds, batch_size=2, chunk_len=3, save_dir=d, seed=3, quality_fn=torch_quality)
    assert m2.stream == [] and m2.samples == []
    assert again['metrics'] == res['metrics'] and again['batches'] == res['batches']
    assert np.array_equal(again['per_frame']['ssim'], res['per_frame']['ssim'])
    # a missing batch alone is recomputed, and what is loaded is what the file holds
    os.remove(os.path.join(d, 'metrics', '2_metric.pkl'))
    with open(os.path.join(d, 'metrics', '0_metric.pkl'), 'wb') as f:
        pickle.dump(dict(saved, mse=123.0), f)
    m3 = _Stub()
    part = quality.evaluate_video_reconstruction(m3, ds, batch_size=2, chunk_len=3, save_dir=d, seed=3, quality_fn=torch_quality)
    assert [(B, Tc) for B, Tc, *_ in m3.stream] == [(1, 3), (1, 3), (1, 1)]
    assert part['batches'][0]['mse'] == 123.0 and part['batches'][1] == res['batches'][1], 'seed + data_idx[0]: a resumed run agrees'
    # save_frames: the frames of both sides, <idx>/<t>.png
    d2 = str(tmp_path / 'eval2')
    full = quality.evaluate_video_reconstruction(_Stub(), ds, batch_size=2, chunk_len=3, save_dir=d2, seed=3,
                                                 quality_fn=torch_quality, save_frames=True, keep_frames=True)
    want = sorted(f'{s}/{i}/{t}.png' for s in ('recon_vids', 'gt_vids') for i in range(3) for t in range(7))
    assert _pngs(d2) == want
    assert np.array_equal(_read_png(os.path.join(d2, 'recon_vids', '1', '4.png')), full['frames'][0][0][1, 4].numpy())
    assert np.array_equal(_read_png(os.path.join(d2, 'gt_vids', '2', '6.png')), full['frames'][1][1][0, 6].numpy())
    with pytest.raises(AssertionError):
        quality.evaluate_video_reconstruction(_Stub(), ds, save_frames=True, quality_fn=torch_quality)


# ----------------------------------------------------------------------------------------------------------------------
# images
# ----------------------------------------------------------------------------------------------------------------------
def _img_batches():
    g = torch.Generator().manual_seed(8)
    imgs = (torch.rand(5, 3, H, W, generator=g) * 2.4 - 1.2)
    return imgs, [dict(img=imgs[:3], data_idx=torch.tensor([40, 41, 42])), dict(img=imgs[3:], data_idx=torch.tensor([7, 9]))]


def test_image_reconstruction_driver(tmp_path):
    imgs, batches = _img_batches()
    m = _Stub()
    d = str(tmp_path / 'eval')
    seen = []

    def lp(pred, gt):
        seen.append((pred.shape, gt.shape))
        return 0.25 * pred.shape[0]
    res = quality.evaluate_image_reconstruction(m, batches, save_dir=d, seed=100, lpips_fn=lp, quality_fn=torch_quality)
    assert m.forwards == 2 and [s[0].shape for s in m.samples] == [(3, 3, H, W), (2, 3, H, W)]
    xs = [_noise(100 + 40, (3, 3, H, W)), _noise(100 + 7, (2, 3, H, W))]          # every image its own noise
    assert torch.equal(m.samples[0][0], xs[0]) and torch.equal(m.samples[1][0], xs[1])
    vals = []
    for b, x in zip(batches, xs):
        tab, p8, g8 = torch_quality(_dec(b['img']) + 0.1 * x, b['img'], want_u8=(True, True))
        vals.append((MT.batch_quality(tab, 3 * H * W), p8, g8))
    for k in ('mse', 'psnr', 'ssim'):
        assert abs(res['metrics'][k] - (3 * vals[0][0][k] + 2 * vals[1][0][k]) / 5) <= 1e-12
    assert seen == [((3, 3, H, W), (3, 3, H, W)), ((2, 3, H, W), (2, 3, H, W))], 'the hook gets NCHW images'
    assert abs(res['metrics']['lpips'] - (3 * 0.75 + 2 * 0.5) / 5) <= 1e-12
    assert sorted(f for f in os.listdir(os.path.join(d, 'metrics')) if f.endswith('.pkl')) == ['40_metric.pkl', '7_metric.pkl']
    assert _pngs(d) == sorted(f'{s}/{i}.png' for s in ('recon_imgs', 'gt_imgs') for i in (40, 41, 42, 7, 9))
    assert np.array_equal(_read_png(os.path.join(d, 'recon_imgs', '41.png')), vals[0][1][1].numpy())
    assert np.array_equal(_read_png(os.path.join(d, 'gt_imgs', '9.png')), vals[1][2][1].numpy())
    with open(os.path.join(d, 'metrics', '7_metric.pkl'), 'rb') as f:
        assert set(pickle.load(f)) == {'mse', 'psnr', 'ssim', 'lpips'}
    m2 = _Stub()
    again = quality.evaluate_image_reconstruction(m2, batches, save_dir=d, seed=100, lpips_fn=lp, quality_fn=torch_quality)
    assert m2.forwards == 0 and m2.samples == [] and again['metrics'] == res['metrics'] and len(seen) == 2
    # without data_idx: the running sample index; without save_dir: nothing is written, no frames are asked for
    asked = []

    def q(pred, gt, pred_nhwc4=False, want_u8=(False, False)):
        asked.append(tuple(want_u8))
        return torch_quality(pred, gt, pred_nhwc4, want_u8)
    plain = quality.evaluate_image_reconstruction(_Stub(), [dict(img=b['img']) for b in batches], seed=100, quality_fn=q)
    assert [b['data_idx'] for b in plain['batches']] == [[0, 1, 2], [3, 4]] and asked == [(False, False)] * 2
    assert 'lpips' not in plain['metrics']


def test_compositional_generation_shifts_slots_as_the_oracle(tmp_path):
    imgs, batches = _img_batches()
    m = _Stub()
    d = str(tmp_path / 'comp')
    res = quality.evaluate_compositional_generation(m, batches, d, seed=1, quality_fn=torch_quality)
    assert res['metrics'] == {'mse': 0.0} and [b['mse'] for b in res['batches']] == [0.0, 0.0]
    with open(os.path.join(d, 'metrics', '40_metric.pkl'), 'rb') as f:
        assert pickle.load(f) == {'mse': 0.0}
    assert _pngs(d) == sorted(f'{s}/{i}.png' for s in ('comp_imgs', 'gt_imgs') for i in (40, 41, 42, 7, 9))
    x = _noise(1 + 40, (3, 3, H, W))                                             # the image side: no same_noise
    assert torch.equal(m.samples[0][0], x)
    mixed = _Stub.frames_of(O.shuffle_slots(_Stub.slots_of(imgs[:3]))) + 0.1 * x
    _, p8, g8 = torch_quality(mixed, imgs[:3], want_u8=(True, True))
    assert not torch.equal(p8, torch_quality(_dec(imgs[:3]) + 0.1 * x, imgs[:3], want_u8=(True, False))[1]), 'the shift changes the frames'
    for j, i in enumerate((40, 41, 42)):
        assert np.array_equal(_read_png(os.path.join(d, 'comp_imgs', f'{i}.png')), p8[j].numpy())
        assert np.array_equal(_read_png(os.path.join(d, 'gt_imgs', f'{i}.png')), g8[j].numpy())
    # the video side: one x_T for all frames of the batch, comp_vids / gt_vids
    ds = _ds(num_videos=3, video_len=5)
    m2 = _Stub()
    d2 = str(tmp_path / 'compv')
    quality.evaluate_compositional_generation(m2, ds, d2, batch_size=3, chunk_len=2, seed=1, quality_fn=torch_quality)
    assert [(B, Tc) for B, Tc, *_ in m2.stream] == [(3, 2), (3, 2), (3, 1)]
    x1 = _noise(1 + 0, (1, 3, H, W))
    assert all(torch.equal(s[0], x1.expand_as(s[0])) for s in m2.samples) and [s[0].shape[0] for s in m2.samples] == [6, 6, 3]
    assert _pngs(d2) == sorted(f'{s}/{i}/{t}.png' for s in ('comp_vids', 'gt_vids') for i in range(3) for t in range(5))
    video = torch.stack([ds.get_video(i)['video'] for i in range(3)])
    slots = O.shuffle_slots(_Stub.slots_of(video.flatten(0, 1)).view(3, 5, N, -1))
    want = torch_quality(_Stub.frames_of(slots.flatten(0, 1)) + 0.1 * x1, video.flatten(0, 1), want_u8=(True, True))
    assert np.array_equal(_read_png(os.path.join(d2, 'comp_vids', '1', '3.png')), want[1].view(3, 5, H, W, 3)[1, 3].numpy())
    assert np.array_equal(_read_png(os.path.join(d2, 'gt_vids', '2', '4.png')), want[2].view(3, 5, H, W, 3)[2, 4].numpy())
    m3 = _Stub()
    quality.evaluate_compositional_generation(m3, ds, d2, batch_size=3, chunk_len=2, seed=1, quality_fn=torch_quality)
    assert m3.stream == [] and m3.samples == []


def test_video_prediction_rolls_out_from_the_history(tmp_path):
    g = torch.Generator().manual_seed(21)
    B, T = 2, _Stub.history_len + _Stub.rollout_len
    img = torch.rand(B, T, 3, H, W, generator=g) * 2 - 1
    slots = _Stub.slots_of(img.flatten(0, 1)).view(B, T, N, -1)
    m = _Stub()
    d = str(tmp_path / 'vp')
    res = quality.evaluate_video_prediction(m, [dict(img=img, slots=slots, data_idx=torch.tensor([5, 6]))], save_dir=d, seed=9,
                                            quality_fn=torch_quality, dpm_steps=3)
    assert len(m.rollouts) == 1 and m.rollouts[0][1] == 3 and torch.equal(m.rollouts[0][0], slots[:, :2])
    x = _noise(9 + 5, (B * 3, 3, H, W))                                           # every frame its own noise: no same_noise
    assert torch.equal(m.samples[0][0], x) and m.samples[0][1] == {'dpm_steps': 3}
    pred = _Stub.frames_of(torch.stack([slots[:, 1] * (0.9 ** (k + 1)) for k in range(3)], 1).flatten(0, 1)) + 0.1 * x
    tab, p8, g8 = torch_quality(pred, img[:, 2:].flatten(0, 1), want_u8=(True, True))
    want = MT.batch_quality(tab, 3 * H * W)
    assert all(abs(res['metrics'][k] - want[k]) <= 1e-12 for k in want) and res['per_frame']['se'].shape == (6,)
    assert _pngs(d) == sorted(f'{s}/{i}/{t}.png' for s in ('pred_vids', 'gt_vids') for i in (5, 6) for t in range(3))
    assert np.array_equal(_read_png(os.path.join(d, 'pred_vids', '6', '2.png')), p8.view(B, 3, H, W, 3)[1, 2].numpy())
    assert np.array_equal(_read_png(os.path.join(d, 'gt_vids', '5', '0.png')), g8.view(B, 3, H, W, 3)[0, 0].numpy())


def test_unseeded_noise_is_drawn_from_the_global_generator():
    _, batches = _img_batches()
    m = _Stub()
    torch.manual_seed(77)
    quality.evaluate_image_reconstruction(m, batches[:1], quality_fn=torch_quality)
    torch.manual_seed(77)
    assert torch.equal(m.samples[0][0], torch.randn(3, 3, H, W))


# ----------------------------------------------------------------------------------------------------------------------
# the entry point refuses bad arguments before any launch; the gate and its band split
# ----------------------------------------------------------------------------------------------------------------------
def test_img_quality_rejects_bad_arguments_without_launch():
    ok = dict(pred=64, gt=128, partial=192, pred_u8=256, gt_u8=320, F=2, H=32, W=32, pred_nhwc4=1, gt_nhwc4=0,
              nbands=MT.img_quality_bands(32, 32)[1])
    bad = [dict(pred=0), dict(gt=0), dict(partial=0),                                 # null pointers
           dict(F=0), dict(F=-1), dict(H=10), dict(W=10), dict(W=257), dict(W=264), dict(H=0),
           dict(pred_nhwc4=2), dict(gt_nhwc4=-1), dict(nbands=0), dict(nbands=2),
           dict(pred=68), dict(gt=130), dict(partial=196)]                            # NHWC-4 rows off 16 bytes, fp32 / fp64 alignment
    for over in bad:
        with pytest.raises(_lib.SdmiError, match='sdmi_img_quality'):
            _lib.call('sdmi_img_quality', None, **dict(ok, **over))
        assert b'sdmi_img_quality' in _lib.lib().sdmi_last_error(), over


@pytest.mark.parametrize('hw,covers,bands', [((11, 11), True, (8, 1)), ((32, 32), True, (24, 1)), ((128, 128), True, (16, 8)),
                                             ((224, 224), True, (8, 27)), ((45, 128), True, (16, 3)), ((15, 128), True, (8, 1)),
                                             ((4096, 256), True, (8, 511)), ((20, 264), False, None), ((10, 64), False, None),
                                             ((64, 10), False, None)])
def test_img_quality_gate_and_band_split(hw, covers, bands):
    assert MT.img_quality_covers(*hw) is covers
    if covers:
        assert MT.img_quality_bands(*hw) == bands
