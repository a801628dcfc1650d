"""The image-quality stage on the GPU (slotdiffusion_amd/quality.py): every driver against the composed computation --
the model's own encode / log_images / decode, then the existing metric functions (mse_metric's sdmi_sqerr_rows,
ssim_metric's sdmi_ssim) and np.round for the frames -- on the tiny 32 x 32 video models, the CLEVRTex SADiffusion, the
plain SA auto-encoder and the LDMSlotFormer of the other GPU tests, with 2 - 4 sampler steps.  The frames are compared
bit for bit, the metrics within 1e-9; resume is checked through the C-ABI call log; one bf16 run is a smoke test."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import slotdiff_oracle as O
from slotdiffusion_amd import _lib, extract, quality
from slotdiffusion_amd import metrics as MT
from tests.test_gpu_bwd_helpers import _end_the_session_on_a_gpu_fault  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-9
SEED = 17


def _noise(idx0, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(SEED + idx0)).cuda()


def _u8(x):
    """The reference's saved frames (test_recon.py:94-106) of NCHW images in [-1, 1] -> uint8 [F, H, W, 3]."""
    return np.round(MT.to_rgb(x).cpu().numpy() * 255.).astype(np.uint8).transpose(0, 2, 3, 1)


def _composed(pred, gt):
    """NCHW frames -> (the batch's values, se [F], ssim [F]) on the existing metric functions, frame by frame."""
    a, b = MT.to_rgb(pred.float()), MT.to_rgb(gt.float())
    se, n = MT._sqerr(a, b)
    ssim = np.array([MT.ssim_metric(a[i:i + 1], b[i:i + 1]) for i in range(a.shape[0])])
    vals = {'mse': float(se.mean()), 'psnr': float(np.mean(10.0 * np.log10(1.0 / (se / n)))), 'ssim': float(ssim.mean())}
    assert abs(vals['mse'] - MT.mse_metric(a, b)) <= TOL and abs(vals['psnr'] - MT.psnr_metric(a, b)) <= TOL
    return vals, se, ssim


def _agree(res, vals, se, ssim):
    for k in ('mse', 'psnr', 'ssim'):
        assert abs(res['metrics'][k] - vals[k]) <= TOL, (k, res['metrics'][k], vals[k])
    assert np.abs(res['per_frame']['se'] - se).max() <= TOL and np.abs(res['per_frame']['ssim'] - ssim).max() <= TOL
    assert np.isfinite(vals['psnr']) and np.all(np.abs(ssim) <= 1.0)


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _calls_logged(path, fn):
    """The C-ABI calls `fn` makes, by entry point, through the call log."""
    _lib.set_call_log(path)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        _lib.set_call_log(None)
    with open(path) as f:
        return out, [line.split('\t')[0] for line in f if line.strip()]


def _video_ds(n=2, T=6):
    return extract.SyntheticVideoDataset(types.SimpleNamespace(resolution=(32, 32)), num_videos=n, video_len=T, seed=3)


def _video_reference(m, ds, chunk_len, steps):
    """encode_stream + dm_decoder.log_images(x_T=...) at the same chunk length, NCHW samples of the whole batch."""
    video = torch.stack([ds.get_video(i)['video'] for i in range(ds.num_videos)]).cuda()
    B, T = video.shape[:2]
    x1 = _noise(0, (1, 3) + tuple(m.latent_res))
    prev, out = None, []
    for t0 in range(0, T, chunk_len):
        chunk = video[:, t0:t0 + chunk_len]
        slots = m.encode_stream(chunk, prev)
        prev = slots[:, -1]
        Tc = chunk.shape[1]
        s = m.dm_decoder.log_images({'slots': slots.flatten(0, 1).contiguous()}, use_dpm=True, x_T=x1.repeat(B * Tc, 1, 1, 1),
                                    dpm_steps=steps)['samples']
        out.append(s.view(B, Tc, 3, 32, 32))
    return torch.cat(out, 1).flatten(0, 1), video.flatten(0, 1)


@pytest.mark.parametrize('chunk_len', [2, 3])
def test_video_reconstruction_equals_the_composed_tail_fp32(chunk_len, tmp_path):
    from tests.test_gpu_pred_tf import _model
    m = _model('SAViDiffusion', False, torch.float32)
    ds = _video_ds()
    d = str(tmp_path / 'eval')
    res, calls = _calls_logged(str(tmp_path / 'calls0.txt'), lambda: quality.evaluate_video_reconstruction(
        m, ds, batch_size=2, chunk_len=chunk_len, save_dir=d, seed=SEED, save_frames=True, keep_frames=True, dpm_steps=3))
    assert calls.count('sdmi_img_quality') == 6 // chunk_len and 'sdmi_ssim' not in calls and 'sdmi_sqerr_rows' not in calls
    pred, gt = _video_reference(m, ds, chunk_len, 3)
    vals, se, ssim = _composed(pred, gt)
    print(f'chunk_len {chunk_len}: {vals};  d ssim {np.abs(res["per_frame"]["ssim"] - ssim).max():.3e}  '
          f'd se {np.abs(res["per_frame"]["se"] - se).max():.3e}')
    _agree(res, vals, se, ssim)
    assert res['per_frame']['se'].shape == (12,) and len(res['batches']) == 1 and res['batches'][0]['data_idx'] == [0, 1]
    pu8, gu8 = res['frames'][0]
    assert pu8.shape == (2, 6, 32, 32, 3) and pu8.dtype == torch.uint8
    assert np.array_equal(pu8.flatten(0, 1).numpy(), _u8(pred)) and np.array_equal(gu8.flatten(0, 1).numpy(), _u8(gt))
    assert len(np.unique(pu8.numpy())) > 8, 'the samples are not constant'
    # the composed tail through the same driver (the module flag): the same frames, the same numbers
    old = MT._IMG_QUALITY_FUSED
    try:
        MT._IMG_QUALITY_FUSED = False
        off = quality.evaluate_video_reconstruction(m, ds, batch_size=2, chunk_len=chunk_len, seed=SEED, keep_frames=True,
                                                    dpm_steps=3)
    finally:
        MT._IMG_QUALITY_FUSED = old
    _agree(off, vals, se, ssim)
    assert torch.equal(off['frames'][0][0], pu8) and torch.equal(off['frames'][0][1], gu8)
    # files: the PNGs read back are the uint8 tensors
    for sub, t8 in (('recon_vids', pu8), ('gt_vids', gu8)):
        for i in range(2):
            assert sorted(os.listdir(os.path.join(d, sub, str(i)))) == sorted(f'{t}.png' for t in range(6))
            for t in range(6):
                assert np.array_equal(_read_png(os.path.join(d, sub, str(i), f'{t}.png')), t8[i, t].numpy())
    # resume: a second call with the same save_dir computes nothing and returns the same result
    again, calls = _calls_logged(str(tmp_path / 'calls1.txt'), lambda: quality.evaluate_video_reconstruction(
        m, ds, batch_size=2, chunk_len=chunk_len, save_dir=d, seed=SEED, dpm_steps=3))
    assert calls == []
    assert again['metrics'] == res['metrics'] and again['batches'] == res['batches']
    assert np.array_equal(again['per_frame']['se'], res['per_frame']['se'])


def test_video_reconstruction_of_a_decoder_model_fp32():
    from tests.test_gpu_pred_tf import _model
    m = _model('SAVi', False, torch.float32)
    ds = _video_ds()
    video = torch.stack([ds.get_video(i)['video'] for i in range(2)]).cuda()
    for cl in (2, 3):
        res = quality.evaluate_video_reconstruction(m, ds, batch_size=2, chunk_len=cl, keep_frames=True)
        prev, out = None, []                      # the stream at the same chunk length (its transition is the fused one)
        for t0 in range(0, 6, cl):
            slots = m.encode_stream(video[:, t0:t0 + cl], prev)
            prev = slots[:, -1]
            out.append(m.decode(slots.flatten(0, 1))[0].view(2, cl, 3, 32, 32))
        pred = torch.cat(out, 1).flatten(0, 1)
        vals, se, ssim = _composed(pred, video.flatten(0, 1))
        _agree(res, vals, se, ssim)
        assert np.array_equal(res['frames'][0][0].flatten(0, 1).numpy(), _u8(pred))


def test_video_reconstruction_bf16_smoke():
    from tests.test_gpu_pred_tf import _model
    m = _model('SAViDiffusion', False, torch.bfloat16)
    res = quality.evaluate_video_reconstruction(m, _video_ds(), batch_size=2, chunk_len=3, seed=SEED, keep_frames=True, dpm_steps=3)
    assert res['per_frame']['se'].shape == (12,) and res['per_frame']['ssim'].shape == (12,)
    assert res['frames'][0][0].shape == (2, 6, 32, 32, 3)
    assert np.all(np.isfinite(res['per_frame']['se'])) and all(np.isfinite(v) for v in res['metrics'].values())
    assert 0.0 <= res['metrics']['ssim'] <= 1.0 and np.all(np.abs(res['per_frame']['ssim']) <= 1.0)


def test_image_reconstruction_of_sadiffusion_fp32(tmp_path):
    from tests.test_gpu_model import ctx
    m, _, img = ctx()
    B, _, H, W = img.shape
    d = str(tmp_path / 'eval')
    batch = dict(img=img.cpu(), data_idx=torch.tensor([30 + i for i in range(B)]))
    res = quality.evaluate_image_reconstruction(m, [batch], save_dir=d, seed=SEED, dpm_steps=3)
    x = _noise(30, (B, 3) + tuple(m.latent_res))
    pred = m({'img': img}, log_images=True, use_dpm=True, x_T=x, dpm_steps=3)['samples']
    vals, se, ssim = _composed(pred, img)
    _agree(res, vals, se, ssim)
    want_p, want_g = _u8(pred), _u8(img)
    for j in range(B):
        assert np.array_equal(_read_png(os.path.join(d, 'recon_imgs', f'{30 + j}.png')), want_p[j])
        assert np.array_equal(_read_png(os.path.join(d, 'gt_imgs', f'{30 + j}.png')), want_g[j])
    assert os.path.exists(os.path.join(d, 'metrics', '30_metric.pkl'))
    hook = quality.evaluate_image_reconstruction(m, [batch], seed=SEED, dpm_steps=3,
                                                 lpips_fn=lambda p, g: float((p - g).abs().mean()))
    assert abs(hook['metrics']['lpips'] - float((pred - img).abs().mean())) <= 1e-6 and hook['metrics']['ssim'] == res['metrics']['ssim']


def test_compositional_generation_samples_the_shifted_slots_fp32(tmp_path):
    from tests.test_gpu_model import ctx
    m, _, img = ctx()
    B = img.shape[0]
    d = str(tmp_path / 'comp')
    res = quality.evaluate_compositional_generation(m, [dict(img=img.cpu())], d, seed=SEED, dpm_steps=3)
    assert res['metrics'] == {'mse': 0.0}
    slots = m({'img': img})['slots']
    mixed = O.shuffle_slots(slots)
    assert not torch.equal(mixed, slots)
    x = _noise(0, (B, 3) + tuple(m.latent_res))
    pred = m.dm_decoder.log_images({'slots': mixed}, use_dpm=True, x_T=x, dpm_steps=3)['samples']
    want_p, want_g = _u8(pred), _u8(img)
    for j in range(B):
        assert np.array_equal(_read_png(os.path.join(d, 'comp_imgs', f'{j}.png')), want_p[j])
        assert np.array_equal(_read_png(os.path.join(d, 'gt_imgs', f'{j}.png')), want_g[j])


def test_image_reconstruction_of_the_plain_autoencoder_fp32():
    from tests import common as C
    from tests.test_gpu_model import _plain_sa
    m = _plain_sa(torch.float32).eval()
    img = C.make_inputs(2)[0].cuda()
    res = quality.evaluate_image_reconstruction(m, [dict(img=img.cpu())])
    pred = m({'img': img})['recon_img']
    vals, se, ssim = _composed(pred, img)
    _agree(res, vals, se, ssim)
    assert res['batches'][0]['data_idx'] == [0, 1]


def test_video_prediction_on_ldmslotformer_bf16(tmp_path):
    from tests import common as C
    from tests import slotformer_ref as R
    from tests.test_gpu_slotformer import _mode
    m = R.gpu_model(decoder=True)
    slots = C.load_golden('ldmslotformer_b2.npz')['slots']
    B, T = slots.shape[:2]
    assert T == m.history_len + m.rollout_len
    img = (torch.randn(B, T, 3, 128, 128, generator=torch.Generator().manual_seed(6)) * 0.5).clamp(-1, 1)
    P = m.rollout_len
    d = str(tmp_path / 'vp')
    with _mode(m, 'bf16', graph=False):
        res = quality.evaluate_video_prediction(m, [dict(img=img, slots=slots, data_idx=torch.tensor([4, 5]))], save_dir=d,
                                                seed=SEED, dpm_steps=2)
        pred_slots = m.rollout(slots[:, :m.history_len].cuda(), P)
        x = _noise(4, (B * P, 3) + tuple(m.latent_res))
        pred = m.log_images({'slots': pred_slots.flatten(0, 1)}, use_dpm=True, x_T=x, dpm_steps=2)['samples']
        torch.cuda.synchronize()
    gt = img[:, m.history_len:].flatten(0, 1).cuda()
    vals, se, ssim = _composed(pred, gt)
    _agree(res, vals, se, ssim)
    assert res['per_frame']['se'].shape == (B * P,)
    want_p, want_g = _u8(pred).reshape(B, P, 128, 128, 3), _u8(gt).reshape(B, P, 128, 128, 3)
    for j, i in enumerate((4, 5)):
        assert sorted(os.listdir(os.path.join(d, 'pred_vids', str(i)))) == sorted(f'{t}.png' for t in range(P))
        for t in range(P):
            assert np.array_equal(_read_png(os.path.join(d, 'pred_vids', str(i), f'{t}.png')), want_p[j, t])
            assert np.array_equal(_read_png(os.path.join(d, 'gt_vids', str(i), f'{t}.png')), want_g[j, t])
