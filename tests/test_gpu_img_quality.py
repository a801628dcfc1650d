"""sdmi_img_quality on the GPU (metrics.image_quality): the per-frame squared error against a float64 sum, SSIM against
the oracle's scipy restatement, both against the composed path on the device, the 8-bit frames bit for bit against
np.round, the two layouts of either input, repeatability, the padding lane and the gate.

Inputs: gt = 2.4 rand - 1.2 (both ends of the clamp are used), pred = gt + 0.2 randn, seed 4321 + 1000 F + 10 H + W.

Bounds.  se: relative 1e-10 against the float64 sum of the fp32 to_rgb differences (n eps for n <= 3 * 256^2 terms is
2e-11).  ssim: |d| <= 1e-8 per frame against oracle.ssim_metric on the to_rgb images.  The oracle multiplies by 255 in
float64, the kernel and the composed path in fp32 (metrics.ssim_metric): on the CPU, for these seeds and shapes, that
moves the oracle's per-frame value by at most 9.4e-10 (measured by `python -m tests.test_gpu_img_quality`, which prints
it per shape); a separable rows-first float64 restatement agrees with scipy's filter to 2e-16, and one dropped or doubled
interior pixel moves a frame's value by 7e-6 or more.  Fused against composed on the device: |d ssim| <= 1e-9, se
relative 1e-10.

Shapes: (2, 45, 128) has three bands of 16 output rows, the last one 3 rows; (1, 15, 128) has fewer output rows (5) than
a sub-band (8); (1, 128, 128) and (1, 224, 224) have 8 and 27 bands; W = 53 is no multiple of 4 (NCHW rows are not
16-byte aligned)."""
import functools

import numpy as np
import pytest
import torch

from oracle import slotdiff_oracle as O
from slotdiffusion_amd import metrics as MT
from slotdiffusion_amd import ops
from tests.test_gpu_bwd_helpers import _end_the_session_on_a_gpu_fault, _gen  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = [(2, 11, 11), (3, 37, 53), (2, 32, 32), (2, 24, 40), (1, 27, 16), (1, 128, 128), (1, 224, 224), (2, 45, 128),
          (1, 15, 128)]
SE_RTOL, SSIM_ORACLE, SSIM_DEVICE = 1e-10, 1e-8, 1e-9


def _inputs(F, H, W):
    g = _gen(4321 + 1000 * F + 10 * H + W)
    gt = 2.4 * torch.rand(F, 3, H, W, generator=g) - 1.2
    pred = gt + 0.2 * torch.randn(F, 3, H, W, generator=g)
    return pred, gt


def _u8_ref(x):
    """The reference's saved frame (test_recon.py:94-106): np.round of the fp32 product, [F, H, W, 3]."""
    return np.round(MT.to_rgb(x).cpu().numpy() * 255.).astype(np.uint8).transpose(0, 2, 3, 1)


@functools.lru_cache(maxsize=None)
def _case(F, H, W):
    """CPU references of one shape, computed once and shared: se float64 [F], the oracle's ssim [F], the frames."""
    pred, gt = _inputs(F, H, W)
    a, b = MT.to_rgb(pred), MT.to_rgb(gt)
    se = ((a.double() - b.double()) ** 2).flatten(1).sum(1).numpy()
    ssim = np.array([O.ssim_metric(a[i:i + 1], b[i:i + 1]) for i in range(F)])
    return dict(pred=pred, gt=gt, a=a, b=b, se=se, ssim=ssim, pu8=_u8_ref(pred), gu8=_u8_ref(gt))


def _nhwc4(x, fill=0.0):
    r = ops.nchw_to_nhwc(x.contiguous(), torch.float32, 4)
    if fill != 0.0:
        r[..., 3] = fill
    return r


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.cpu().contiguous().view(torch.uint8), b.cpu().contiguous().view(torch.uint8))


@pytest.mark.parametrize('F,H,W', SHAPES)
def test_se_and_ssim_against_float64_and_the_oracle(F, H, W):
    c = _case(F, H, W)
    assert MT.img_quality_covers(H, W)
    tab, pu8, gu8 = MT.image_quality(c['pred'].cuda(), c['gt'].cuda(), fused=True)
    assert tab.shape == (F, 2) and tab.dtype == torch.float64 and tab.is_cuda and pu8 is None and gu8 is None
    t = tab.cpu().numpy()
    rel = np.abs(t[:, 0] - c['se']) / c['se']
    d = np.abs(t[:, 1] - c['ssim'])
    print(f'({F},{H},{W}): se rel {rel.max():.3e}  ssim |d| {d.max():.3e}  ssim {t[:, 1]}')
    assert rel.max() <= SE_RTOL
    assert d.max() <= SSIM_ORACLE
    assert np.all((t[:, 1] > 0.0) & (t[:, 1] < 1.0))


@pytest.mark.parametrize('F,H,W', SHAPES)
def test_fused_equals_the_composed_path_on_the_device(F, H, W):
    c = _case(F, H, W)
    pred, gt = c['pred'].cuda(), c['gt'].cuda()
    fused = MT.image_quality(pred, gt, want_u8=(True, True), fused=True)
    comp = MT.image_quality(pred, gt, want_u8=(True, True), fused=False)
    f, k = fused[0].cpu().numpy(), comp[0].cpu().numpy()
    a, b = MT.to_rgb(pred), MT.to_rgb(gt)
    se_fn, n = MT._sqerr(a, b)                                                    # the existing metric functions, per frame
    ssim_fn = np.array([MT.ssim_metric(a[i:i + 1], b[i:i + 1]) for i in range(F)])
    assert n == 3 * H * W
    d_se = max(np.abs(f[:, 0] - k[:, 0]).max() / k[:, 0].min(), (np.abs(f[:, 0] - se_fn) / se_fn).max())
    d_ss = max(np.abs(f[:, 1] - k[:, 1]).max(), np.abs(f[:, 1] - ssim_fn).max())
    print(f'({F},{H},{W}): fused vs composed  se rel {d_se:.3e}  ssim |d| {d_ss:.3e}')
    assert d_se <= SE_RTOL and d_ss <= SSIM_DEVICE
    assert torch.equal(fused[1], comp[1]) and torch.equal(fused[2], comp[2])
    # the flag and the default: inside the gate the default is the fused launch
    assert _bits_equal(MT.image_quality(pred, gt)[0], fused[0])
    old = MT._IMG_QUALITY_FUSED
    try:
        MT._IMG_QUALITY_FUSED = False
        assert _bits_equal(MT.image_quality(pred, gt)[0], comp[0])
    finally:
        MT._IMG_QUALITY_FUSED = old
    # the batch's values as the reference averages them
    vals = MT.batch_quality(fused[0].cpu(), n)
    assert abs(vals['mse'] - MT.mse_metric(a, b)) <= SE_RTOL * vals['mse']
    assert abs(vals['psnr'] - MT.psnr_metric(a, b)) <= 1e-9
    assert abs(vals['ssim'] - MT.ssim_metric(a, b)) <= SSIM_DEVICE


@pytest.mark.parametrize('F,H,W', [SHAPES[0], SHAPES[1], SHAPES[7]])
def test_identical_images(F, H, W):
    x = _case(F, H, W)['gt'].cuda()
    t = MT.image_quality(x, x.clone(), fused=True)[0].cpu().numpy()
    assert np.all(t[:, 0] == 0.0)
    assert np.abs(t[:, 1] - 1.0).max() <= 1e-9


@pytest.mark.parametrize('F,H,W', SHAPES)
def test_uint8_frames_bit_for_bit(F, H, W):
    c = _case(F, H, W)
    _, pu8, gu8 = MT.image_quality(c['pred'].cuda(), c['gt'].cuda(), want_u8=(True, True), fused=True)
    assert pu8.dtype == torch.uint8 and pu8.shape == (F, H, W, 3)
    assert np.array_equal(pu8.cpu().numpy(), c['pu8']) and np.array_equal(gu8.cpu().numpy(), c['gu8'])
    t_only, p_only, g_none = MT.image_quality(c['pred'].cuda(), c['gt'].cuda(), want_u8=(True, False), fused=True)
    assert g_none is None and torch.equal(p_only, pu8)
    t_none, none, g_only = MT.image_quality(c['pred'].cuda(), c['gt'].cuda(), want_u8=(False, True), fused=True)
    assert none is None and torch.equal(g_only, gu8) and _bits_equal(t_only, t_none)


def _half_values():
    """fp32 inputs x whose to_rgb(x) * 255.f is exactly k + 0.5: float32((k + 0.5) / 255) and its neighbours, kept where
    the fp32 product lands on the half and x = 2 a - 1 maps back to a."""
    out = []
    for k in range(255):
        a0 = np.float32((k + 0.5) / 255.0)
        for a in (np.nextafter(a0, np.float32(0)), a0, np.nextafter(a0, np.float32(1))):
            x = np.float32(a * np.float32(2) - np.float32(1))
            back = np.float32(np.float32(x * np.float32(0.5)) + np.float32(0.5))
            if back == a and np.float32(a * np.float32(255.0)) == np.float32(k + 0.5):
                out.append(x)
    return np.array(out, dtype=np.float32)


def test_uint8_rounds_half_to_even_and_clamps():
    halves = _half_values()
    prod = (MT.to_rgb(torch.from_numpy(halves)).numpy() * np.float32(255.0))
    assert len(halves) >= 100 and np.all(prod - np.floor(prod) == 0.5)
    beyond = np.array([-3.0, -1.2, -1.0000001, -1.0, 1.0, 1.0000001, 1.2, 3.0, 1e30, -1e30], dtype=np.float32)
    H, W = 16, 20
    vals = np.concatenate([halves, beyond])
    x = torch.from_numpy(np.resize(vals, 3 * H * W).reshape(1, 3, H, W).copy())
    assert int(np.sum(np.isin(x.numpy(), halves))) >= 100
    y = torch.from_numpy(np.resize(vals[::-1].copy(), 3 * H * W).reshape(1, 3, H, W).copy())
    want_x, want_y = _u8_ref(x), _u8_ref(y)
    up = np.round(prod).astype(np.int64)
    assert np.all(up % 2 == 0) and (up > prod).any() and (up < prod).any(), 'halves go to the even neighbour, both ways'
    for px, py in ((False, False), (True, False), (False, True), (True, True)):
        xin = _nhwc4(x.cuda()) if px else x.cuda()
        yin = _nhwc4(y.cuda()) if py else y.cuda()
        _, a8, b8 = MT.image_quality(xin, yin, pred_nhwc4=px, gt_nhwc4=py, want_u8=(True, True), fused=True)
        assert np.array_equal(a8.cpu().numpy(), want_x) and np.array_equal(b8.cpu().numpy(), want_y)
    assert want_x.min() == 0 and want_x.max() == 255


@pytest.mark.parametrize('F,H,W', [SHAPES[1], SHAPES[2], SHAPES[7]])
def test_layouts_repeat_and_leave_inputs_alone(F, H, W):
    c = _case(F, H, W)
    pred, gt = c['pred'].cuda(), c['gt'].cuda()
    p4, g4 = _nhwc4(pred), _nhwc4(gt)
    keep = [t.clone() for t in (pred, gt, p4, g4)]
    base = MT.image_quality(pred, gt, want_u8=(True, True), fused=True)
    again = MT.image_quality(pred, gt, want_u8=(True, True), fused=True)
    assert all(_bits_equal(a, b) for a, b in zip(base, again)), 'two runs give the same bits'
    for px, py in ((True, False), (False, True), (True, True)):
        got = MT.image_quality(p4 if px else pred, g4 if py else gt, pred_nhwc4=px, gt_nhwc4=py, want_u8=(True, True), fused=True)
        assert all(_bits_equal(a, b) for a, b in zip(base, got)), (px, py)
    for t, k in zip((pred, gt, p4, g4), keep):
        assert _bits_equal(t, k)
    # the padding lane is never read
    pn, gn = _nhwc4(pred, float('nan')), _nhwc4(gt, float('nan'))
    got = MT.image_quality(pn, gn, pred_nhwc4=True, gt_nhwc4=True, want_u8=(True, True), fused=True)
    assert all(_bits_equal(a, b) for a, b in zip(base, got))
    # an NCHW tensor that starts 4 bytes off a 16-byte boundary (the scalar-load path at W % 4 == 0)
    buf = torch.empty(pred.numel() + 1, device='cuda')
    buf[1:] = pred.flatten()
    off = buf[1:].view(pred.shape)
    assert off.data_ptr() % 16 == 4
    got = MT.image_quality(off, gt, want_u8=(True, True), fused=True)
    assert all(_bits_equal(a, b) for a, b in zip(base, got))


def test_outside_the_gate_takes_the_composed_path():
    F, H, W = 1, 20, 264
    assert not MT.img_quality_covers(H, W) and not MT.img_quality_covers(10, 32) and not MT.img_quality_covers(32, 10)
    assert MT.img_quality_covers(11, 11) and MT.img_quality_covers(4096, 256)
    c = _case(F, H, W)
    from slotdiffusion_amd import _lib
    with pytest.raises(_lib.SdmiError, match='sdmi_img_quality'):
        MT.image_quality(c['pred'].cuda(), c['gt'].cuda(), fused=True)
    tab, pu8, _ = MT.image_quality(c['pred'].cuda(), _nhwc4(c['gt'].cuda()), gt_nhwc4=True, want_u8=(True, False))
    t = tab.cpu().numpy()
    assert (np.abs(t[:, 0] - c['se']) / c['se']).max() <= SE_RTOL
    assert np.abs(t[:, 1] - c['ssim']).max() <= SSIM_ORACLE
    assert np.array_equal(pu8.cpu().numpy(), c['pu8'])


if __name__ == '__main__':                  # the docstring's CPU figure: what the fp32 `* 255` moves the oracle's value by
    worst = 0.0
    for F, H, W in SHAPES + [(1, 20, 264)]:
        c = _case(F, H, W)
        a255, b255 = (c['a'] * 255.0).double() / 255.0, (c['b'] * 255.0).double() / 255.0
        moved = max(abs(O.ssim_metric(a255[i:i + 1], b255[i:i + 1]) - c['ssim'][i]) for i in range(F))
        worst = max(worst, moved)
        print(f'({F},{H},{W}): fp32 x255 moves the oracle by {moved:.3e}')
    print(f'max {worst:.3e};  exact halves: {len(_half_values())}')
