"""sdmi_slot_panel on the GPU: the fused panel against vis.slot_panel_composed on the same device (whose masks and argmax
are sdmi_mask_upsample_argmax's), byte for byte, at the smallest shapes that reach each hazard -- a non-square integer
ratio (a transposition shows), a non-integer ratio, planar masks with per-slot images at odd sizes (unaligned store
edges), a height of two row bands, the image (G = F) and the video (G = 1) form, every recon layout, the id source
inside and outside its range; soft and hard from one launch against two; a sentinel around a strided sub-rectangle; and
operands on which every product is exact, against integer arithmetic."""
import numpy as np
import pytest
import torch

from slotdiffusion_amd import ops, vis

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _rand(shape, seed, lo=-1.2, hi=1.2):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).to(DEV)


def _seg(F, h, w, N, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.softmax(torch.randn(F, h * w, N, generator=g) * 2, -1).to(DEV)


def _both(img, **kw):
    """(fused, composed) of one call; with hard=True each is a pair."""
    got = vis.slot_panel(img, fused=True, **kw)
    ref = vis.slot_panel(img, fused=False, **kw)
    torch.cuda.synchronize()
    return got, ref


def _same(got, ref):
    if isinstance(got, tuple):
        return all(_same(a, b) for a, b in zip(got, ref))
    return got.dtype == torch.uint8 and got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize('hw', [(4, 6), (5, 7)])
@pytest.mark.parametrize('G', [3, 1])
@pytest.mark.parametrize('recon', [None, 'nchw', 'nhwc4'])
def test_attention_map_panel_equals_composed(hw, G, recon):
    F, N, H, W = 3, 5, 16, 24
    assert vis.slot_panel_band(N, 4, H, W, *hw) < H, 'the height spans at least two row bands'
    img = _rand((F, 3, H, W), 1)
    seg = _seg(F, hw[0], hw[1], N, 2)
    kw = dict(seg=seg, hw=hw, G=G, hard=True, tiles=('img', 'color', 'overlay'))
    if recon == 'nchw':
        kw.update(recon=_rand((F, 3, H, W), 3), tiles=('img', 'recon', 'color', 'overlay'))
    elif recon == 'nhwc4':
        kw.update(recon=_rand((F, H, W, 4), 3), recon_nhwc4=True, tiles=('img', 'recon', 'color', 'overlay'))
    got, ref = _both(img, **kw)
    I, GH, GW = vis.panel_geometry(F, N, len(kw['tiles']), H, W, G)
    assert got[0].shape == (I, 3, GH, GW) and I == F // G
    assert _same(got, ref)
    assert not torch.equal(got[0], got[1])                     # soft masks are not one-hot


def test_nhwc4_image_and_gt_tile():
    F, N, H, W = 3, 5, 16, 24
    rows = _rand((F, H, W, 4), 4)
    gt = torch.randint(0, 20, (F, H, W), generator=torch.Generator().manual_seed(5)).to(DEV)
    gt[0, 0, 0], gt[1, 3, 4] = 20, -3                           # outside the palette: byte 0
    got, ref = _both(rows, img_nhwc4=True, seg=_seg(F, 4, 6, N, 6), hw=(4, 6), gt=gt, G=3,
                     tiles=('img', 'gtcolor', 'color', 'overlay'))
    assert _same(got, ref)
    assert (got[0, :, 2, 2 + (W + 2)] == 0).all() and (got[0, :, (H + 2) + 2 + 3, 2 + (W + 2) + 4] == 0).all()


@pytest.mark.parametrize('G', [3, 1])
def test_planar_masks_with_slot_images_at_odd_sizes(G):
    F, N, H, W = 3, 3, 11, 13
    img = _rand((F, 3, H, W), 7)
    masks = _seg(F, H, W, N, 8).permute(0, 2, 1).reshape(F, N, H, W).contiguous()
    slot_img = _rand((F, N, 3, H, W), 9)
    recon = _rand((F, 3, H, W), 10)
    got, ref = _both(img, masks=masks, slot_img=slot_img, recon=recon, G=G, hard=True,
                     tiles=('img', 'recon', 'color', 'overlay'))
    assert _same(got, ref)
    got, ref = _both(img, masks=masks, slot_img=slot_img, recon=recon, G=G, tiles=('img', 'recon'))
    assert _same(got, ref)


@pytest.mark.parametrize('G', [3, 1])
def test_id_source_inside_and_outside_its_range(G):
    F, N, H, W = 3, 20, 16, 24
    img = _rand((F, 3, H, W), 11)
    ids = torch.randint(0, N, (F, H, W), generator=torch.Generator().manual_seed(12)).to(DEV)
    got, ref = _both(img, ids=ids, num_classes=N, G=G, tiles=('img', 'color', 'overlay'))
    assert _same(got, ref)
    bad = ids.clone()
    bad[0, 0, 0], bad[1, 5, 7], bad[2, 15, 23] = N, -1, 1 << 20
    got, ref = _both(img, ids=bad, num_classes=N, G=G, hard=True, tiles=('img', 'color', 'overlay'))
    assert _same(got, ref) and torch.equal(got[0], got[1])      # an id map is one-hot already
    pic, row = 0, 2                                            # frame 0, pixel (0, 0) in either form
    assert (got[0][pic, :, row, 2 + (W + 2)] == 0).all()        # colour tile: byte 0
    for k in range(N):                                          # no slot tile owns the pixel: white
        assert (got[0][pic, :, row, 2 + (3 + k) * (W + 2)] == 255).all()


def test_soft_and_hard_of_one_launch_equal_two_launches():
    F, N, H, W, hw = 3, 5, 16, 24, (5, 7)
    img = _rand((F, 3, H, W), 13)
    seg = _seg(F, hw[0], hw[1], N, 14)
    soft, hard = vis.slot_panel(img, seg=seg, hw=hw, hard=True, fused=True)
    alone = vis.slot_panel(img, seg=seg, hw=hw, fused=True)
    _, idx = ops.mask_upsample_argmax(seg, hw[0], hw[1], H, W, want_up=False)
    onehot = torch.nn.functional.one_hot(idx, N).permute(0, 3, 1, 2).float().contiguous()
    hard2 = vis.slot_panel(img, masks=onehot, fused=True)
    assert torch.equal(soft, alone) and torch.equal(hard, hard2)


@pytest.mark.parametrize('sentinel', [0xAA, 0x55])
def test_sentinel_around_a_strided_sub_rectangle(sentinel):
    """Two videos' panels as bands of rows inside a wider, taller picture: every byte of the rectangles is written, none
    outside them (the second sentinel value rules out a byte that only happens to equal the first)."""
    F, N, H, W, hw = 3, 5, 16, 24, (4, 6)
    _, GH, GW = vis.panel_geometry(F, N, 3, H, W, 1)
    big = torch.full((F, 3, 3 + 2 * GH + 5, GW + 7), sentinel, dtype=torch.uint8, device=DEV)
    hbig = big.clone()
    want = []
    for v in range(2):
        img, seg = _rand((F, 3, H, W), 20 + v), _seg(F, hw[0], hw[1], N, 30 + v)
        y0 = 3 + v * GH
        view = lambda b: b[:, :, y0:y0 + GH, 3:3 + GW]            # noqa: E731  (odd offsets: unaligned rows)
        vis.slot_panel(img, seg=seg, hw=hw, hard=True, fused=True, out=(view(big), view(hbig)))
        want.append(vis.slot_panel(img, seg=seg, hw=hw, hard=True, fused=False))
    torch.cuda.synchronize()
    inside = torch.zeros_like(big, dtype=torch.bool)
    inside[:, :, 3:3 + 2 * GH, 3:3 + GW] = True
    for b, k in ((big, 0), (hbig, 1)):
        assert (b[~inside] == sentinel).all()
        assert torch.equal(b[:, :, 3:3 + GH, 3:3 + GW], want[0][k]) and torch.equal(b[:, :, 3 + GH:3 + 2 * GH, 3:3 + GW], want[1][k])


@pytest.mark.parametrize('shift', [1, 2, 3])
def test_hard_view_offset_against_the_soft_view(shift):
    """soft and hard share their strides but not their `address & 3`: the hard view starts `shift` bytes further into a
    row of its buffer.  The LDS copy of a row follows its destination's misalignment, so the hard pass must not see
    the soft pass's pixel bytes in its padding columns."""
    F, N, H, W, hw = 3, 5, 16, 24, (4, 6)
    _, GH, GW = vis.panel_geometry(F, N, 3, H, W, 1)
    img, seg = _rand((F, 3, H, W), 50), _seg(F, hw[0], hw[1], N, 51)
    a = torch.full((F, 3, GH + 2, GW + 8), 0xAA, dtype=torch.uint8, device=DEV)
    b = a.clone()
    soft, hard = a[:, :, 1:1 + GH, 1:1 + GW], b[:, :, 1:1 + GH, 1 + shift:1 + shift + GW]
    assert soft.stride() == hard.stride() and (soft.data_ptr() ^ hard.data_ptr()) & 3
    vis.slot_panel(img, seg=seg, hw=hw, hard=True, fused=True, out=(soft, hard))
    ws, wh = vis.slot_panel(img, seg=seg, hw=hw, hard=True, fused=False)
    assert torch.equal(soft, ws) and torch.equal(hard, wh)
    for buf, view in ((a, soft), (b, hard)):
        keep = view.clone()
        view.fill_(0xAA)
        assert (buf == 0xAA).all()                              # nothing outside the rectangle was written
        view.copy_(keep)


def test_attention_map_view_with_a_storage_offset_is_accepted():
    """A contiguous attention map that is not 16-byte aligned (a slice of a larger tensor with an odd frame size): the
    wrapper hands the kernel an aligned copy, on the automatic path too."""
    F, N, H, W, hw = 3, 5, 16, 24, (5, 7)
    img = _rand((F, 3, H, W), 60)
    seg = _seg(F + 1, hw[0], hw[1], N, 61)[1:]
    assert seg.is_contiguous() and seg.data_ptr() % 16
    want = vis.slot_panel(img, seg=seg, hw=hw, fused=False)
    assert torch.equal(vis.slot_panel(img, seg=seg, hw=hw, fused=True), want)
    assert torch.equal(vis.slot_panel(img, seg=seg, hw=hw), want)


@pytest.mark.parametrize('planar', [True, False])
def test_exact_arithmetic_operands_match_integer_expectation(planar):
    """Masks in {0, 0.5, 1} at h == H and images on multiples of 1 / 128: every product and sum is exact, so the bytes
    are (255 (i + 128)) // 256 for a pixel i / 128 shown as it is, (255 (i + 384)) // 512 under a half mask and 255
    under a zero mask, whatever the contraction or the order of operations."""
    F, N, H, W = 2, 3, 11, 13
    g = torch.Generator().manual_seed(40)
    i = torch.randint(-128, 129, (F, 3, H, W), generator=g)
    img = (i.float() / 128.).to(DEV)
    patterns = torch.tensor([[1., 0., 0.], [.5, .5, 0.], [0., .5, .5], [0., 0., 1.], [0., 1., 0.]])
    pick = torch.randint(0, len(patterns), (F, H, W), generator=g)
    m = patterns[pick].permute(0, 3, 1, 2).contiguous()                       # [F, N, H, W]
    if planar:
        soft, hard = vis.slot_panel(img, masks=m.to(DEV), tiles=('img',), hard=True, fused=True)
    else:
        seg = m.flatten(2).permute(0, 2, 1).contiguous().to(DEV)
        soft, hard = vis.slot_panel(img, seg=seg, hw=(H, W), tiles=('img',), hard=True, fused=True)
    i = i.numpy().astype(np.int64)
    shown = (255 * (i + 128)) // 256
    half = (255 * (i + 384)) // 512
    mm = m.numpy()[:, :, None]                                                # [F, N, 1, H, W]
    want_soft = np.where(mm == 1., shown[:, None], np.where(mm == .5, half[:, None], 255))
    one = np.eye(N)[m.numpy().argmax(1)].transpose(0, 3, 1, 2)[:, :, None]    # the first maximum: the lowest index
    want_hard = np.where(one == 1., shown[:, None], 255)
    for got, want in ((soft, want_soft), (hard, want_hard)):
        got = got.cpu().numpy()
        assert got.shape == (F, 3, H + 4, 4 * (W + 2) + 2)
        assert np.array_equal(got[:, :, 2:2 + H, 2:2 + W], shown)
        for k in range(N):
            x0 = 2 + (1 + k) * (W + 2)
            assert np.array_equal(got[:, :, 2:2 + H, x0:x0 + W], want[:, k]), k
        pad = np.ones(got.shape[2:], dtype=bool)
        for k in range(N + 1):
            pad[2:2 + H, 2 + k * (W + 2):2 + k * (W + 2) + W] = False
        assert (got[:, :, pad] == 0).all()
