"""Slot-decomposition panels of the validation pass (video_based/vis.py, the `_make_*` builders and `_convert_*` of
img_based/method.py and video_based/method.py): image, reconstruction, coloured mask, overlay and one masked tile per
slot, laid out by make_grid and converted to bytes.

`slot_panel` is the entry: on the GPU, inside `slot_panel_covers`, it is ONE sdmi_slot_panel launch from the masks as
our kernels leave them (Slot Attention's attention map [F, h*w, N], the decoder's planar alpha masks, or a ground-truth
id map) and the frames (NCHW, or the decoder's NHWC-4 rows) to the uint8 panel, soft and hard (one-hot) at once.
`slot_panel_composed` is the reference's chain restated in plain torch ops -- the builders, a make_grid written here
(torchvision is not a dependency) and the truncating byte conversion; it runs on host tensors too, is what the fused
launch is tested against byte for byte, and is the path outside the gate.

A tile list names the tiles in front of the N slot tiles: 'img', 'recon', 'color', 'overlay', 'gtcolor'.  The
reference's builders are
    _make_img_grid (SA)            ('img', 'recon'),  slot_img = recons, masks = the alpha masks
    _make_video_grid (SAVi)        ('img', 'recon', 'color', 'overlay'),  slot_img = recons
    _make_slots_img (SADiffusion)  ('img', ['recon'], ['gtcolor'], 'color', 'overlay')  (without recon the reference's
                                   insert(2) puts 'gtcolor' AFTER 'color')
    _make_slots_video              ('img', ['recon'], 'color', 'overlay')
"""
import os

import numpy as np
import torch

__all__ = ['PALETTE', 'TILE_CODES', 'torch_palette', 'panel_geometry', 'slot_panel', 'slot_panel_composed',
           'slot_panel_covers', 'slot_panel_band', 'make_grid', 'to_bytes', 'save_panels']

# the 20 colours of the reference's table (video_based/vis.py:5-9), as data (tests/golden/vis_palette.json)
PALETTE = [[174, 199, 232], [152, 223, 138], [31, 119, 180], [255, 187, 120],
           [188, 189, 34], [140, 86, 75], [255, 152, 150], [214, 39, 40],
           [197, 176, 213], [148, 103, 189], [196, 156, 148], [23, 190, 207],
           [247, 182, 210], [219, 219, 141], [255, 127, 14], [158, 218, 229],
           [44, 160, 44], [112, 128, 144], [227, 119, 194], [82, 84, 163]]

TILE_CODES = {'img': 0, 'recon': 1, 'color': 2, 'overlay': 3, 'gtcolor': 4}     # include/sdmi.h: sdmi_slot_panel
PAD = 2                                       # make_grid's default padding
_PANEL_FUSED = True                           # off: slot_panel always takes the composed path
_LDS_BUDGET = 160 * 1024
_pal_cache = {}


def torch_palette(device='cpu'):
    """fp32 [20, 3] in [-1, 1], derived as the reference derives it (vis.py:12-15): / 255.0 in float64, to float32,
    then * 2 - 1."""
    key = str(device)
    if key not in _pal_cache:
        _pal_cache[key] = (torch.from_numpy(np.array(PALETTE) / 255.0).float() * 2. - 1.).to(device)
    return _pal_cache[key]


def panel_geometry(F, N, nprefix, H, W, G=1):
    """-> (pictures, GH, GW) of F frames in tile rows of G: make_grid with padding 2 and nrow = nprefix + N."""
    assert F % G == 0, (F, G)
    return F // G, G * (H + PAD) + PAD, (nprefix + N) * (W + PAD) + PAD


# ------------------------------------------------------------------------------------------
# the gate of sdmi_slot_panel, mirrored (csrc/slot_panel.hip: pnl_plan)
# ------------------------------------------------------------------------------------------
def _src_lo(scale, y):
    f = np.float32(scale * (np.float32(y) + np.float32(0.5))) - np.float32(0.5)
    return int(max(f, np.float32(0.)))


def _band_rows(band, h, H):
    scale = np.float32(h) / np.float32(H)
    most = 1
    for r0 in range(0, H, band):
        r1 = min(r0 + band, H)
        lo = _src_lo(scale, r1 - 1)
        hi = lo + (1 if lo < h - 1 else 0)
        most = max(most, hi - _src_lo(scale, r0) + 1)
    return most


def slot_panel_band(N, nprefix, H, W, h, w, staged=True):
    """The band height (8, 4, 2 or 1 output rows per workgroup) sdmi_slot_panel uses for a shape, 0 when not even one
    row fits its LDS budget.  staged: the mask source is the attention map [F, h*w, N], whose rows are staged in LDS."""
    GW = (nprefix + N) * (W + PAD) + PAD
    pitch = (GW + 3 + 3) // 4 * 4
    band = 8
    while band > H:
        band //= 2
    while band >= 1:
        stage = ((_band_rows(band, h, H) * w * N + 8 + 3) // 4 * 4) if staged else 0
        if stage * 4 + band * W * 4 + 3 * band * pitch <= _LDS_BUDGET:
            return band
        band //= 2
    return 0


def slot_panel_covers(N, nprefix, H, W, h, w, staged=True, P=20, colour=True):
    """The gate of sdmi_slot_panel (include/sdmi.h): N, sizes >= 1, at most 8 tiles in front, N <= P when a COLOR or
    OVERLAY tile is asked for, and one band row inside the LDS budget."""
    if N < 1 or min(H, W, h, w) < 1 or not 0 <= nprefix <= 8 or (colour and N > P):
        return False
    return slot_panel_band(N, nprefix, H, W, h, w, staged) > 0


# ------------------------------------------------------------------------------------------
# composed path: the reference's chain in torch ops
# ------------------------------------------------------------------------------------------
def make_grid(tiles, nrow, padding=PAD, pad_value=-1.):
    """torchvision.utils.make_grid for [n, C, H, W] tiles (no normalisation): rows of `nrow` tiles, `padding` pixels of
    pad_value above and left of every tile and along the bottom and right edges."""
    n, C, H, W = tiles.shape
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    hh, ww = H + padding, W + padding
    grid = tiles.new_full((C, hh * ymaps + padding, ww * xmaps + padding), pad_value)
    for k in range(n):
        y, x = divmod(k, xmaps)
        grid[:, y * hh + padding:y * hh + padding + H, x * ww + padding:x * ww + padding + W] = tiles[k]
    return grid


def to_bytes(x):
    """to_rgb_from_tensor, * 255, astype(np.uint8): [-1, 1] floats -> bytes, TRUNCATED (method.py:31-44, 50-57)."""
    return ((x * 0.5 + 0.5).clamp(0, 1) * 255.).to(torch.uint8)


def _upsample_host(seg, h, w, H, W):
    """mask_up_kernel's bilinear upsample (align_corners=False) in torch ops, expression for expression:
    seg [F, h*w, N] -> [F, N, H, W].  For the host side of the composed path."""
    F, _, N = seg.shape
    s = seg.reshape(F, h, w, N).float()
    one, half = torch.tensor(1., dtype=torch.float32), torch.tensor(0.5, dtype=torch.float32)
    sy = torch.tensor(h, dtype=torch.float32) / torch.tensor(H, dtype=torch.float32)
    sx = torch.tensor(w, dtype=torch.float32) / torch.tensor(W, dtype=torch.float32)
    fy = (sy * (torch.arange(H, dtype=torch.float32) + half) - half).clamp_min(0.)
    fx = (sx * (torch.arange(W, dtype=torch.float32) + half) - half).clamp_min(0.)
    y0, x0 = fy.long(), fx.long()
    y1, x1 = y0 + (y0 < h - 1).long(), x0 + (x0 < w - 1).long()
    ly1, lx1 = (fy - y0.float()).to(seg.device), (fx - x0.float()).to(seg.device)
    ly0, lx0 = one.to(seg.device) - ly1, one.to(seg.device) - lx1
    y0, y1, x0, x1 = (t.to(seg.device) for t in (y0, y1, x0, x1))
    lx0, lx1 = lx0.view(1, 1, W, 1), lx1.view(1, 1, W, 1)
    ly0, ly1 = ly0.view(1, H, 1, 1), ly1.view(1, H, 1, 1)
    top = lx0 * s[:, y0][:, :, x0] + lx1 * s[:, y0][:, :, x1]
    bot = lx0 * s[:, y1][:, :, x0] + lx1 * s[:, y1][:, :, x1]
    return (ly0 * top + ly1 * bot).permute(0, 3, 1, 2).contiguous()


def _nchw(x, nhwc4):
    return x[..., :3].permute(0, 3, 1, 2) if nhwc4 else x


def _masks_and_ids(img, seg, hw, masks, ids, num_classes):
    """-> (m [F, N, H, W] fp32, a [F, H, W] int64 with -1 for an id outside [0, N))."""
    F, _, H, W = img.shape
    if ids is not None:
        ids = ids.long()
        valid = (ids >= 0) & (ids < num_classes)
        a = torch.where(valid, ids, torch.full_like(ids, -1))
        m = torch.nn.functional.one_hot(a.clamp_min(0), num_classes).permute(0, 3, 1, 2).float()
        return m * valid.unsqueeze(1).float(), a
    if masks is not None:                          # planar [F, N, h, w]
        h, w = masks.shape[-2:]
        seg = masks.flatten(2).permute(0, 2, 1).contiguous()
    else:
        h, w = hw
    if seg.is_cuda:
        from . import ops
        m, a = ops.mask_upsample_argmax(seg.float().contiguous(), h, w, H, W)
        return m, a
    m = _upsample_host(seg, h, w, H, W)
    return m, m.argmax(1)                          # (the first maximal value: the lowest index wins a tie)


def _draw(a, pal):
    """torch_draw_mask with our rule for ids outside the table: the colour -1 (byte 0) -> ([F, 3, H, W], valid)."""
    valid = (a >= 0) & (a < pal.shape[0])
    col = pal[a.clamp(0, pal.shape[0] - 1)].permute(0, 3, 1, 2)
    return col, valid.unsqueeze(1)


def slot_panel_composed(img, *, seg=None, hw=None, masks=None, ids=None, num_classes=None, recon=None, gt=None,
                        slot_img=None, tiles=('img', 'color', 'overlay'), G=1, hard=False, palette=None,
                        img_nhwc4=False, recon_nhwc4=False):
    """The reference's builders followed by make_grid and the byte conversion, in plain torch ops (arguments:
    slot_panel's).  -> uint8 [pictures, 3, GH, GW], or (soft, hard) of them with hard=True.  On the GPU the upsampled
    masks and their argmax are ops.mask_upsample_argmax's; on the host a restatement of that kernel's arithmetic."""
    img = _nchw(img.float(), img_nhwc4)
    F, _, H, W = img.shape
    pal = torch_palette(img.device) if palette is None else palette
    m, a = _masks_and_ids(img, seg, hw, masks, ids, num_classes)
    N = m.shape[1]
    neg = torch.tensor(-1., dtype=torch.float32, device=img.device)
    front = []
    for name in tiles:
        if name == 'img':
            t = img
        elif name == 'recon':
            t = _nchw(recon.float(), recon_nhwc4)
        elif name == 'gtcolor':
            col, valid = _draw(gt.long(), pal)
            t = torch.where(valid, col, neg)
        else:
            assert N <= pal.shape[0], 'more slots than colours'
            col, valid = _draw(a, pal)
            if name == 'color':
                t = torch.where(valid, col, neg)
            elif name == 'overlay':                               # torch_draw_rgb_mask, alpha = 0.7
                t = torch.where(valid, img * 0.7 + col * (1. - 0.7), neg)
            else:
                raise KeyError(name)
        front.append(t.unsqueeze(1))
    src = img.unsqueeze(1) if slot_img is None else slot_img.float()
    outs = []
    variants = [m]
    if hard:                                                      # make_one_hot: 1 at the argmax
        onehot = torch.nn.functional.one_hot(a.clamp_min(0), N).permute(0, 3, 1, 2).float()
        variants.append(onehot * (a >= 0).unsqueeze(1).float())
    for mk in variants:
        mk = mk.unsqueeze(2)
        allt = torch.cat(front + [src * mk + (1. - mk)], dim=1)   # [F, K, 3, H, W]
        K = allt.shape[1]
        pics = torch.stack([make_grid(allt[i:i + G].flatten(0, 1), nrow=K, pad_value=-1.) for i in range(0, F, G)])
        outs.append(to_bytes(pics))
    return (outs[0], outs[1]) if hard else outs[0]


# ------------------------------------------------------------------------------------------
# the wrapper
# ------------------------------------------------------------------------------------------
def _f32(x):
    return None if x is None else x.float().contiguous()


def _i32(x):
    return None if x is None else x.to(torch.int32).contiguous()


def slot_panel(img, *, seg=None, hw=None, masks=None, ids=None, num_classes=None, recon=None, gt=None, slot_img=None,
               tiles=('img', 'color', 'overlay'), G=1, hard=False, palette=None, img_nhwc4=False, recon_nhwc4=False,
               out=None, fused=None):
    """F frames -> the uint8 panel [pictures, 3, GH, GW] (panel_geometry); with hard=True -> (soft, hard), the second
    with one-hot masks in the slot tiles.

    img [F, 3, H, W] fp32, or [F, H, W, 4] with img_nhwc4; recon likewise (recon_nhwc4) for a 'recon' tile.  Exactly one
    mask source: seg [F, h*w, N] with hw = (h, w) (Slot Attention's attention map), masks [F, N, h, w] (planar), or ids
    [F, H, W] integer with num_classes (the ground-truth panel).  gt [F, H, W] integer feeds 'gtcolor'.  slot_img
    [F, N, 3, H, W] replaces img inside the slot tiles.  Frame f lands in picture f // G, tile row f % G.  out: a uint8
    tensor [pictures, 3, GH, GW] (or a pair for hard=True) to write into, any strides with unit column stride -- a band
    of rows of a taller picture, say.  fused: None = the fused launch when the tensors are on the GPU, the shape is
    inside slot_panel_covers and _PANEL_FUSED is on; True = the launch or an error; False = the composed path."""
    assert (seg is not None) + (masks is not None) + (ids is not None) == 1, 'exactly one mask source'
    F = img.shape[0]
    H, W = (img.shape[1:3] if img_nhwc4 else img.shape[2:4])
    if ids is not None:
        N, (h, w) = int(num_classes), (H, W)
    elif masks is not None:
        N, (h, w) = masks.shape[1], masks.shape[-2:]
    else:
        N, (h, w) = seg.shape[2], hw
        assert seg.shape[1] == h * w
    tiles = tuple(tiles)
    colour = any(t in ('color', 'overlay') for t in tiles)
    pal = torch_palette(img.device) if palette is None else palette
    I, GH, GW = panel_geometry(F, N, len(tiles), H, W, G)
    if fused is None:
        fused = _PANEL_FUSED and img.is_cuda and slot_panel_covers(N, len(tiles), H, W, h, w, seg is not None,
                                                                   pal.shape[0], colour)
    outs = None
    if out is not None:
        outs = tuple(out) if hard else (out,)
        for o in outs:
            assert o.dtype == torch.uint8 and tuple(o.shape) == (I, 3, GH, GW) and o.stride(3) == 1, 'bad out'
        assert not hard or all(o.stride() == outs[0].stride() for o in outs), 'soft and hard share their strides'
    if not fused:
        res = slot_panel_composed(img, seg=seg, hw=hw, masks=masks, ids=ids, num_classes=num_classes, recon=recon,
                                  gt=gt, slot_img=slot_img, tiles=tiles, G=G, hard=hard, palette=palette,
                                  img_nhwc4=img_nhwc4, recon_nhwc4=recon_nhwc4)
        if outs is None:
            return res
        for o, r in zip(outs, res if hard else (res,)):
            o.copy_(r)
        return out
    from . import _lib
    if outs is None:
        outs = tuple(torch.empty((I, 3, GH, GW), dtype=torch.uint8, device=img.device) for _ in range(2 if hard else 1))
    code = 0
    for j, t in enumerate(tiles):
        code |= TILE_CODES[t] << (4 * j)
    seg32 = _f32(seg)
    if seg32 is not None and seg32.data_ptr() % 16:        # a view with a storage offset: the kernel's 16-byte loads
        seg32 = seg32.clone()
    keep = [_f32(img), _f32(recon), seg32, _f32(masks), _i32(ids), _i32(gt), _f32(slot_img), _f32(pal)]
    p = [0 if t is None else t.data_ptr() for t in keep]
    o0 = outs[0]
    _lib.call('sdmi_slot_panel', torch.cuda.current_stream().cuda_stream, img=p[0], recon=p[1], seg=(p[2] or p[3]),
              ids=p[4], gt=p[5], slot_img=p[6], palette=p[7], soft=o0.data_ptr(),
              hard=(outs[1].data_ptr() if hard else 0), F=F, G=G, N=N, P=pal.shape[0], H=H, W=W, h=h, w=w,
              img_nhwc4=int(img_nhwc4), recon_nhwc4=int(recon_nhwc4), seg_planar=int(masks is not None),
              nprefix=len(tiles), tiles=code, img_stride=o0.stride(0), ch_stride=o0.stride(1), row_stride=o0.stride(2))
    del keep
    if out is not None:
        return out
    return outs if hard else outs[0]


def save_panels(path, log):
    """Write the pictures of a validation log (Method.validate: uint8 arrays, [H, W, 3] = an image, [T, 3, H, W] = a
    video) under `path`: an image as <key>.png, a video as a folder <key>/ of one PNG per frame (no mp4); '/' in a key
    becomes '_'.  Other values are skipped.  -> the paths written."""
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    written = []
    for key, val in log.items():
        if not (isinstance(val, np.ndarray) and val.dtype == np.uint8):
            continue
        name = key.replace('/', '_')
        if val.ndim == 3:
            f = os.path.join(path, name + '.png')
            Image.fromarray(val).save(f)
            written.append(f)
        elif val.ndim == 4:
            d = os.path.join(path, name)
            os.makedirs(d, exist_ok=True)
            for t, frame in enumerate(val):
                f = os.path.join(d, f'{t:04d}.png')
                Image.fromarray(np.ascontiguousarray(frame.transpose(1, 2, 0))).save(f)
                written.append(f)
    return written
