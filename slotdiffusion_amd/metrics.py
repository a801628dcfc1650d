"""Evaluation metrics with the pixel work on the GPU.

Host-side mirror of video_based/models/eval_utils.py (img_based twin identical): ARI / FG-ARI
(119-186), Hungarian mIoU (238-263, 293-320), mBO (266-290, 323-333), MSE / PSNR (75-92).  The
per-pixel part -- the (gt id, pred id) contingency table of every image, the per-image squared
error -- runs in HIP kernels (sdmi_contingency, sdmi_sqerr_rows); what is left is arithmetic on a
[B, C, K] table of exact integers, done with the reference's own float32 formulas on the host, and
scipy's linear_sum_assignment for the matching, exactly as the reference does.

The evaluation stage (slotdiffusion_amd/evaluate.py) does not make id maps at all: sdmi_seg_tables turns Slot
Attention's attention map into the tables directly (seg_tables), with one extra row for the pixels of the overlap
map of COCO / VOC (img_based/models/eval_utils.py:119-135), and scores_from_tables does the arithmetic.  The five
*_metric functions take the reference's optional third argument, inst_overlap_mask, through the same tables.

The image-quality stage (slotdiffusion_amd/quality.py) scores a batch of frames in one launch: image_quality ->
sdmi_img_quality gives the per-frame squared error and SSIM of the to_rgb images and the 8-bit frames the reference
saves, from NCHW images or the decoder's NHWC-4 rows; batch_quality turns the table into mse / psnr / ssim.

Not covered: LPIPS (lpips networks), bounding-box AP/AR (torchvision ops), postproc_mask.
"""
import numpy as np
import torch

from . import _lib

__all__ = ['contingency', 'adjusted_rand_index', 'ARI_metric', 'fARI_metric', 'miou_metric',
           'fmiou_metric', 'mbo_metric', 'mse_metric', 'psnr_metric', 'seg_tables', 'seg_tables_covers',
           'overlap_tables', 'scores_from_tables', 'batch_scores', 'to_rgb', 'image_quality', 'img_quality_covers',
           'img_quality_bands', 'batch_quality']


def _need_gpu(t):
    if not t.is_cuda:
        raise RuntimeError('slotdiffusion_amd.metrics runs on the GPU (libsdmi); got a CPU tensor')


def contingency(true_ids, pred_ids, num_true=None, num_pred=None):
    """Integer ids [B, ...] (any trailing shape, e.g. [B,H,W] or [B,T,H,W]) -> int32 table
    [B, C, K] on the device; C / K default to max id + 1 over the batch (the one_hot widths)."""
    _need_gpu(true_ids)
    _need_gpu(pred_ids)
    assert true_ids.shape == pred_ids.shape
    assert 'int' in str(true_ids.dtype) and 'int' in str(pred_ids.dtype)
    B = true_ids.shape[0]
    g = true_ids.reshape(B, -1).to(torch.int32).contiguous()
    q = pred_ids.reshape(B, -1).to(torch.int32).contiguous()
    C = int(num_true if num_true is not None else int(g.max()) + 1)
    K = int(num_pred if num_pred is not None else int(q.max()) + 1)
    counts = torch.zeros((B, C, K), dtype=torch.int32, device=g.device)
    _lib.call('sdmi_contingency', torch.cuda.current_stream().cuda_stream, gt=g.data_ptr(),
              pred=q.data_ptr(), counts=counts.data_ptr(), B=B, P=g.shape[1], Kg=C, Kp=K)
    return counts


def _ari_from_table(tab):
    """Adjusted Rand index per image from the float32 contingency table [B, C, K], with the float32
    operation order of the reference (eval_utils.py:157-176) so that the scores are identical:
    pairs(v) = sum v*(v-1) over cells / row sums / column sums; expected = rows*cols / total pairs;
    score = (cells - expected) / ((rows + cols)/2 - expected), 1 where that denominator is 0."""
    pairs = lambda v, dims: torch.sum(v * (v - 1), dim=dims)
    row_tot, col_tot = tab.sum(-1), tab.sum(-2)
    n_pix = row_tot.sum(1)
    same_cell = pairs(tab, [1, 2])
    same_row, same_col = pairs(row_tot, 1), pairs(col_tot, 1)
    chance = same_row * same_col / torch.clamp(n_pix * (n_pix - 1), min=1)
    gap = (same_row + same_col) / 2 - chance
    score = (same_cell - chance) / gap
    return torch.where(gap != 0, score, torch.ones_like(score))


def adjusted_rand_index(true_ids, pred_ids, ignore_background=False):
    """-> float32 [B] (CPU), eval_utils.py:119-176."""
    N = contingency(true_ids, pred_ids).cpu().float()
    if ignore_background:
        N = N[:, 1:]
    return _ari_from_table(N)


def ARI_metric(x, y, inst_overlap_mask=None):
    if inst_overlap_mask is not None:
        return batch_scores(overlap_tables(x, y, inst_overlap_mask), ('ari',))['ari']
    return adjusted_rand_index(x, y, ignore_background=False).mean().item()


def fARI_metric(x, y, inst_overlap_mask=None):
    if inst_overlap_mask is not None:
        return batch_scores(overlap_tables(x, y, inst_overlap_mask), ('fari',))['fari']
    return adjusted_rand_index(x, y, ignore_background=True).mean().item()


def _iou_tables(gt_mask, pred_mask):
    """Per-image (intersect [N_i, M_i] float32) with the per-image one_hot widths of the
    reference (N_i = max gt id of the image + 1, M_i likewise)."""
    return _crop_per_image(contingency(gt_mask, pred_mask).cpu())


def _crop_per_image(T):
    out = []
    for b in range(T.shape[0]):
        t = T[b]
        rows = torch.nonzero(t.sum(1)).flatten()
        cols = torch.nonzero(t.sum(0)).flatten()
        n = int(rows.max()) + 1 if len(rows) else 1
        m = int(cols.max()) + 1 if len(cols) else 1
        out.append(t[:n, :m].float())
    return out


def _iou(inter, ignore_background):
    true_cnt = inter.sum(1)                      # pixels per gt id (one_hot column sums)
    pred_cnt = inter.sum(0)
    if ignore_background:
        inter, true_cnt = inter[1:], true_cnt[1:]
    union = true_cnt[:, None] + pred_cnt[None] - inter
    return (inter / (union + 1e-8)).numpy()


def _hungarian_miou(inter, ignore_background):
    from scipy.optimize import linear_sum_assignment
    if inter.shape[0] == 1 and ignore_background:          # GT holds only the background id
        return np.nan
    iou = _iou(inter, ignore_background)
    N, M = iou.shape
    row_ind, col_ind = linear_sum_assignment(iou, maximize=True)
    if M >= N:
        return iou[row_ind, col_ind].mean()
    return iou[row_ind, col_ind].sum() / float(N)


def miou_metric(gt_mask, pred_mask, inst_overlap_mask=None, ignore_background=False):
    if inst_overlap_mask is not None:
        k = 'fmiou' if ignore_background else 'miou'
        return batch_scores(overlap_tables(gt_mask, pred_mask, inst_overlap_mask), (k,))[k]
    ious = [_hungarian_miou(t, ignore_background) for t in _iou_tables(gt_mask, pred_mask)]
    if all(np.isnan(v) for v in ious):
        return np.nan
    return np.nanmean(ious)


def fmiou_metric(gt_mask, pred_mask, inst_overlap_mask=None):
    return miou_metric(gt_mask, pred_mask, inst_overlap_mask, ignore_background=True)


def mbo_metric(gt_mask, pred_mask, inst_overlap_mask=None):
    if inst_overlap_mask is not None:
        return batch_scores(overlap_tables(gt_mask, pred_mask, inst_overlap_mask), ('mbo',))['mbo']
    mbos = []
    for t in _iou_tables(gt_mask, pred_mask):
        if t.shape[0] == 1:
            mbos.append(np.nan)
        else:
            mbos.append(_iou(t, True).max(1).mean())
    return np.nanmean(mbos)


# ------------------------------------------------------------------------------------------
# tables with the overlap row (sdmi_seg_tables' layout) and the scores on them
# ------------------------------------------------------------------------------------------
SCORE_KEYS = ('ari', 'fari', 'miou', 'fmiou', 'mbo')
_SEG_LDS = 160 * 1024


def seg_tables_covers(N, Kg, w, maps=1):
    """The gate of sdmi_seg_tables (include/sdmi.h): the table size sdmi_contingency admits, and the tables plus a
    one-row band (two source rows) inside the LDS."""
    if not (N >= 1 and Kg >= 1 and w >= 1 and (Kg + 1) * N <= 8192):
        return False
    return maps * (Kg + 1) * N * 4 + ((2 * w * N + 11) // 4 * 4) * 4 <= _SEG_LDS


def seg_tables(seg, gt, hw, num_true, *, time_major=False, gt2=None, overlap=None, counts=None, ids_dtype=None,
               fused=None):
    """Slot Attention's attention map -> contingency tables, without masks or id maps in memory (sdmi_seg_tables).

    seg [F, h*w, N] fp32 with hw = (h, w), F = B * T frames in [B][T] order (time_major=False) or the stream's [T][B]
    order (True).  gt, gt2 (optional second ground truth: semantic ids), overlap (optional; non-zero = overlapped):
    int32 [B, T, H, W], any batch / time strides (a chunk of a longer video is a plain slice).  num_true = Kg.
    -> counts int32 [B, maps, Kg + 1, N] (row Kg: the overlapped pixels by predicted id), created zeroed when not
    given and otherwise ADDED to (the next chunk of the same videos), and the id map [F, H, W] when ids_dtype
    (torch.int32 / torch.uint8) asks for one.  Outside seg_tables_covers, or with fused=False, the same tables come
    from the composed path: mask_upsample_argmax(want_up=False), then sdmi_contingency on rows remapped by `overlap`."""
    from . import ops
    _need_gpu(seg)
    h, w = hw
    F_, M, N = seg.shape
    B, T, H, W = gt.shape
    Kg = int(num_true)
    maps_in = [gt] + ([gt2] if gt2 is not None else [])
    assert F_ == B * T and M == h * w and seg.dtype == torch.float32
    for m in maps_in + ([overlap] if overlap is not None else []):
        _need_gpu(m)
        assert m.dtype == torch.int32 and m.shape == gt.shape and m.stride() == gt.stride(), 'maps share shape and strides'
    assert gt.stride(3) == 1 and gt.stride(2) == W, 'a map\'s [H, W] plane is contiguous'
    if counts is None:
        counts = torch.zeros((B, len(maps_in), Kg + 1, N), dtype=torch.int32, device=seg.device)
    assert counts.shape == (B, len(maps_in), Kg + 1, N) and counts.dtype == torch.int32 and counts.is_contiguous()
    seg = seg.contiguous()
    if seg.data_ptr() % 16:
        seg = seg.clone()
    if fused is None:
        fused = seg_tables_covers(N, Kg, w, len(maps_in))
    if fused:
        ids = torch.empty((F_, H, W), dtype=ids_dtype, device=seg.device) if ids_dtype is not None else None
        assert ids_dtype in (None, torch.int32, torch.uint8)
        _lib.call('sdmi_seg_tables', torch.cuda.current_stream().cuda_stream, seg=seg.data_ptr(), gt=gt.data_ptr(),
                  gt2=gt2.data_ptr() if gt2 is not None else 0, overlap=overlap.data_ptr() if overlap is not None else 0,
                  counts=counts.data_ptr(), ids=ids.data_ptr() if ids is not None else 0,
                  ids_u8=int(ids_dtype == torch.uint8), B=B, T=T, time_major=int(time_major), N=N, h=h, w=w, H=H, W=W,
                  Kg=Kg, map_bstride=gt.stride(0), map_tstride=gt.stride(1))
        return (counts, ids) if ids_dtype is not None else counts
    _, idx = ops.mask_upsample_argmax(seg, h, w, H, W, want_up=False)           # [F, H, W] int64
    idx = idx.view(T, B, H, W).transpose(0, 1) if time_major else idx.view(B, T, H, W)
    for i, m in enumerate(maps_in):
        rows = m if overlap is None else torch.where(overlap != 0, torch.full_like(m, Kg), m)
        counts[:, i] += contingency(rows, idx, Kg + 1, N)
    if ids_dtype is not None:
        flat = idx.transpose(0, 1) if time_major else idx
        return counts, flat.reshape(F_, H, W).to(ids_dtype)
    return counts


def overlap_tables(gt_mask, pred_mask, inst_overlap_mask=None):
    """Id maps [B, ...] (+ overlap map of the same shape, non-zero = overlapped) -> int table [B, Kg + 1, N] on the CPU in
    sdmi_seg_tables' layout: overlapped pixels are counted in the extra row Kg under their predicted id."""
    Kg, N = int(gt_mask.max()) + 1, int(pred_mask.max()) + 1
    rows = gt_mask
    if inst_overlap_mask is not None:
        rows = torch.where(inst_overlap_mask.to(gt_mask.device) != 0, torch.full_like(gt_mask, Kg), gt_mask)
    return contingency(rows, pred_mask, Kg + 1, N).cpu()


def _resolve_overlap(tab):
    """One sample's [Kg + 1, N] integer table -> [Kg, N + 1]: the reference's preproc_masks_overlap on counts
    (img_based/models/eval_utils.py:130-134).  The overlapped pixels (row Kg) become gt 0 / predicted id
    `largest predicted id of the image + 1`, that maximum taken over ALL pixels, overlapped ones included."""
    body, extra = tab[:-1], tab[-1]
    out = torch.zeros((body.shape[0], body.shape[1] + 1), dtype=tab.dtype)
    out[:, :-1] = body
    n_ov = int(extra.sum())
    if n_ov:
        top = int(torch.nonzero(body.sum(0) + extra).max())
        out[0, top + 1] += n_ov
    return out


def scores_from_tables(tables, keys=SCORE_KEYS):
    """tables: integer [S, Kg + 1, N] (sdmi_seg_tables' / overlap_tables' layout; any device) of ONE batch, in the sense
    of the reference's metric functions: the S samples share the one_hot widths of adjusted_rand_index
    (eval_utils.py:161-167).  -> {key: float array [S]} per-sample ARI, FG-ARI (float32, reference operation order:
    _ari_from_table), Hungarian mIoU, foreground mIoU and mBO (NaN where the reference returns NaN: a ground truth
    that holds the background id alone)."""
    tabs = torch.stack([_resolve_overlap(t) for t in torch.as_tensor(tables).cpu().long()])      # [S, Kg, N + 1]
    out = {}
    if 'ari' in keys or 'fari' in keys:
        used_r = torch.nonzero(tabs.sum((0, 2))).flatten()
        used_c = torch.nonzero(tabs.sum((0, 1))).flatten()
        C = int(used_r.max()) + 1 if len(used_r) else 1
        K = int(used_c.max()) + 1 if len(used_c) else 1
        full = tabs[:, :C, :K].float().contiguous()
        if 'ari' in keys:
            out['ari'] = _ari_from_table(full).numpy()
        if 'fari' in keys:
            out['fari'] = _ari_from_table(full[:, 1:].contiguous()).numpy()
    per = _crop_per_image(tabs)
    if 'miou' in keys:
        out['miou'] = np.array([_hungarian_miou(t, False) for t in per], dtype=np.float64)
    if 'fmiou' in keys:
        out['fmiou'] = np.array([_hungarian_miou(t, True) for t in per], dtype=np.float64)
    if 'mbo' in keys:
        out['mbo'] = np.array([np.nan if t.shape[0] == 1 else _iou(t, True).max(1).mean() for t in per], dtype=np.float64)
    return out


def batch_scores(tables, keys=SCORE_KEYS, per_sample=None):
    """The reference's value of each metric for one batch (eval_utils.py:190-211, 310-370): the float32 mean of the
    per-sample ARI / FG-ARI, the nanmean of the others (NaN when every sample is NaN)."""
    per = per_sample if per_sample is not None else scores_from_tables(tables, keys)
    out = {}
    for k in keys:
        v = per[k]
        if k in ('ari', 'fari'):
            out[k] = torch.from_numpy(np.asarray(v, dtype=np.float32)).mean().item()
        else:
            out[k] = np.nan if np.all(np.isnan(v)) else float(np.nanmean(v))
    return out


def _sqerr(x, y, mode=0):
    _need_gpu(x)
    _need_gpu(y)
    assert x.shape == y.shape
    B = x.shape[0]
    xf = x.reshape(B, -1).float().contiguous()
    yf = y.reshape(B, -1).float().contiguous()
    n = xf.shape[1]
    nchunk = max(1, min(64, n // 4096))
    part = torch.empty((B, nchunk), dtype=torch.float64, device=x.device)
    _lib.call('sdmi_sqerr_rows', torch.cuda.current_stream().cuda_stream, x=xf.data_ptr(),
              y=yf.data_ptr(), partial=part.data_ptr(), B=B, n=n, nchunk=nchunk, mode=mode)
    return part.cpu().sum(1).numpy(), n


def mse_metric(x, y):
    """x/y [B,3,H,W] in [0,1]: squared error summed over an image, mean over the batch."""
    se, _ = _sqerr(x, y)
    return float(se.mean())


def psnr_metric(x, y):
    """skimage.metrics.peak_signal_noise_ratio(data_range=1) per image, mean over the batch:
    10 * log10(1 / mean squared error)."""
    se, n = _sqerr(x, y)
    return float(np.mean(10.0 * np.log10(1.0 / (se / n))))


def ssim_metric(x, y):
    """eval_utils.ssim_metric (eval_utils.py:91-106): x / y [B,3,H,W] in [0,1] -> mean over images of
    skimage's structural_similarity(x*255, y*255, channel_axis=0, gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False, data_range=255).  skimage is absent offline: the published algorithm
    is restated (sdmi_ssim); parity with skimage itself is unpinned."""
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    _need_gpu(x)
    _need_gpu(y)
    assert x.shape == y.shape and x.dim() == 4
    B, Cc, H, W = x.shape
    xf = (x.float() * 255.0).contiguous()
    yf = (y.float() * 255.0).contiguous()
    out = torch.empty((B * Cc,), dtype=torch.float64, device=x.device)
    _lib.call('sdmi_ssim', torch.cuda.current_stream().cuda_stream, x=xf.data_ptr(), y=yf.data_ptr(),
              out=out.data_ptr(), P=B * Cc, H=H, W=W, data_range=255.0)
    return float(out.view(B, Cc).mean(1).mean().cpu())        # mean over channels, then over images


# ------------------------------------------------------------------------------------------
# the scoring tail of the reconstruction / prediction scripts in one launch (sdmi_img_quality)
# ------------------------------------------------------------------------------------------
_IMG_QUALITY_FUSED = True          # tests and tools/bench_quality.py flip it: False sends image_quality down the composed path


def to_rgb(x):
    """to_rgb_from_tensor (utils.py:47-49): [-1, 1] -> [0, 1], clamped."""
    return (x * 0.5 + 0.5).clamp(0, 1)


def img_quality_covers(H, W):
    """The gate of sdmi_img_quality (include/sdmi.h): an 11 x 11 window fits, one thread per output column."""
    return bool(H >= 11 and 11 <= W <= 256)


def img_quality_bands(H, W):
    """The kernel's band split of (H, W) (img_quality.hip, iq_geom): up to 8 sub-bands of 8 SSIM output rows side by side
    in the 256 threads, W - 10 rounded up to 32 threads each -> (output rows per band, bands per frame)."""
    h, w = H - 10, W - 10
    cw = (w + 31) // 32 * 32
    s = max(1, min(8, 256 // cw, (h + 7) // 8))
    return s * 8, (h + s * 8 - 1) // (s * 8)


def image_quality(pred, gt, *, pred_nhwc4=False, gt_nhwc4=False, want_u8=(False, False), fused=None):
    """MSE / PSNR / SSIM and the saved frames of a batch of F frames, as the reference's eval_imgs + save_results compute
    them (eval_utils.py:73-106, img_based/test_recon.py:47-61, 94-103).  pred, gt: fp32 in nominal [-1, 1], each NCHW
    [F, 3, H, W] or, with its flag, NHWC-4 [F, H, W, 4] (the decoder's rows: no transposition).  -> (table, pred_u8,
    gt_u8): table fp64 [F, 2] on the device, (squared error of the to_rgb images summed over 3 * H * W, SSIM of the
    frame); the uint8 frames [F, H, W, 3] that want_u8 = (pred, gt) asks for, None otherwise.  No host synchronisation:
    mse / psnr / ssim of the batch are batch_quality(table.cpu(), 3 * H * W).

    Inside img_quality_covers this is one sdmi_img_quality launch and a sum over its per-band partials; outside it, or
    with fused=False (default: the module flag _IMG_QUALITY_FUSED), the composed path on the kernels behind mse_metric /
    psnr_metric / ssim_metric with the same arithmetic."""
    from . import ops
    _need_gpu(pred)
    _need_gpu(gt)
    assert pred.dtype == torch.float32 and gt.dtype == torch.float32 and pred.dim() == 4 and gt.dim() == 4

    def hw(t, nhwc4):
        if nhwc4:
            assert t.shape[3] == 4, 'NHWC-4 rows are [F, H, W, 4]'
            return t.shape[0], t.shape[1], t.shape[2]
        assert t.shape[1] == 3, 'NCHW images are [F, 3, H, W]'
        return t.shape[0], t.shape[2], t.shape[3]
    F_, H, W = hw(pred, pred_nhwc4)
    assert hw(gt, gt_nhwc4) == (F_, H, W), 'pred and gt hold the same frames'
    if fused is None:
        fused = _IMG_QUALITY_FUSED and img_quality_covers(H, W)
    if fused:
        pred, gt = pred.contiguous(), gt.contiguous()
        if pred_nhwc4 and pred.data_ptr() % 16:
            pred = pred.clone()
        if gt_nhwc4 and gt.data_ptr() % 16:
            gt = gt.clone()
        _, nb = img_quality_bands(H, W)
        part = torch.empty((F_, nb, 2), dtype=torch.float64, device=pred.device)
        u8 = [torch.empty((F_, H, W, 3), dtype=torch.uint8, device=pred.device) if w else None for w in want_u8]
        _lib.call('sdmi_img_quality', torch.cuda.current_stream().cuda_stream, pred=pred.data_ptr(), gt=gt.data_ptr(),
                  partial=part.data_ptr(), pred_u8=u8[0].data_ptr() if u8[0] is not None else 0,
                  gt_u8=u8[1].data_ptr() if u8[1] is not None else 0, F=F_, H=H, W=W, pred_nhwc4=int(pred_nhwc4),
                  gt_nhwc4=int(gt_nhwc4), nbands=nb)
        return part.sum(1), u8[0], u8[1]
    a = to_rgb(ops.nhwc_to_nchw(pred.contiguous(), 3) if pred_nhwc4 else pred).contiguous()
    b = to_rgb(ops.nhwc_to_nchw(gt.contiguous(), 3) if gt_nhwc4 else gt).contiguous()
    st = torch.cuda.current_stream().cuda_stream
    n = 3 * H * W
    nchunk = max(1, min(64, n // 4096))
    part = torch.empty((F_, nchunk), dtype=torch.float64, device=a.device)
    _lib.call('sdmi_sqerr_rows', st, x=a.data_ptr(), y=b.data_ptr(), partial=part.data_ptr(), B=F_, n=n, nchunk=nchunk, mode=0)
    xs, ys = (a * 255.0).contiguous(), (b * 255.0).contiguous()
    planes = torch.empty((F_ * 3,), dtype=torch.float64, device=a.device)
    _lib.call('sdmi_ssim', st, x=xs.data_ptr(), y=ys.data_ptr(), out=planes.data_ptr(), P=F_ * 3, H=H, W=W, data_range=255.0)
    table = torch.stack([part.sum(1), planes.view(F_, 3).mean(1)], 1)
    u8 = [torch.round(t).to(torch.uint8).permute(0, 2, 3, 1).contiguous() if w else None for t, w in zip((xs, ys), want_u8)]
    return table, u8[0], u8[1]


def batch_quality(table, n):
    """The reference's values of one batch from its [F, 2] table (on the host) and n = 3 * H * W: mse = mean over frames
    of the squared error (eval_utils.py:75-78), psnr = mean over frames of 10 log10(1 / (se / n)) (81-88), ssim = mean
    over frames (91-106)."""
    t = np.asarray(table, dtype=np.float64)
    with np.errstate(divide='ignore'):
        psnr = float(np.mean(10.0 * np.log10(1.0 / (t[:, 0] / n))))
    return {'mse': float(t[:, 0].mean()), 'psnr': psnr, 'ssim': float(t[:, 1].mean())}


def shuffle_slots(slots):
    """Compositional generation (video_based/test_comp_gen.py:25-31): slot i of every item is taken
    from the item i places further along the batch, so each new scene mixes objects of N scenes.
    slots [B,T,N,C] or [B,N,C] -> a new tensor of the same shape (the input is left untouched)."""
    nd = slots.dim()
    assert nd in (3, 4)
    B, N = slots.shape[0], slots.shape[-2]
    shift = torch.arange(N, device=slots.device)
    shift = torch.where(shift < B, shift, torch.zeros_like(shift))     # slots[i:] is empty for i >= B
    src = (torch.arange(B, device=slots.device)[:, None] + shift[None]) % B
    slot_ix = torch.arange(N, device=slots.device)[None].expand(B, N)
    if nd == 3:
        return slots[src, slot_ix]
    return slots[src, :, slot_ix].permute(0, 2, 1, 3).contiguous()
