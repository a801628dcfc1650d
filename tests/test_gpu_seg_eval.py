"""sdmi_seg_tables on the GPU: the tables of the fused kernel against the composed path (sdmi_mask_upsample_argmax, then
sdmi_contingency) as integers, against a float64 bilinear upsample, on ties, across calls and frame orders, with two
ground truths and the overlap row; and evaluate_video_segmentation on a small SAViDiffusion against model.encode of the
whole clip.

Everything compared is an integer table, so every comparison is for equality.  The float64 check may leave out a pixel
whose float64 top-two margin is below 1e-6 (from both tables; at most 0.1 % of a case's pixels): with the recipe used
here -- softmax of 3 * randn, seed 1234 + 100 h + N -- no pixel of any listed shape falls under that margin on the CPU,
so the cap is not expected to be used."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from slotdiffusion_amd import evaluate, extract, ops
from slotdiffusion_amd import metrics as MT
from tests.test_gpu_bwd_helpers import _end_the_session_on_a_gpu_fault, _gen  # noqa: F401
from tests.test_seg_eval_cpu import cpu_tables

pytestmark = pytest.mark.gpu

SHAPES = [(8, 8, 32, 32, 5), (4, 4, 32, 32, 7), (6, 10, 24, 40, 11), (9, 9, 36, 36, 16), (5, 5, 32, 32, 17), (7, 7, 28, 28, 1)]
B, KG = 3, 6
MARGIN, CAP = 1e-6, 1e-3


def _seg(h, w, N, frames=B):
    return torch.softmax(3.0 * torch.randn(frames, h * w, N, generator=_gen(1234 + 100 * h + N)), dim=-1)


def _gt(frames, H, W, seed, kg=KG):
    return torch.randint(0, kg, (frames, 1, H, W), generator=_gen(seed), dtype=torch.int32)


def _composed(seg, gt, h, w, num_true=KG):
    """-> (tables [B, Kg, N] of sdmi_contingency on the ids of sdmi_mask_upsample_argmax, those ids [F, H, W] int64)."""
    H, W = gt.shape[-2:]
    _, idx = ops.mask_upsample_argmax(seg, h, w, H, W, want_up=False)
    return MT.contingency(gt, idx.view(gt.shape), num_true, seg.shape[-1]), idx


@pytest.mark.parametrize('h,w,H,W,N', SHAPES)
def test_tables_equal_the_composed_path_bit_for_bit(h, w, H, W, N):
    seg, gt = _seg(h, w, N).cuda(), _gt(B, H, W, 5 + N).cuda()
    want, idx = _composed(seg, gt, h, w)
    seg0, gt0 = seg.clone(), gt.clone()
    got, ids = MT.seg_tables(seg, gt, (h, w), KG, ids_dtype=torch.int32, fused=True)
    assert got.shape == (B, 1, KG + 1, N) and got.dtype == torch.int32
    assert torch.equal(got[:, 0, :KG], want) and int(got[:, 0, KG].sum()) == 0
    assert ids.shape == (B, H, W) and torch.equal(ids.long(), idx)
    assert torch.equal(seg, seg0) and torch.equal(gt, gt0)
    got8, ids8 = MT.seg_tables(seg, gt, (h, w), KG, ids_dtype=torch.uint8, fused=True)
    assert torch.equal(got8, got) and ids8.dtype == torch.uint8 and torch.equal(ids8.long(), idx)
    assert torch.equal(MT.seg_tables(seg, gt, (h, w), KG, fused=True), got)               # without the id map
    assert torch.equal(MT.seg_tables(seg, gt, (h, w), KG), got), 'every listed shape is inside the gate'
    off, ids_off = MT.seg_tables(seg, gt, (h, w), KG, ids_dtype=torch.int32, fused=False)  # the path outside the gate
    assert torch.equal(off, got) and torch.equal(ids_off, ids)


@pytest.mark.parametrize('h,w,H,W,N', SHAPES)
def test_tables_equal_a_float64_upsample(h, w, H, W, N):
    seg, gt = _seg(h, w, N), _gt(B, H, W, 7 + N)
    up = F.interpolate(seg.double().permute(0, 2, 1).reshape(B, N, h, w), size=(H, W), mode='bilinear', align_corners=False)
    idx64 = up.argmax(1)
    if N > 1:
        top = up.topk(2, dim=1).values
        close = (top[:, 0] - top[:, 1]) < MARGIN
    else:
        close = torch.zeros((B, H, W), dtype=torch.bool)
    left_out = int(close.sum())
    print(f'({h},{w},{H},{W},{N}): {left_out} of {B * H * W} pixels under the margin')
    assert left_out <= CAP * B * H * W
    gt = torch.where(close.view(B, 1, H, W), torch.full_like(gt, -1), gt)                  # left out of both tables
    want = torch.stack([torch.bincount((gt[b, 0].long() * N + idx64[b])[~close[b]].flatten(), minlength=(KG + 1) * N)
                        for b in range(B)]).view(B, 1, KG + 1, N)
    got = MT.seg_tables(seg.cuda(), gt.cuda(), (h, w), KG, fused=True).cpu().long()
    assert torch.equal(got, want)
    assert int(got.sum()) == B * H * W - left_out


def test_ties_go_to_the_lowest_slot():
    h, w, H, W, N = 8, 8, 32, 32, 7
    gt = _gt(B, H, W, 3).cuda()
    const = torch.full((B, h * w, N), 1.0 / N).cuda()
    t, ids = MT.seg_tables(const, gt, (h, w), KG, ids_dtype=torch.int32, fused=True)
    assert int(ids.abs().max()) == 0 and int(t[..., 1:].sum()) == 0 and int(t[..., 0].sum()) == B * H * W
    g = _gen(9)
    seg = 0.05 * torch.rand(B, h * w, N, generator=g)
    seg[..., 4] = seg[..., 2] = 0.4 + 0.1 * torch.rand(B, h * w, generator=g)           # two identical, dominating maps
    t, ids = MT.seg_tables(seg.cuda(), gt, (h, w), KG, ids_dtype=torch.int32, fused=True)
    assert bool((ids == 2).all()) and int(t[..., 2].sum()) == B * H * W
    for hh, ww, HH, WW, NN in SHAPES[:5]:                 # multiples of 1/8: the bilinear sums are exact, ties are common
        q = (torch.randint(0, 9, (B, hh * ww, NN), generator=g).float() / 8.0).cuda()
        gq = _gt(B, HH, WW, 11).cuda()
        want, idx = _composed(q, gq, hh, ww)
        got, ids = MT.seg_tables(q, gq, (hh, ww), KG, ids_dtype=torch.int32, fused=True)
        assert torch.equal(got[:, 0, :KG], want) and torch.equal(ids.long(), idx)
        ref = F.interpolate(q.double().cpu().permute(0, 2, 1).reshape(B, NN, hh, ww), size=(HH, WW), mode='bilinear',
                            align_corners=False)
        best = ref.max(1, keepdim=True).values
        first = ((ref == best).float().argmax(1))                                        # lowest index among the maxima
        assert int(((ref == best).sum(1) > 1).sum()) >= 30, 'the case has ties'
        assert torch.equal(ids.long().cpu(), first)


def test_calls_accumulate_and_frame_orders_agree():
    h, w, H, W, N, T, Bv = 8, 8, 32, 32, 5, 6, 3
    seg = _seg(h, w, N, frames=Bv * T).cuda()                                            # [b][t] order
    gt = _gt(Bv * T, H, W, 21).view(Bv, T, H, W).cuda()
    whole = MT.seg_tables(seg, gt, (h, w), KG, fused=True)
    assert whole.shape == (Bv, 1, KG + 1, N)
    assert whole.flatten(1).sum(1).tolist() == [T * H * W] * Bv, 'one table per video, every pixel once'
    want, _ = _composed(seg, gt.view(Bv * T, 1, H, W), h, w)
    assert torch.equal(whole[:, 0, :KG], want.view(Bv, T, KG, N).sum(1).int())
    assert len({tuple(t.flatten().tolist()) for t in whole}) == Bv, 'three distinct videos'
    # two calls on the halves continue the same tables (ground truth passed as strided slices of the whole video's)
    s4 = seg.view(Bv, T, h * w, N)
    half = MT.seg_tables(s4[:, :3].reshape(Bv * 3, h * w, N), gt[:, :3], (h, w), KG, fused=True)
    assert not torch.equal(half, whole)
    both = MT.seg_tables(s4[:, 3:].reshape(Bv * 3, h * w, N), gt[:, 3:], (h, w), KG, counts=half, fused=True)
    assert both is half and torch.equal(both, whole)
    # the stream's time-major frames
    tm = s4.transpose(0, 1).reshape(T * Bv, h * w, N)
    assert torch.equal(MT.seg_tables(tm, gt, (h, w), KG, time_major=True, fused=True), whole)
    c = None
    for t0 in range(0, T, 2):
        c = MT.seg_tables(s4[:, t0:t0 + 2].transpose(0, 1).reshape(2 * Bv, h * w, N), gt[:, t0:t0 + 2], (h, w), KG,
                          time_major=True, counts=c, fused=True)
    assert torch.equal(c, whole)
    assert torch.equal(MT.seg_tables(tm, gt, (h, w), KG, time_major=True, fused=False), whole)
    # ids outside [0, Kg) are skipped
    bad = gt.clone()
    bad[:, :, :4] = KG
    bad[:, :, 4:6] = -2
    t = MT.seg_tables(seg, bad, (h, w), KG, fused=True)
    assert t.flatten(1).sum(1).tolist() == [T * (H - 6) * W] * Bv


@pytest.mark.parametrize('h,w,H,W,N', [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_two_ground_truths_and_the_overlap_row(h, w, H, W, N):
    g = _gen(31 + N)
    seg = _seg(h, w, N).cuda()
    gt = torch.randint(0, KG, (B, 1, H, W), generator=g, dtype=torch.int32)
    sem = torch.randint(0, 4, (B, 1, H, W), generator=g, dtype=torch.int32)
    ov = (torch.rand(B, 1, H, W, generator=g) < 0.1).int()
    ov[2] = 0
    ov[2, 0, 4:9, 3:12] = 1
    got, ids = MT.seg_tables(seg, gt.cuda(), (h, w), KG, gt2=sem.cuda(), overlap=ov.cuda(), ids_dtype=torch.int32, fused=True)
    pred = ids.cpu().long().view(B, 1, H, W)
    assert got.shape == (B, 2, KG + 1, N)
    want = torch.stack([cpu_tables(gt.long(), pred, ov.long(), KG, N), cpu_tables(sem.long(), pred, ov.long(), KG, N)], 1)
    assert torch.equal(got.cpu().long(), want)
    assert torch.equal(got[:, 0, KG], got[:, 1, KG]) and int(got[:, 0, KG].sum()) == int(ov.sum())
    assert torch.equal(MT.seg_tables(seg, gt.cuda(), (h, w), KG, gt2=sem.cuda(), overlap=ov.cuda(), fused=False), got)
    for m in range(2):
        a, b = MT.scores_from_tables(got[:, m]), MT.scores_from_tables(want[:, m])
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)
    # and the public metric functions with the overlap argument, on the device
    if N > 1:
        for k, fn in (('ari', MT.ARI_metric), ('fari', MT.fARI_metric), ('miou', MT.miou_metric), ('fmiou', MT.fmiou_metric),
                      ('mbo', MT.mbo_metric)):
            val = fn(gt.view(B, H, W).long().cuda(), pred.view(B, H, W).cuda(), ov.view(B, H, W).cuda())
            assert abs(float(val) - MT.batch_scores(cpu_tables(gt.long(), pred, ov.long()))[k]) <= 1e-6, k


# ----------------------------------------------------------------------------------------------------------------------
# the stream
# ----------------------------------------------------------------------------------------------------------------------
def _video_eval(dtype):
    from tests.test_gpu_pred_tf import _model
    m = _model('SAViDiffusion', False, dtype)
    ds = extract.SyntheticVideoSegDataset(types.SimpleNamespace(resolution=(32, 32)), num_videos=2, video_len=6, seed=3,
                                          num_objects=3)
    names = ('ARI', 'fARI', 'miou', 'fmiou', 'mbo')
    return m, ds, {cl: evaluate.evaluate_video_segmentation(m, ds, batch_size=2, chunk_len=cl, metrics=names) for cl in (2, 3)}


def test_video_evaluation_equals_the_clip_encode_fp32():
    m, ds, res = _video_eval(torch.float32)
    vids = [ds.get_video(i) for i in range(2)]
    video = torch.stack([d['video'] for d in vids]).cuda()
    gt = torch.stack([d['masks'] for d in vids])
    _, masks = m.encode(video)                                                  # [B, T, N, H, W] upsampled fp32
    assert masks.shape == (2, 6, m.num_slots, 32, 32)
    pred = masks.argmax(dim=2)
    num_true = int(gt.max()) + 1
    want = MT.contingency(gt.cuda(), pred, num_true, m.num_slots).cpu()
    for cl in (2, 3):
        tabs = res[cl]['tables']
        assert len(tabs) == 1 and tabs[0].shape == (2, 1, num_true + 1, m.num_slots)
        assert torch.equal(tabs[0][:, 0, :num_true], want) and int(tabs[0][:, 0, num_true].sum()) == 0
        assert tabs[0].flatten(1).sum(1).tolist() == [6 * 32 * 32] * 2
        ref = MT.batch_scores(cpu_tables(gt, pred.cpu(), None, num_true, m.num_slots))
        for name, k in (('ARI', 'ari'), ('fARI', 'fari'), ('miou', 'miou'), ('fmiou', 'fmiou'), ('mbo', 'mbo')):
            assert abs(res[cl]['metrics'][name] - ref[k]) <= 1e-12 and res[cl]['nan_batches'][name] == 0
    assert len(pred.unique()) > 1, 'the attention map uses more than one slot'


def test_image_evaluation_equals_the_encode_masks_fp32():
    """evaluate_image_segmentation on the CLEVRTex SADiffusion: instance and semantic tables with the overlap row, from
    sdmi_seg_tables on the model's attention map, against the argmax of model.encode's upsampled masks."""
    from tests.test_gpu_model import ctx
    m, _, img = ctx()
    B, _, H, W = img.shape
    g = _gen(41)
    gt = torch.randint(0, 5, (B, H // 16, W // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2)
    sem = (gt + 1) // 2
    ov = (torch.rand(B, H, W, generator=g) < 0.05).long()
    batch = dict(img=img.cpu(), masks=gt, sem_masks=sem, inst_overlap_masks=ov)
    res = evaluate.evaluate_image_segmentation(m, [batch], metrics=('ARI', 'fARI', 'miou', 'fmiou', 'mbo'))
    pred = m.encode(img)[1].argmax(dim=1).cpu()
    want = torch.stack([cpu_tables(gt, pred, ov, 5, m.num_slots), cpu_tables(sem, pred, ov, 5, m.num_slots)], 1)
    assert torch.equal(res['tables'][0].long(), want)
    for p, t in (('inst', want[:, 0]), ('sem', want[:, 1])):
        ref = MT.batch_scores(t)
        for name, k in (('ARI', 'ari'), ('fARI', 'fari'), ('miou', 'miou'), ('fmiou', 'fmiou'), ('mbo', 'mbo')):
            assert abs(res['metrics'][f'{p}/{name}'] - ref[k]) <= 1e-12
    plain = evaluate.evaluate_image_segmentation(m, [dict(img=img.cpu(), masks=gt)])
    assert set(plain['metrics']) == {'fARI', 'miou', 'mbo'}
    assert torch.equal(plain['tables'][0][:, 0].long(), cpu_tables(gt, pred, None, 5, m.num_slots))


def test_video_evaluation_of_a_decoder_model_fp32():
    """SAVi's masks come from its decoder: argmax and sdmi_contingency per chunk, one table per video."""
    from tests.test_gpu_pred_tf import _model
    m = _model('SAVi', False, torch.float32)
    ds = extract.SyntheticVideoSegDataset(types.SimpleNamespace(resolution=(32, 32)), num_videos=2, video_len=6, seed=3,
                                          num_objects=3)
    res = {cl: evaluate.evaluate_video_segmentation(m, ds, batch_size=2, chunk_len=cl) for cl in (2, 3)}
    vids = [ds.get_video(i) for i in range(2)]
    video = torch.stack([d['video'] for d in vids]).cuda()
    gt = torch.stack([d['masks'] for d in vids])
    pm = m({'img': video})['masks']                                             # [B, T, N, 1, H, W]
    pred = pm.squeeze(-3).argmax(dim=-3).cpu()
    want = cpu_tables(gt, pred, None, int(gt.max()) + 1, pm.shape[2])
    for cl in (2, 3):
        assert torch.equal(res[cl]['tables'][0][:, 0].long(), want)
    assert res[2]['metrics'] == res[3]['metrics'] and set(res[2]['metrics']) == {'fARI', 'miou', 'mbo'}


def test_video_evaluation_does_not_depend_on_the_chunk_length_bf16():
    m, ds, res = _video_eval(torch.bfloat16)
    assert torch.equal(res[2]['tables'][0], res[3]['tables'][0])
    assert res[2]['metrics'] == res[3]['metrics']
    assert res[2]['tables'][0].flatten(1).sum(1).tolist() == [6 * 32 * 32] * 2
