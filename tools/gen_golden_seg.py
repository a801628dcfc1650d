"""Record tests/golden/seg_eval_ref.npz from the reference's own segmentation metrics (build container only; never
imported by a test).

    python tools/gen_golden_seg.py

Through tools/ref_harness.py (the import route of gen_golden.py's main_metrics): img_based/models/eval_utils.py for ARI,
fARI, miou, fmiou and mbo with and without inst_overlap_mask, and video_based/models/eval_utils.py for the same ids
seen as [B, T, H, W] videos.  Inputs: B = 4 maps of 16 x 16 with at most 6 ids, holding
  image 0  a generic scene, partly overlapped;
  image 1  a ground truth that is background only (the NaN branch of hungarian_miou / mean_best_overlap);
  image 2  a prediction that uses fewer ids than the ground truth has (the M < N branch);
  image 3  an overlap region that covers EVERY pixel of the largest predicted id, so that `pred.max() + 1` is seen to be
           taken on the image before the overwrite (eval_utils.py:131-134).
Data only: ids, overlap maps and scores."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import ref_harness as rh                     # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'seg_eval_ref.npz')


def inputs():
    g = torch.Generator().manual_seed(77)
    S = 16
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing='ij')
    gt = torch.zeros((4, S, S), dtype=torch.int64)
    pred = torch.zeros((4, S, S), dtype=torch.int64)
    ov = torch.zeros((4, S, S), dtype=torch.int64)
    # image 0: four objects on a background, a noisy prediction over 6 ids, an overlap patch across two objects
    gt[0] = (yy // 8) * 2 + xx // 8 + 1
    gt[0][(yy + xx) % 7 == 0] = 0
    noise = torch.randint(0, 6, (S, S), generator=g)
    pred[0] = torch.where(torch.rand(S, S, generator=g) < 0.75, (gt[0] + 1) % 6, noise)
    ov[0, 5:11, 6:10] = 1
    # image 1: background only
    pred[1] = torch.randint(0, 4, (S, S), generator=g)
    ov[1, 0:3, 0:5] = 1
    # image 2: five ground-truth ids, two predicted ones
    gt[2] = (yy // 4 + xx // 6) % 5
    pred[2] = (xx >= 7).long()
    ov[2, 12:, 12:] = 1
    # image 3: predicted id 5 only inside the overlap region
    gt[3] = torch.where(yy < 6, 1, torch.where(xx < 9, 2, 3))
    gt[3][7:9] = 0
    pred[3] = (gt[3] + torch.randint(0, 2, (S, S), generator=g)) % 4
    pred[3, 2:6, 3:8] = 5
    ov[3, 1:7, 2:10] = 1
    assert int((pred[3] == 5).sum()) > 0 and bool((ov[3][pred[3] == 5] == 1).all()) and int(pred[3].max()) == 5
    assert int(gt.max()) <= 5 and int(pred.max()) <= 5
    return gt, pred, ov


def main():
    rh.ref_models('img_based')
    rh.ref_models('video_based')
    from slotdiffusion.img_based.models import eval_utils as ei
    from slotdiffusion.video_based.models import eval_utils as ev
    gt, pred, ov = inputs()
    G = dict(gt=gt.to(torch.int16), pred=pred.to(torch.int16), overlap=ov.to(torch.int16))
    for tag, o in (('plain', None), ('overlap', ov)):
        per = {k: [] for k in ('ari', 'fari', 'miou', 'fmiou', 'mbo')}
        for i in range(gt.shape[0]):
            a, b = ei.preproc_masks_overlap(gt[i], pred[i], None if o is None else o[i])
            per['ari'].append(float(ei.adjusted_rand_index(a[None], b[None], False)[0]))
            per['fari'].append(float(ei.adjusted_rand_index(a[None], b[None], True)[0]))
            per['miou'].append(float(ei.hungarian_miou(a.flatten(), b.flatten(), ignore_background=False)))
            per['fmiou'].append(float(ei.hungarian_miou(a.flatten(), b.flatten(), ignore_background=True)))
            per['mbo'].append(float(ei.mean_best_overlap(a.flatten(), b.flatten())))
        for k, v in per.items():
            G[f'{tag}/{k}_per_image'] = torch.tensor(v, dtype=torch.float64)
        # the batch as the metric functions see it (ARI: the one_hot widths are the batch's)
        if o is None:
            x, y = gt, pred
        else:
            x, y = gt.clone(), pred.clone()
            for i in range(gt.shape[0]):
                x[i], y[i] = ei.preproc_masks_overlap(x[i], y[i], o[i])
        G[f'{tag}/ari_batch_per_image'] = ei.adjusted_rand_index(x, y, False)
        G[f'{tag}/fari_batch_per_image'] = ei.adjusted_rand_index(x, y, True)
        args = (gt, pred) if o is None else (gt, pred, o)
        for k, fn in (('ari', ei.ARI_metric), ('fari', ei.fARI_metric), ('miou', ei.miou_metric),
                      ('fmiou', ei.fmiou_metric), ('mbo', ei.mbo_metric)):
            G[f'{tag}/{k}'] = torch.tensor(float(fn(*args)), dtype=torch.float64)
    # the same ids as two videos of two frames, T folded into the pixel axis as video_based/test_seg.py:25-30 does
    gv, pv = gt.view(2, 2, 16, 16), pred.view(2, 2, 16, 16)
    G['video/ari_per_video'] = ev.adjusted_rand_index(gv, pv, False)
    G['video/fari_per_video'] = ev.adjusted_rand_index(gv, pv, True)
    gf, pf = gv.flatten(1, 2), pv.flatten(1, 2)
    for k, fn in (('ari', ev.ARI_metric), ('fari', ev.fARI_metric), ('miou', ev.miou_metric), ('fmiou', ev.fmiou_metric),
                  ('mbo', ev.mbo_metric)):
        G[f'video/{k}'] = torch.tensor(float(fn(gf, pf)), dtype=torch.float64)
    G['video/miou_per_video'] = torch.tensor([float(ev.hungarian_miou(gf[i].flatten(), pf[i].flatten(), False)) for i in range(2)],
                                             dtype=torch.float64)
    G['video/mbo_per_video'] = torch.tensor([float(ev.mean_best_overlap(gf[i].flatten(), pf[i].flatten())) for i in range(2)],
                                            dtype=torch.float64)
    np.savez_compressed(OUT, **{k: v.numpy() for k, v in G.items()})
    print(OUT, os.path.getsize(OUT), 'bytes')
    for k, v in G.items():
        if k not in ('gt', 'pred', 'overlap'):
            print(k, v.flatten().tolist())


if __name__ == '__main__':
    main()
