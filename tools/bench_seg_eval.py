"""Time the segmentation evaluation stage at the MOVi-E shape -- 128 x 128 frames, 15 slots of 192, the shipped transformer
transition -- on a bf16 SAViDiffusion, batches of 1, 4 and 8 synthetic videos of --frames frames (default 24) with
synthetic ground truth, on two paths in ONE process, alternating inside every round (same box, same session; medians over
rounds between HIP events, the spread reported):

    stream     evaluate.stream_chunk_tables per chunk of --chunk frames: engine.encode_stream(want_seg=True), then ONE
               sdmi_seg_tables launch per chunk that adds to the video's table
    composed   model.encode on the whole clip (which writes the upsampled fp32 masks [B, T, N, H, W] through
               sdmi_mask_upsample_argmax), argmax over slots, sdmi_contingency

    python tools/bench_seg_eval.py [--frames 24] [--chunk 6] [--rounds 7] [--reps 3] [--out profiles/seg_eval_bench.json]

Reported per batch size: videos / s and ms per video batch of each path; torch.cuda.max_memory_allocated of one pass of
each path above what is allocated before it; ms per frame of the mask-to-table part ALONE on the same attention maps --
`fused` (sdmi_seg_tables, one launch per chunk), `composed` (sdmi_mask_upsample_argmax writing the masks as model.encode
does, argmax, the int32 copy, sdmi_contingency) and `composed_lean` (sdmi_mask_upsample_argmax(want_up=False), the int32
copy, sdmi_contingency: metrics.seg_tables outside the kernel's gate) --; C-ABI calls per frame of that part, from the
call log (_lib.set_call_log: written while counting only, never while timing); whether the three give equal tables (they
must: asserted); and how many pixels the two end-to-end paths place differently (the stream's transition is the fused
sdmi_pred_tf, the clip's the composed chain, so bf16 slots differ in the last bits and a pixel near a tie may flip)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

_LOG = tempfile.NamedTemporaryFile(prefix='sdmi_calls_', suffix='.log', delete=False).name
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import _lib, configs, evaluate, extract, models, ops    # noqa: E402
from slotdiffusion_amd import metrics as MT                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--chunk', type=int, default=6)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--treps', type=int, default=20)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_seg_eval.py measures on the GPU; none found')

T, CH = args.frames, args.chunk
BATCHES = (1, 4, 8)
PATHS = ('stream', 'composed')
PARTS = ('fused', 'composed', 'composed_lean')


def build():
    cfg = configs.movie_cfg()
    m = models.SAViDiffusion(cfg['resolution'], CH, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'],
                             cfg['loss_dict'], compute_dtype=torch.bfloat16)
    return m.cuda().eval(), cfg


def whole(m, video, gt, num_true, path):
    """-> int32 tables [B, Kg, N] of one batch of videos."""
    if path == 'stream':
        prev, counts = None, None
        for t0 in range(0, T, CH):
            prev, counts = evaluate.stream_chunk_tables(m, video[:, t0:t0 + CH], prev, gt[:, t0:t0 + CH], counts, num_true)
        return counts[:, 0, :num_true]
    _, masks = m.encode(video)                                            # [B, T, N, H, W] fp32
    return MT.contingency(gt, masks.argmax(dim=2), num_true, m.num_slots)


def part(seg_tm, gt, hw, num_true, which):
    """The mask-to-table part on given attention maps seg_tm [T, B, h*w, N] -> tables [B, Kg, N]."""
    B = gt.shape[0]
    H, W = gt.shape[-2:]
    if which == 'fused':
        counts = None
        for t0 in range(0, T, CH):
            counts = MT.seg_tables(seg_tm[t0:t0 + CH].flatten(0, 1), gt[:, t0:t0 + CH], hw, num_true, time_major=True,
                                   counts=counts, fused=True)
        return counts[:, 0, :num_true]
    flat = seg_tm.transpose(0, 1).reshape(B * T, seg_tm.shape[2], seg_tm.shape[3])        # [b][t] order, as the clip encode has it
    if which == 'composed':
        up, _ = ops.mask_upsample_argmax(flat, hw[0], hw[1], H, W)
        idx = up.view(B, T, -1, H, W).argmax(dim=2)
    else:
        idx = ops.mask_upsample_argmax(flat, hw[0], hw[1], H, W, want_up=False)[1].view(B, T, H, W)
    return MT.contingency(gt, idx, num_true, seg_tm.shape[3])


def logged_calls(fn):
    n0 = sum(1 for _ in open(_LOG))
    _lib.set_call_log(_LOG)
    fn()
    _lib.set_call_log(None)                  # off while timing
    return [l.split('\t')[0] for l in open(_LOG)][n0:]


def timed(fn, reps=None):
    reps = reps or args.reps
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return peak - base


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


_lib.set_call_log(None)
m, cfg = build()
hw = tuple(m.visual_resolution)
res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
           part_reps=args.treps, frames=T, chunk_len=CH, resolution=list(cfg['resolution']), attention_map=list(hw),
           num_slots=m.num_slots, slot_size=cfg['slot_dict']['slot_size'], dtype='bf16 model; attention maps and tables fp32 / int32',
           batches=[])
with torch.no_grad():
    for B in BATCHES:
        ds = extract.SyntheticVideoSegDataset(dict(resolution=cfg['resolution']), num_videos=B, video_len=T, seed=B, num_objects=10)
        items = [ds.get_video(i) for i in range(B)]
        video = torch.stack([d['video'] for d in items]).cuda()
        masks = torch.stack([d['masks'] for d in items])
        num_true = int(masks.max()) + 1
        gt = masks.to(device='cuda', dtype=torch.int32)
        outs = {}
        for p in PATHS:
            for _ in range(2):                                               # warm-up: weight preparation, code objects
                outs[p] = whole(m, video, gt, num_true, p)
        moved = int((outs['stream'] - outs['composed']).abs().sum()) // 2
        seg_tm = torch.cat([m.encode_stream(video[:, t0:t0 + CH], None, want_seg=True)[1] for t0 in range(0, T, CH)], 0)
        pouts, calls = {}, {}
        for w in PARTS:
            part(seg_tm, gt, hw, num_true, w)
            names = logged_calls(lambda w=w: pouts.__setitem__(w, part(seg_tm, gt, hw, num_true, w)))
            calls[w] = dict(per_frame=len(names) / T, by_entry={n: names.count(n) / T for n in sorted(set(names))})
        assert torch.equal(pouts['fused'], pouts['composed']) and torch.equal(pouts['fused'], pouts['composed_lean']), \
            'the three mask-to-table paths give different tables'
        assert pouts['fused'].flatten(1).sum(1).tolist() == [T * gt.shape[-2] * gt.shape[-1]] * B
        mem = {p: peak_bytes(lambda p=p: whole(m, video, gt, num_true, p)) for p in PATHS}
        mem_part = {w: peak_bytes(lambda w=w: part(seg_tm, gt, hw, num_true, w)) for w in PARTS}
        t_whole = {p: [] for p in PATHS}
        t_part = {w: [] for w in PARTS}
        for _ in range(args.rounds):
            for p in PATHS:                                                  # alternate the paths inside every round
                t_whole[p].append(timed(lambda p=p: whole(m, video, gt, num_true, p)))
            for w in PARTS:
                t_part[w].append(timed(lambda w=w: part(seg_tm, gt, hw, num_true, w), args.treps) / T)
        entry = dict(videos=B, frames=T, num_true=num_true,
                     pixels_placed_differently_stream_vs_composed=moved, pixels=B * T * gt.shape[-2] * gt.shape[-1],
                     mask_to_table_paths_equal=True,
                     ms_per_video_batch={p: stats(v) for p, v in t_whole.items()},
                     videos_per_s={p: B / statistics.median(v) * 1e3 for p, v in t_whole.items()},
                     max_memory_allocated_above_start_bytes=mem,
                     mask_to_table_ms_per_frame={w: stats(v) for w, v in t_part.items()},
                     mask_to_table_calls_per_frame=calls,
                     mask_to_table_max_memory_above_start_bytes=mem_part)
        res['batches'].append(entry)
        print(f'B{B} x {T} frames: ' + ', '.join(f'{p} {entry["videos_per_s"][p]:.2f} videos/s ({mem[p] / 2**20:.1f} MiB)' for p in PATHS) +
              '; mask-to-table ' + ', '.join(f'{w} {entry["mask_to_table_ms_per_frame"][w]["median"]:.4f} ms/frame '
                                             f'({calls[w]["per_frame"]:.2f} calls, {mem_part[w] / 2**20:.1f} MiB)' for w in PARTS) +
              f'; {moved} of {entry["pixels"]} pixels differ between the end-to-end paths', file=sys.stderr)
os.unlink(_LOG)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
