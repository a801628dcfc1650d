"""Time whole-video slot extraction at the Physion shape -- 128 x 128 frames, 8 slots of 192, the shipped transformer
transition (2 layers, 4 heads of 48, ffn 768) -- on a bf16 SAVi, batches of 1, 4 and 8 synthetic videos of --frames
frames (default 24), on three paths in ONE process, alternating inside every round (same box, same
session; medians over rounds between HIP events, the spread reported):

    fused      engine.encode_stream, the transition as one sdmi_pred_tf launch          (kern._PRED_TF on)
    composed   engine.encode_stream, the transition as engine.slot_transition's launches (kern._PRED_TF off)
    clip       model.encode on the whole clip (the per-frame LayerNorm and K/V GEMM in front of Slot Attention)

    python tools/bench_extract.py [--frames 24] [--rounds 7] [--reps 3] [--out profiles/extract_bench.json]

Reported per batch size: frames / s and ms per video batch of each path; ms per frame of the recurrence alone for the
two stream paths (engine.stream_recurrence on keys / values computed once, continuing from given slots, so that every
one of the T frames carries a transition); ms of ONE transition alone on either path (--treps back-to-back calls between
HIP events); C-ABI calls per frame of the recurrence without the T copies that stack the frames, counted from the call
log of SDMI_CALL_LOG (_lib.set_call_log: written while counting only, never while timing); and the largest difference
between the fused and the composed slots."""
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
from slotdiffusion_amd import _lib, configs, engine, extract, kern, models    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--treps', type=int, default=50)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_extract.py measures on the GPU; none found')

T = args.frames
BATCHES = (1, 4, 8)
PATHS = ('fused', 'composed', 'clip')


def build():
    cfg = configs.savi_cfg()
    cfg['slot_dict'].update(num_slots=8)
    m = models.SAVi(cfg['resolution'], T, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'],
                    cfg['loss_dict'], compute_dtype=torch.bfloat16)
    return m.cuda().eval(), cfg


def whole(m, video, path):
    kern._PRED_TF = path == 'fused'
    try:
        return m.encode(video) if path == 'clip' else m.encode_stream(video)
    finally:
        kern._PRED_TF = True


def recurrence(m, kv, prev, path):
    kern._PRED_TF = path == 'fused'
    try:
        return engine.stream_recurrence(m, kv, prev)
    finally:
        kern._PRED_TF = True


def transition(m, slots, path):
    kern._PRED_TF = path == 'fused'
    try:
        return engine.stream_transition(m.K(), slots, m.pred_dict, m.pred_state)
    finally:
        kern._PRED_TF = True


def logged_calls(fn):
    """Entry points fn issues, in order, read back from the call log."""
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


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


_lib.set_call_log(None)
m, cfg = build()
res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
           transition_reps=args.treps, frames=T, resolution=list(cfg['resolution']), num_slots=8, slot_size=cfg['slot_dict']['slot_size'],
           pred=dict(cfg['pred_dict']), dtype='bf16 model (sdmi_pred_tf: bf16 operands; composed transition: fp32 master weights)',
           batches=[])
with torch.no_grad():
    for B in BATCHES:
        ds = extract.SyntheticVideoDataset(dict(resolution=cfg['resolution']), num_videos=B, video_len=T, seed=B)
        video = torch.stack([ds.get_video(i)['video'] for i in range(B)]).cuda()
        kv = engine.stream_keys_values(m, video)
        prev = m.encode_stream(video[:, :1].contiguous())[:, 0].contiguous()      # slots to continue from
        outs, calls = {}, {}
        for p in PATHS:
            for _ in range(2):                                           # warm-up: weight preparation, code objects
                outs[p] = whole(m, video, p)
                outs[p] = outs[p][0] if isinstance(outs[p], tuple) else outs[p]
            if p != 'clip':
                recurrence(m, kv, prev, p)
                names = logged_calls(lambda p=p: recurrence(m, kv, prev, p))
                loop = [n for n in names if n != 'sdmi_cast2d']                    # (the T copies that stack the frames)
                calls[p] = dict(per_frame=len(loop) / T, by_entry={n: loop.count(n) / T for n in sorted(set(loop))})
        dev = float((outs['fused'] - outs['composed']).abs().max())
        dev_clip = float((outs['composed'] - outs['clip']).abs().max())
        t_whole = {p: [] for p in PATHS}
        t_rec = {p: [] for p in PATHS if p != 'clip'}
        t_tr = {p: [] for p in t_rec}
        last = outs['clip'][:, -1].contiguous()
        for p in t_tr:
            transition(m, last, p)
        for _ in range(args.rounds):
            for p in PATHS:                                              # alternate the paths inside every round
                t_whole[p].append(timed(lambda p=p: whole(m, video, p)))
            for p in t_rec:
                t_rec[p].append(timed(lambda p=p: recurrence(m, kv, prev, p)) / T)
                t_tr[p].append(timed(lambda p=p: transition(m, last, p), args.treps))
        entry = dict(videos=B, frames=T,
                     max_abs_diff_fused_vs_composed=dev, max_abs_diff_composed_vs_clip=dev_clip, slots_abs_max=float(outs['clip'].abs().max()),
                     calls_per_frame_of_the_recurrence=calls,
                     ms_per_video_batch={p: stats(v) for p, v in t_whole.items()},
                     frames_per_s={p: B * T / statistics.median(v) * 1e3 for p, v in t_whole.items()},
                     recurrence_ms_per_frame={p: stats(v) for p, v in t_rec.items()},
                     transition_alone_ms={p: stats(v) for p, v in t_tr.items()})
        res['batches'].append(entry)
        print(f'B{B} x {T} frames: ' + ', '.join(f'{p} {entry["frames_per_s"][p]:.0f} frames/s' for p in PATHS) +
              '; recurrence ' + ', '.join(f'{p} {entry["recurrence_ms_per_frame"][p]["median"]:.4f} ms/frame '
                                          f'({calls[p]["per_frame"]:.1f} calls)' for p in t_rec) +
              '; transition alone ' + ', '.join(f'{p} {entry["transition_alone_ms"][p]["median"]:.4f} ms' for p in t_tr) +
              f'; diff {dev:.2e}', file=sys.stderr)
os.unlink(_LOG)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
