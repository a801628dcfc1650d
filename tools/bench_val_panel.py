"""Time the slot-decomposition panel of the validation pass at the MOVi-E shape -- 128 x 128 frames, 15 slots, attention
map 32 x 32, --frames frames per video (default 24), --videos sampled videos (default 8, params.n_samples) -- on a bf16
SAViDiffusion, on two paths in ONE process, alternating inside every round (same box, same session; medians over rounds,
the spread reported):

    fused      vis.slot_panel(hard=True): ONE sdmi_slot_panel launch per video from the attention maps and the frames to
               the soft and the hard uint8 panels
    composed   vis.slot_panel_composed(hard=True): sdmi_mask_upsample_argmax, the reference's builders in torch ops, a
               make_grid per frame, the byte conversion on the device

    python tools/bench_val_panel.py [--frames 24] [--videos 8] [--rounds 7] [--reps 3] [--out profiles/val_panel_bench.json]

Reported per video: wall ms from the attention maps to both 8-bit panels ON THE HOST (a device synchronise after the
copies), bytes copied to the host, C-ABI calls (from the call log, written while counting only) and ATen operators
(a TorchDispatchMode count), and the time of the panel call alone between HIP events on the stream -- no host copy;
it still contains the Python launch overhead and, for the composed path, the gaps between its many ATen launches.  Then one tiny epoch
(--epoch-steps training steps of batch 2 x 3 frames, then a validation pass over --val-videos videos with panels and 2
sampler steps) on either path: the share of the epoch's wall time spent validating.  Both paths must give equal bytes
(asserted)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

_LOG = tempfile.NamedTemporaryFile(prefix='sdmi_calls_', suffix='.log', delete=False).name
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import _lib, configs, extract, models, vis          # noqa: E402
from slotdiffusion_amd import validate as V                                 # noqa: E402
from slotdiffusion_amd.method import Method, SyntheticDataModule           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--videos', type=int, default=8)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--epoch-steps', type=int, default=8)
ap.add_argument('--val-videos', type=int, default=2)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_val_panel.py measures on the GPU; none found')
T = args.frames
PATHS = ('fused', 'composed')


class Params(dict):
    __getattr__ = dict.get


class OpCount(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def panel(video, seg, hw, path):
    return vis.slot_panel(video, seg=seg, hw=hw, tiles=('img', 'color', 'overlay'), G=1, hard=True, fused=(path == 'fused'))


def to_host(video, seg, hw, path):
    soft, hard = panel(video, seg, hw, path)
    out = soft.cpu(), hard.cpu()
    torch.cuda.synchronize()
    return out


def wall(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def device(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def logged_calls(fn):
    n0 = sum(1 for _ in open(_LOG))
    _lib.set_call_log(_LOG)
    fn()
    _lib.set_call_log(None)
    return [ln.split('\t')[0] for ln in open(_LOG)][n0:]


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


_lib.set_call_log(None)
cfg = configs.movie_cfg()
P = Params(model='SAViDiffusion', optimizer='Adam', weight_decay=0.0, max_epochs=1, train_batch_size=2, dataset='movi',
           movi_level='e', lr=1e-4, dec_lr=2e-4, clip_grad=0.05, warmup_steps_pct=0.05, denoise_loss_w=1., input_frames=3,
           n_sample_frames=3, n_samples=args.val_videos, val_batch_size=2, eval_interval=1,
           val_sampler_kwargs=dict(dpm_steps=2), **cfg)
m = models.build_model(P).cuda()
m.set_compute_dtype('bf16')
m.eval()
hw = tuple(m.visual_resolution)
ds = extract.SyntheticVideoSegDataset(P, num_videos=args.videos, video_len=T, num_objects=10)
res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
           frames=T, videos=args.videos, resolution=list(cfg['resolution']), attention_map=list(hw), num_slots=m.num_slots,
           dtype='bf16 model; attention maps fp32, panels uint8', band_rows=vis.slot_panel_band(m.num_slots, 3, 128, 128, *hw))
with torch.no_grad():
    data = []
    for i in range(args.videos):
        video = ds.get_video(i)['video'].cuda()
        seg = m.encode_stream(video[None], None, want_seg=True)[1][:, 0].contiguous()
        data.append((video, seg))
    outs = {p: [to_host(v, s, hw, p) for v, s in data] for p in PATHS for _ in range(2)}        # (warm-up too)
    for a, b in zip(outs['fused'], outs['composed']):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'the two paths give different bytes'
    video, seg = data[0]
    calls, aten = {}, {}
    for p in PATHS:
        names = logged_calls(lambda p=p: to_host(video, seg, hw, p))
        calls[p] = dict(per_video=len(names), by_entry={n: names.count(n) for n in sorted(set(names))})
        with OpCount() as oc:
            to_host(video, seg, hw, p)
        aten[p] = oc.n
    t_wall, t_dev = {p: [] for p in PATHS}, {p: [] for p in PATHS}
    for _ in range(args.rounds):
        for p in PATHS:
            t_wall[p].append(statistics.mean(wall(lambda: to_host(v, s, hw, p), args.reps) for v, s in data))
            t_dev[p].append(device(lambda: panel(video, seg, hw, p), args.reps))
    res['per_video'] = dict(bytes_equal=True,
                            host_bytes={p: int(sum(t.numel() for t in outs[p][0])) for p in PATHS},
                            masks_to_host_panel_wall_ms={p: stats(v) for p, v in t_wall.items()},
                            panel_call_device_ms={p: stats(v) for p, v in t_dev.items()},
                            c_abi_calls=calls, aten_operators=aten)

# two tiny epochs on either path; the second (warm) one is measured: the share of its wall time spent validating
share = {}
P['max_epochs'] = 2
for p in PATHS:
    vis._PANEL_FUSED = p == 'fused'
    mm = models.build_model(P).cuda()
    mm.set_compute_dtype('bf16')
    dm = V.WithValidation(SyntheticDataModule(P, steps_per_epoch=args.epoch_steps, frames=3),
                          extract.SyntheticVideoSegDataset(P, num_videos=args.val_videos, video_len=T, num_objects=10),
                          batch_size=2)
    meth = Method(mm, dm, P)
    marks = []

    def timed_validate(*a, _inner=meth.validate, **k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = _inner(*a, **k)
        torch.cuda.synchronize()
        marks.append((t0, time.perf_counter()))
        return out
    meth.validate = timed_validate
    meth.fit()
    (a0, a1), (b0, b1) = marks                         # epoch 2 runs from the end of validation 1 to the end of validation 2
    share[p] = dict(first_validation_s=a1 - a0, epoch_s=b1 - a1, validation_s=b1 - b0, share=(b1 - b0) / (b1 - a1))
    del mm, meth
vis._PANEL_FUSED = True
res['tiny_epoch'] = dict(train_steps=args.epoch_steps, val_videos=args.val_videos, frames=T, sampler_steps=2, by_path=share)
os.unlink(_LOG)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
