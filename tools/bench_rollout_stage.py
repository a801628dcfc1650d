"""Time the rollouts of the rollout stage (slotdiffusion_amd/unroll.py) at the Physion shape -- 150 frames, 45 observed,
history 15, frame_offset 3, 8 slots of 192, 12 layers, bf16: per batch of V videos 3 V sequences of 35 steps -- on four
paths in ONE process, interleaved (medians over rounds of back-to-back rollouts between HIP events):

    feed_graph   LDMSlotFormer.unroll: the glue between steps as one sdmi_rollout_feed launch, replayed from a HIP graph
    feed_eager   the same launches issued from Python
    glue_graph   today's rollout() on the same batched streams: the composed glue (sdmi_cast2d / sdmi_igemm / sdmi_act /
                 sdmi_add_pos), replayed from a HIP graph                                     <- the yardstick
    ref_loop     the reference's loop shape: one rollout() call per offset (V sequences each), composed glue + graph

    python tools/bench_rollout_stage.py [--videos 1 4 8] [--rounds 7] [--reps 3] [--out file.json]

Reported per batch: ms per video batch, videos/s, C-ABI calls and kernels per step past the setup (sdmi_rollout_layer
issues two kernels), and the largest difference between the paths' outputs, which are compared before anything is
timed.  Two gains are kept apart: feed_graph against glue_graph is the kernel, glue_graph against ref_loop is batching the
offsets.  Weights: the deterministic fill of tests/detfill.py (the decoder is not evaluated)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import kern, ops                            # noqa: E402
from tests import slotformer_ref as R                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--videos', type=int, nargs='+', default=[1, 4, 8])
ap.add_argument('--video-len', type=int, default=150)
ap.add_argument('--obs', type=int, default=45)
ap.add_argument('--offset', type=int, default=3)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_rollout_stage.py measures on the GPU; none found')

O = args.offset
P = (args.video_len - args.obs + O - 1) // O
m = R.build(num_layers=args.layers, rollout_len=P).cuda().eval()
m.set_compute_dtype('bf16')
PATHS = {'feed_graph': (True, True), 'feed_eager': (True, False), 'glue_graph': (False, True), 'ref_loop': (False, True)}


def run(path, past):
    """past [V, O, h, N, D] -> [V, O, P, N, D]."""
    kern._ROLLOUT_FEED, m.use_graph = PATHS[path]
    V = past.shape[0]
    if path == 'ref_loop':
        return torch.stack([m.rollout(past[:, off].contiguous(), P) for off in range(O)], 1)
    return m.unroll(past.flatten(0, 1), P).unflatten(0, (V, O))


def count(path, past):
    """C-ABI calls of one eager pass of the path's launches -> (calls, kernels) per step past the setup."""
    seen, orig = [], kern.call

    def spy(fname, *a, **k):
        seen.append(fname)
        return orig(fname, *a, **k)
    graph = PATHS[path][1]
    PATHS[path] = (PATHS[path][0], False)
    kern.call = ops.call = spy
    try:
        run(path, past)
    finally:
        kern.call = ops.call = orig
        PATHS[path] = (PATHS[path][0], graph)
    rollouts = O if path == 'ref_loop' else 1
    setup = seen.index('sdmi_rollout_layer') - (0 if PATHS[path][0] else 1)      # (the composed step starts at its add_pos)
    body = len(seen) - rollouts * setup
    kernels = body + sum(f == 'sdmi_rollout_layer' for f in seen)
    by = {}
    for f in seen:
        by[f] = by.get(f, 0) + 1
    return dict(calls_per_step=body / (rollouts * P), kernels_per_step=kernels / (rollouts * P), setup_calls=setup,
                calls_by_entry=by)


res = dict(shape=dict(video_len=args.video_len, obs_frames=args.obs, history=m.history_len, frame_offset=O, pred_len=P,
                      slots=[m.num_slots, m.slot_size], layers=args.layers, dtype='bf16'),
           rounds=args.rounds, reps=args.reps, batches=[])
with torch.no_grad():
    for V in args.videos:
        g = torch.Generator().manual_seed(77 + V)
        past = torch.randn(V, O, m.history_len, m.num_slots, m.slot_size, generator=g).cuda()
        outs = {}
        for k in PATHS:                                            # warm-up (weight packing, capture) + two more
            for _ in range(3):
                outs[k] = run(k, past).clone()
            assert torch.isfinite(outs[k]).all()
        diff = {k: float((outs[k] - outs['glue_graph']).abs().max()) for k in PATHS}
        assert torch.equal(outs['feed_graph'], outs['feed_eager'])
        counts = {k: count(k, past) for k in ('feed_eager', 'glue_graph', 'ref_loop')}
        counts['feed_graph'] = counts['feed_eager']                # (the same kernels, replayed)
        times = {k: [] for k in PATHS}
        for _ in range(args.rounds):
            for k in PATHS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    run(k, past)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.reps)
        ms = {k: statistics.median(v) for k, v in times.items()}
        res['batches'].append(dict(
            videos=V, sequences=V * O, ms_per_video_batch=ms, videos_per_s={k: 1e3 * V / v for k, v in ms.items()},
            ms_rounds=times, feed_graph_over_glue_graph=ms['feed_graph'] / ms['glue_graph'],
            glue_graph_over_ref_loop=ms['glue_graph'] / ms['ref_loop'],
            calls_per_step={k: c['calls_per_step'] for k, c in counts.items()},
            kernels_per_step={k: c['kernels_per_step'] for k, c in counts.items()},
            setup_calls={k: c['setup_calls'] for k, c in counts.items()},
            calls_by_entry={k: c['calls_by_entry'] for k, c in counts.items()},
            max_abs_diff_vs_glue_graph=diff, pred_abs_max=float(outs['glue_graph'].abs().max())))
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
