"""Time one LDMSlotFormer rollout at the shipped shape -- B = 128, 15 burn-in frames x 8 slots -> 10 predicted frames,
12 layers, bf16 -- on the three inference paths in ONE process, interleaved (same box, same session;
medians over rounds of back-to-back rollouts between HIP events):

    fused-graph   sdmi_rollout_layer (2 launches per layer), all steps replayed from one HIP graph
    fused-eager   the same launches issued from Python
    per-layer     the per-layer launches of engine.transformer_predictor (ROLLOUT_FUSED=0), eager

    python tools/bench_rollout.py [--batch 128] [--pred-len 10] [--layers 12] [--rounds 7] [--reps 3] [--out file.json]

Launches per rollout are counted at the C ABI (one count per entry-point call; sdmi_rollout_layer issues two kernels).
The outputs of the three paths are compared (rel-L2 against the per-layer path) before anything is timed.  Weights:
the deterministic fill of tests/detfill.py (the decoder is not evaluated and keeps its initial values)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import kern                                  # noqa: E402
from tests import slotformer_ref as R                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=128)
ap.add_argument('--pred-len', type=int, default=10)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_rollout.py measures on the GPU; none found')

m = R.build(num_layers=args.layers, rollout_len=args.pred_len).cuda().eval()
m.set_compute_dtype('bf16')
B, P = args.batch, args.pred_len
past = torch.randn(B, m.history_len, m.num_slots, m.slot_size, generator=torch.Generator().manual_seed(77)).cuda()
PATHS = {'fused_graph': (True, True), 'fused_eager': (True, False), 'per_layer': (False, False)}


def run(path):
    kern._ROLLOUT_FUSED, m.use_graph = PATHS[path]
    return m.rollout(past, P)


def count_launches(path):
    n, orig = {}, kern.call

    def spy(fname, *a, **k):
        n[fname] = n.get(fname, 0) + (2 if fname == 'sdmi_rollout_layer' else 1)
        return orig(fname, *a, **k)
    import slotdiffusion_amd.ops as ops_
    kern.call = ops_.call = spy
    try:
        run(path)
    finally:
        kern.call = ops_.call = orig
    return n


with torch.no_grad():
    outs = {}
    for k in PATHS:                                                # warm-up (weight packing, capture) + two more
        for _ in range(3):
            outs[k] = run(k).clone()
        assert torch.isfinite(outs[k]).all()
    rel = {k: float((outs[k] - outs['per_layer']).norm() / outs['per_layer'].norm()) for k in PATHS}
    assert torch.equal(outs['fused_graph'], outs['fused_eager'])
    launches = {k: count_launches(k) for k in ('fused_eager', 'per_layer')}
    times = {k: [] for k in PATHS}
    for _ in range(args.rounds):
        for k in PATHS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.reps)
res = dict(batch=B, history=[m.history_len, m.num_slots], pred_len=P, layers=args.layers, dtype='bf16',
           ms={k: statistics.median(v) for k, v in times.items()}, ms_rounds=times,
           launches={k: sum(v.values()) for k, v in launches.items()}, launches_by_entry=launches,
           rel_l2_vs_per_layer=rel)
res['launches']['fused_graph'] = res['launches']['fused_eager']       # (the same kernels, replayed)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
