"""Time the graph-replayed sampling pass of two solver configurations in ONE process, interleaved (DESIGN section 5:
same box, same session; medians over rounds of back-to-back replays between HIP events).

    python tools/time_sampler.py [--batch 64] [--dtype bf16] [--rounds 7] [--reps 5] [--out file.json]

A = the default 20-NFE singlestep-3 pass, B = multistep order 2 / 10 steps (override with --b-method/--b-order/--b-steps).
Weights: the deterministic fill of tests/detfill.py on the CLEVRTex configuration."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import ops                                  # noqa: E402
from slotdiffusion_amd.configs import clevrtex_cfg                 # noqa: E402
from slotdiffusion_amd.models import SADiffusion                   # noqa: E402
from tests.detfill import det_fill_, is_buffer_name                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--dtype', default='bf16')
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--b-method', default='multistep')
ap.add_argument('--b-order', type=int, default=2)
ap.add_argument('--b-steps', type=int, default=10)
ap.add_argument('--out', default=None)
args = ap.parse_args()

cfg = clevrtex_cfg()
m = SADiffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['loss_dict'],
                compute_dtype={'bf16': torch.bfloat16, 'fp32': torch.float32}[args.dtype])
det_fill_(m.state_dict().items(), skip=is_buffer_name)
m = m.cuda().eval()
m.use_graph = True
B = args.batch
g = torch.Generator().manual_seed(77)
slots = torch.randn(B, m.num_slots, m.slot_size, generator=g).cuda()
x_T = ops.nchw_to_nhwc(torch.randn(B, 3, *m.latent_res, generator=g).cuda(), torch.float32, 4)
conf = {'A': dict(), 'B': dict(steps=args.b_steps, order=args.b_order, method=args.b_method)}
with torch.no_grad():
    for kw in conf.values():                                       # capture + two warm replays each
        for _ in range(3):
            out = m._dpm_sample(x_T, slots, **kw)[0]
        assert torch.isfinite(out).all()
    times = {k: [] for k in conf}
    for _ in range(args.rounds):
        for k, kw in conf.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.reps):
                m._dpm_sample(x_T, slots, **kw)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.reps)
res = dict(batch=B, dtype=args.dtype, a='singlestep order 3, 20 steps (default)',
           b=f'{args.b_method} order {args.b_order}, {args.b_steps} steps',
           a_ms=statistics.median(times['A']), b_ms=statistics.median(times['B']),
           a_ms_rounds=times['A'], b_ms_rounds=times['B'])
res['b_over_a'] = res['b_ms'] / res['a_ms']
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
