"""Time the Physion VQA readout at the shipped shapes -- B = 64 (training) / 128 (evaluation), T = 75 frames, 8 slots x
192, feats_dim 192, agg max -- in fp32 and bf16, on its two paths in ONE process, alternating (same
box, same session; medians over rounds of back-to-back calls between HIP events, the spread of the rounds reported):

    fused      sdmi_readout_fwd (2 launches, loss fused) + sdmi_readout_bwd (1 launch)
    composed   engine.readout_composed: one sdmi_igemm call for U | V, framework ops for the rest, autograd backward
               (made of what the project had before the kernels: the baseline, not the code under test)

    python tools/bench_readout.py [--rounds 9] [--reps 10] [--out profiles/readout_bench.json]

Reported per dtype and path: ms per evaluation forward (B = 128), ms per training step (forward + backward + fused
Adam, B = 64) issued eagerly and replayed from a HIP graph, and the C-ABI calls per forward / step (sdmi_readout_fwd
counts as its two launches; the framework kernels of the composed path come on top of its count).  Algorithmic bytes
and FLOPs of both paths, and of the reference's pair-gather form, come from the shapes.  Weights: the deterministic
fill of tests/detfill.py."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import kern, ops                             # noqa: E402
from slotdiffusion_amd.optim import FusedAdam, GraphedTrainStep     # noqa: E402
from tests import readout_ref as R                                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--train-batch', type=int, default=64)
ap.add_argument('--eval-batch', type=int, default=128)
ap.add_argument('--frames', type=int, default=75)
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_readout.py measures on the GPU; none found')

N, C, F, T = 8, 192, 192, args.frames
P = N * (N - 1) // 2
PATHS = {'fused': True, 'composed': False}


def work(B, elt):
    """Algorithmic FLOPs / bytes of one forward from the shapes: the fused path multiplies every slot ROW by W_a | W_b and
    reads slots + weights, writes [B, T]; the composed path does the same GEMM but writes U | V and the [B, T, P, F]
    pair tensor and reads them back; the reference's form multiplies every PAIR by W1 (P / N x the MACs) and
    materialises [B, T, P, 2C]."""
    rows = B * T * N
    return dict(fused=dict(flops=2.0 * rows * C * 2 * F, bytes=float(rows * C * elt + 2 * C * F * elt + 4 * B * T)),
                composed=dict(flops=2.0 * rows * C * 2 * F + 2.0 * B * T * P * F,
                              bytes=float(rows * C * elt + 2 * C * F * elt + 2 * 4 * rows * 2 * F + 2 * 4 * B * T * P * F)),
                reference_form=dict(flops=2.0 * B * T * P * 2 * C * F, bytes=float(2 * 4 * B * T * P * 2 * C)))


def count_calls(fn):
    n, orig = {}, kern.call

    def spy(fname, *a, **k):
        n[fname] = n.get(fname, 0) + (2 if fname == 'sdmi_readout_fwd' else 1)
        return orig(fname, *a, **k)
    import slotdiffusion_amd.optim as optim_
    kern.call = ops.call = optim_.call = spy
    try:
        fn()
    finally:
        kern.call = ops.call = optim_.call = orig
    return n


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.reps


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0), shape=dict(T=T, N=N, C=C, F=F),
           train_batch=args.train_batch, eval_batch=args.eval_batch, rounds=args.rounds, reps=args.reps, dtypes={})
for dt in ('fp32', 'bf16'):
    g = torch.Generator().manual_seed(5)
    ev = {'slots': torch.randn(args.eval_batch, T, N, C, generator=g).cuda(),
          'label': (torch.rand(args.eval_batch, generator=g) > 0.5).float().cuda()}
    tr = {'slots': torch.randn(args.train_batch, T, N, C, generator=g).cuda(),
          'label': (torch.rand(args.train_batch, generator=g) > 0.5).float().cuda()}
    runs = {}
    for path, fused in PATHS.items():
        kern._READOUT_FUSED = fused
        m = R.build().cuda()
        m.set_compute_dtype(dt)
        opt = FusedAdam(m, lr=1e-3, clip_grad=0.0, total_steps=10 ** 6, warmup_pct=0.0, min_lr_ratio=0.01)

        def fwd(m=m):
            m.eval()
            with torch.no_grad():
                return m(ev)['vqa_loss']

        def step(m=m, opt=opt):
            m.train()
            opt.zero_grad()
            out = m(tr)
            m.calc_train_loss(tr, out)['vqa_loss'].backward()
            opt.step()

        for _ in range(3):
            fwd()
            step()
        m.train()
        graphed = GraphedTrainStep(m, opt, tr, loss_key='vqa_loss')     # captured under this path's setting
        runs[path] = dict(fwd=fwd, step=step, graph=lambda graphed=graphed: graphed(tr), fused=fused, model=m)
    out = dict(work_eval=work(args.eval_batch, 4 if dt == 'fp32' else 2),
               work_train_fwd=work(args.train_batch, 4 if dt == 'fp32' else 2), launches={}, ms={})
    for path, r in runs.items():
        kern._READOUT_FUSED = r['fused']
        out['launches'][path] = dict(fwd=count_calls(r['fwd']), step=count_calls(r['step']))
    times = {p: dict(fwd=[], step_eager=[], step_graph=[]) for p in PATHS}
    for _ in range(args.rounds):
        for path, r in runs.items():                                   # alternate the paths inside every round
            kern._READOUT_FUSED = r['fused']
            times[path]['fwd'].append(timed(r['fwd']))
            times[path]['step_eager'].append(timed(r['step']))
            times[path]['step_graph'].append(timed(r['graph']))
    out['ms'] = {p: {k: stats(v) for k, v in t.items()} for p, t in times.items()}
    res['dtypes'][dt] = out
kern._READOUT_FUSED = True
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
