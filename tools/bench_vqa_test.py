"""Time the Physion VQA test stage (slotdiffusion_amd/vqa.py) at the Physion shape -- 1200 test videos of 75 frames, 8
slots x 192, feats_dim 192, agg max, 8 tasks, 6 thresholds, batches of 128 -- for banks of W = 1 / 10 / 50 checkpoints, with
bf16 and fp32 operands, slots resident on the device, in ONE process with the stages alternating inside every round
(same box, same session; medians over rounds, the spread of the rounds reported):

    fused       one pass over the test set, one sdmi_vqa_score launch per batch for all W checkpoints and K thresholds
    composed    W passes: per checkpoint the weights loaded into the model, the test set through model.forward
                (sdmi_readout_fwd: two launches per batch), the decisions and the table in torch at the end
    reference   the reference's loop shape: K W passes of the composed forward (every threshold reloads every
                checkpoint and walks the test set again)

    python tools/bench_vqa_test.py [--rounds 5] [--out profiles/vqa_test_bench.json]

Reported per dtype, W and stage: wall-clock ms per evaluation (host work and the final device-to-host copy included: a
stage is what the user waits for), the C-ABI calls per batch of videos and the launches those calls make (the framework
kernels of the composed stages come on top).  And the kernel alone on one batch of 128, between HIP events:
sdmi_vqa_score against W sdmi_readout_fwd calls plus the thresholding and the table in torch on the ready logits.
Building the bank (stacking and packing W checkpoints) is a one-time cost, reported apart.  Weights: the deterministic
fill of tests/detfill.py, varied per checkpoint."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import kern, ops                                              # noqa: E402
from slotdiffusion_amd.vqa import DEFAULT_THRESHS, ReadoutBank, evaluate_physion_vqa, logit_cuts    # noqa: E402
from tests import readout_ref as R                                                   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--videos', type=int, default=1200)
ap.add_argument('--frames', type=int, default=75)
ap.add_argument('--batch', type=int, default=128)
ap.add_argument('--banks', type=int, nargs='+', default=[1, 10, 50])
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_vqa_test.py measures on the GPU; none found')

N, C, F, T, J = 8, 192, 192, args.frames, 8
THRESHS = list(DEFAULT_THRESHS)
K = len(THRESHS)


class ResidentSet:
    """PhysionVQATestSet's surface over slots that already sit on the device."""

    def __init__(self, n, seed=5):
        g = torch.Generator().manual_seed(seed)
        self.slots = torch.cat([torch.randn(min(200, n - s), T, N, C, generator=g) for s in range(0, n, 200)]).cuda()
        self.labels = (torch.rand(n, generator=g) > 0.5).float().tolist()
        self.task_idx = (torch.arange(n) % J).tolist()
        self.all_tasks = ['Collide', 'Contain', 'Dominoes', 'Drape', 'Drop', 'Link', 'Roll', 'Support']
        self._label = torch.tensor(self.labels).cuda()
        self._task = torch.tensor(self.task_idx).cuda()

    def __len__(self):
        return self.slots.shape[0]

    def batches(self, batch_size):
        for s in range(0, len(self), batch_size):
            yield {'slots': self.slots[s:s + batch_size], 'label': self._label[s:s + batch_size],
                   'task_idx': self._task[s:s + batch_size]}


def state_dicts(model, n):
    base = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    return [{k: ((torch.roll(v, 3 * i, 0) if k.startswith('linear1') else v) * (1.0 + 0.01 * i) if k in R.KEYS else v)
             for k, v in base.items()} for i in range(n)]


def count_calls(fn):
    n, orig = {}, kern.call

    def spy(fname, *a, **k):
        n[fname] = n.get(fname, 0) + 1
        return orig(fname, *a, **k)
    kern.call = ops.call = spy
    try:
        fn()
    finally:
        kern.call = ops.call = orig
    return n


LAUNCHES = {'sdmi_readout_fwd': 2}             # launches per C-ABI call (1 unless listed)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), rounds=v)


ds = ResidentSet(args.videos)
nb = (len(ds) + args.batch - 1) // args.batch
cuts = logit_cuts(THRESHS).cuda()
res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0),
           shape=dict(videos=len(ds), T=T, N=N, C=C, F=F, tasks=J, thresholds=K, batch=args.batch, batches=nb),
           rounds=args.rounds, reps_kernel=args.reps, dtypes={})
for dt in ('bf16', 'fp32'):
    model = R.build().cuda()
    model.set_compute_dtype(dt)
    model.eval()
    out = {}
    for W in args.banks:
        sds = state_dicts(model, W)
        t0 = time.perf_counter()
        bank = ReadoutBank.from_weights(model, sds)
        w1p, b1, w2, b2 = bank.operands()
        torch.cuda.synchronize()
        prep_ms = (time.perf_counter() - t0) * 1e3
        stages = {
            'fused': lambda: evaluate_physion_vqa(model, ds, bank, THRESHS, args.batch, fused=True),
            'composed': lambda: evaluate_physion_vqa(model, ds, bank, THRESHS, args.batch, fused=False),
            'reference_loop_shape': lambda: [evaluate_physion_vqa(model, ds, bank, [t], args.batch, fused=False)
                                             for t in THRESHS],
        }
        a, b = stages['fused'](), stages['composed']()                      # warm-up, and the two stages agree
        assert (a['table'] == b['table']).all() and a['fused'] and not b['fused']
        calls = {}
        for name, fn in stages.items():
            c = count_calls(fn)
            calls[name] = dict(c_abi_calls_per_batch={k: v / nb for k, v in c.items()},
                               launches_of_those_per_batch=sum(v * LAUNCHES.get(k, 1) for k, v in c.items()) / nb)
        # the kernel alone, one batch
        x, lab, tsk = ds.slots[:args.batch], ds._label[:args.batch], ds._task[:args.batch]
        table = torch.zeros((W, K, J), dtype=torch.int32, device='cuda')
        onehot = torch.nn.functional.one_hot(tsk, J).float()

        def k_fused():
            ops.vqa_score(x, w1p, b1, w2, b2, 'max', bank.dtype, lab, tsk, cuts, J, correct=table)

        def k_composed():
            lg = torch.stack([ops.readout_fwd(x, w1p[w], b1[w], w2[w], b2[w:w + 1], 'max', bank.dtype)['logits']
                              for w in range(W)])
            ok = (lg[:, None, :] > cuts[None, :, None]) == (lab != 0)[None, None, :]
            return (ok.float() @ onehot).to(torch.int32)

        k_fused()
        assert (table == k_composed()).all()
        times = {n: [] for n in stages}
        ktimes = dict(vqa_score=[], readout_fwd_x_W_plus_torch=[])
        for r in range(args.rounds):
            for name, fn in stages.items():                                  # alternate the stages inside every round
                if name == 'reference_loop_shape' and r >= max(2, args.rounds // 2):
                    continue                                                 # K times the composed stage: fewer rounds
                times[name].append(wall(fn))
            ktimes['vqa_score'].append(events(k_fused, args.reps))
            ktimes['readout_fwd_x_W_plus_torch'].append(events(k_composed, args.reps))
        flops = 4.0 * W * args.batch * T * N * C * F
        out[f'W={W}'] = dict(bank_prepare_ms=prep_ms, calls=calls, stage_ms={n: stats(v) for n, v in times.items()},
                             kernel_one_batch_ms={n: stats(v) for n, v in ktimes.items()},
                             kernel_one_batch_flops=flops,
                             kernel_tflops=flops / (statistics.median(ktimes['vqa_score']) * 1e-3) / 1e12)
        print(dt, W, {n: round(statistics.median(v), 3) for n, v in {**times, **ktimes}.items()}, flush=True)
    res['dtypes'][dt] = out
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
