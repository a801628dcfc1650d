"""Measurements of the UniPC sampler, one mode per run:

    python tools/time_unipc.py pass     [--batch 64] [--dtype bf16] [--rounds 7] [--reps 5] [--out file.json]
    python tools/time_unipc.py tail     [--batch 64] [--dtype bf16]
    python tools/time_unipc.py converge [--out file.json]

pass      graph-replayed pass times in ONE process, interleaved (medians over rounds of back-to-back replays between HIP
          events): the default 20-NFE singlestep-3 pass, multistep-3 at 20, UniPC-3 bh2 at 10 and at 20 evaluations.
tail      two eager passes each of multistep-3 / 10 and UniPC-3 / 10, to be run under a kernel trace of its own:
          dpm_step_kernel and unipc_step_kernel then appear with 20 calls each at the same shape.
converge  fp32, B = 2, the deterministic-fill weights (RANDOM weights, not a trained model): rel-L2 of the final latent
          against a 200-evaluation multistep-3 logSNR run from the same x_T, at 5 / 8 / 10 / 15 / 20 evaluations, for
          UniPC-3 bh2, UniPC-3 without corrector, multistep-3 and the default singlestep-3 (each on its default grid).
Weights: the deterministic fill of tests/detfill.py on the CLEVRTex configuration."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd.configs import clevrtex_cfg                 # noqa: E402
from slotdiffusion_amd.models import SADiffusion                   # noqa: E402
from tests.detfill import det_fill_, is_buffer_name                # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('mode', choices=('pass', 'tail', 'converge'))
ap.add_argument('--batch', type=int, default=64)
ap.add_argument('--dtype', default='bf16')
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default=None)
args = ap.parse_args()

conv = args.mode == 'converge'
B = 2 if conv else args.batch
dtype = torch.float32 if conv else {'bf16': torch.bfloat16, 'fp32': torch.float32}[args.dtype]
cfg = clevrtex_cfg()
m = SADiffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['loss_dict'],
                compute_dtype=dtype)
det_fill_(m.state_dict().items(), skip=is_buffer_name)
m = m.cuda().eval()
m.use_graph = args.mode == 'pass'
g = torch.Generator().manual_seed(77)
slots = torch.randn(B, m.num_slots, m.slot_size, generator=g).cuda()
x_T = torch.randn(B, 3, *m.latent_res, generator=g).cuda()


def sample(**kw):
    return m.dm_decoder.generate_imgs(cond=slots, batch_size=B, x_T=x_T, **kw)


def unipc(n, **kw):
    return dict(use_unipc=True, unipc_steps=n, **{'unipc_' + k: v for k, v in kw.items()})


def multistep(n, **kw):
    return dict(dpm_method='multistep', dpm_order=3, dpm_steps=n, **{'dpm_' + k: v for k, v in kw.items()})


res = dict(mode=args.mode, batch=B, dtype=str(dtype))
with torch.no_grad():
    if args.mode == 'pass':
        conf = {'default singlestep-3 / 20': dict(), 'multistep-3 / 20': multistep(20), 'UniPC-3 bh2 / 10': unipc(10),
                'UniPC-3 bh2 / 20': unipc(20)}
        for kw in conf.values():                                   # capture + two warm replays each
            for _ in range(3):
                assert torch.isfinite(sample(**kw)).all()
        times = {k: [] for k in conf}
        for _ in range(args.rounds):
            for k, kw in conf.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.reps):
                    sample(**kw)
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.reps)
        res['ms'] = {k: statistics.median(v) for k, v in times.items()}
        res['ms_rounds'] = times
    elif args.mode == 'tail':
        for kw in (multistep(10), unipc(10)):
            for _ in range(2):
                assert torch.isfinite(sample(**kw)).all()
        torch.cuda.synchronize()
    else:
        ref = sample(**multistep(200, skip_type='logSNR'))
        rel = lambda x: float((x - ref).norm() / ref.norm())
        res['weights'] = 'deterministic fill (random), not a trained model'
        res['rel_l2'] = {}
        for n in (5, 8, 10, 15, 20):
            res['rel_l2'][n] = {'UniPC-3 bh2': rel(sample(**unipc(n))),
                                'UniPC-3 no corrector': rel(sample(**unipc(n, corrector=False))),
                                'multistep-3': rel(sample(**multistep(n))),
                                'singlestep-3 (default)': rel(sample(dpm_steps=n))}
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
