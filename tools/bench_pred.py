"""Time ONE slot transition of the video models at the shipped shapes -- B N in {16 x 11, 16 x 15, 64 x 7} rows with
(D, H) in {(128, 256), (192, 384), (256, 512)} -- on a bf16 model, on its two paths in ONE process, alternating (DESIGN
section 5: same box, same session; medians over rounds of back-to-back calls between HIP events, the spread reported):

    fused      sdmi_pred_step, one launch
    composed   engine.residual_mlp_predictor / engine.lstm_wrapper: sdmi_layernorm, sdmi_igemm, sdmi_lstm_cell launches
               (fp32 arithmetic on the master weights, as the model runs them when it records gradients)

    python tools/bench_pred.py [--rounds 9] [--reps 50] [--out profiles/pred_step_bench.json]

Modes: mlp (the residual MLP alone), rnn (the LSTM wrapper alone, behind a transformer whose launches are the same on
both paths and are not timed), mlp+rnn.  The state is a given (h, c) pair: the steady state of a clip, not its first
transition.  Reported per shape, mode and path: ms per transition issued eagerly and replayed from a HIP graph that
holds GRAPH_LEN back-to-back transitions (a graph of one launch would measure the replay's own cost, which a captured
clip spreads over all its launches), and the C-ABI calls per transition.  The two paths' results are compared at every
shape before timing."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import configs, engine, kern, models, ops    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--reps', type=int, default=50)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_pred.py measures on the GPU; none found')

GEOMS = [(128, 256), (192, 384), (256, 512)]
ROWS = [16 * 11, 16 * 15, 64 * 7]
BASE, WRAP = 'predictor.base_predictor', 'predictor'
GRAPH_LEN = 8
MODES = {'mlp': (BASE, None), 'rnn': (None, WRAP), 'mlp+rnn': (BASE, WRAP)}


def build(D, H):
    cfg = configs.savi_cfg()
    cfg['slot_dict'].update(slot_size=D, slot_mlp_size=H)
    cfg['enc_dict']['enc_out_channels'] = D
    cfg['dec_dict']['dec_channels'] = (D, 64, 64, 64, 64)
    cfg['pred_dict'].update(pred_type='mlp', pred_rnn=True)
    m = models.SAVi(cfg['resolution'], cfg['clip_len'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'],
                    cfg['pred_dict'], cfg['loss_dict'], compute_dtype=torch.bfloat16)
    return m.cuda().eval()


def transition(K, x, state, base, wrap, fused):
    if fused:
        out = K.pred_step(x, base, wrap, True, state)
        assert out is not None, 'the shipped geometries are inside pred_step_covers'
        return out[0]
    y = engine.residual_mlp_predictor(K, x, base, True) if base else x
    return engine.lstm_wrapper(K, y, state, wrap)[0] if wrap else y


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
    return dict(median=statistics.median(v), min=min(v), max=max(v))


res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
           graph_len=GRAPH_LEN,
           dtype='bf16 model (fused: bf16 operands; composed: fp32 master weights)', shapes=[])
with torch.no_grad():
    for D, H in GEOMS:
        m = build(D, H)
        K = m.K()
        for R in ROWS:
            g = torch.Generator().manual_seed(R + D)
            x = torch.randn(R, D, generator=g).cuda()
            state = (torch.randn(R, H, generator=g).cuda() * 0.3, torch.randn(R, H, generator=g).cuda() * 0.5)
            entry = dict(D=D, H=H, rows=R, modes={})
            for mode, (base, wrap) in MODES.items():
                st = state if wrap else None
                runs = {}
                for path, fused in (('fused', True), ('composed', False)):
                    fn = lambda fused=fused: transition(K, x, st, base, wrap, fused)
                    for _ in range(3):
                        y = fn()
                    graph = torch.cuda.CUDAGraph()
                    torch.cuda.synchronize()
                    with torch.cuda.graph(graph):
                        for _ in range(GRAPH_LEN):
                            fn()
                    runs[path] = dict(eager=fn, graph=graph.replay, y=y.clone(), calls=count_calls(fn))
                dev = float((runs['fused']['y'] - runs['composed']['y']).abs().max())
                times = {p: dict(eager=[], graph=[]) for p in runs}
                for _ in range(args.rounds):
                    for p, r in runs.items():                          # alternate the paths inside every round
                        times[p]['eager'].append(timed(r['eager']))
                        times[p]['graph'].append(timed(r['graph']) / GRAPH_LEN)
                entry['modes'][mode] = dict(
                    max_abs_diff_fused_vs_composed=dev,
                    calls={p: r['calls'] for p, r in runs.items()},
                    ms={p: {k: stats(v) for k, v in t.items()} for p, t in times.items()})
                f, c = entry['modes'][mode]['ms']['fused'], entry['modes'][mode]['ms']['composed']
                print(f'D{D} H{H} rows {R} {mode}: fused {f["eager"]["median"]:.4f} / {f["graph"]["median"]:.4f} ms, '
                      f'composed {c["eager"]["median"]:.4f} / {c["graph"]["median"]:.4f} ms (eager / graph), diff {dev:.2e}',
                      file=sys.stderr)
            res['shapes'].append(entry)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
