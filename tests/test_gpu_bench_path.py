"""The configuration bench.py TIMES -- configs[1] at B = 64, bf16 storage, HIP-graph replay, fused SpatialTransformer
blocks -- chained to the fp32 HIP path on the same weights and inputs (the fp32 path is what the oracle / reference
fixtures pin to 1e-4: tests/test_gpu_model.py, test_gpu_train.py).  VERDICT round 3, item 5a."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B = 64


def _pair():
    import bench
    mb, cfg, _ = bench.build_model(torch.bfloat16)
    mf, _, _ = bench.build_model(torch.float32)          # same seed: identical fp32 master weights
    for m in (mb, mf):
        m.train_dropout = 0.0                            # (its counter-based stream has no fp32 / bf16 twin)
    return mb.cuda(), mf.cuda(), cfg


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_train_step_b64_bf16_graph_against_fp32():
    import bench
    from slotdiffusion_amd.optim import FusedAdam, GraphedTrainStep
    mb, mf, cfg = _pair()
    assert torch.equal(mb.arena(), mf.arena())
    img = bench.synth_batch(B, 0, 'cuda')
    g = torch.Generator().manual_seed(9)
    batch = dict(img=img, t=torch.randint(0, 1000, (B,), generator=g).cuda(),
                 noise=torch.randn(B, 3, 32, 32, generator=g).cuda())
    # fp32 HIP path, eager
    mf.train()
    mf.grad_arena().zero_()
    of = mf(batch)
    loss_f = mf.calc_train_loss(batch, of)['denoise_loss']
    loss_f.backward()
    torch.cuda.synchronize()
    gf = mf.grad_arena().clone()
    # the timed form: bf16, whole step replayed from HIP graphs
    mb.train()
    opt = FusedAdam(mb, lr=1e-4, dec_lr=2e-4, clip_grad=1.0, total_steps=100000)
    step = GraphedTrainStep(mb, opt, batch)
    step(batch)
    torch.cuda.synchronize()
    loss_b = float(step.loss)
    gb = mb.grad_arena().clone()
    with torch.no_grad():
        mb.eval(), mf.eval()
        sb, mkb = mb.encode(img)
        sf, mkf = mf.encode(img)
    agree = float((mkb.argmax(1) == mkf.argmax(1)).float().mean())
    cos = float((gb.double() * gf.double()).sum() / (gb.double().norm() * gf.double().norm()))
    R = dict(loss_bf16=loss_b, loss_fp32=float(loss_f.detach()), grad_rel_l2=_rel(gb, gf), grad_cos=cos,
             grad_norm_ratio=float(gb.norm() / gf.norm()), slots_rel_l2=_rel(sb, sf), mask_agreement=agree)
    print('bench-path train step, bf16 graph vs fp32:', R)
    assert loss_b == loss_b and abs(loss_b - float(loss_f.detach())) < 0.02 * abs(float(loss_f.detach()))
    assert agree > 0.99
    # measured on MI355X: loss 1.14434 vs 1.14452, whole-arena gradient rel-L2 0.47 %, cosine 0.99999, norm ratio
    # 0.9990, mask agreement 99.8 %
    assert R['grad_cos'] > 0.999 and abs(R['grad_norm_ratio'] - 1.0) < 0.01 and R['grad_rel_l2'] < 0.02


def test_sampling_pass_b64_bf16_graph_against_fp32():
    import bench
    from slotdiffusion_amd import ops
    mb, mf, cfg = _pair()
    img = bench.synth_batch(B, 0, 'cuda')
    g = torch.Generator().manual_seed(77)
    with torch.no_grad():
        mb.eval(), mf.eval()
        slots, _ = mf.encode(img)                          # one conditioning for both
        x_T = ops.nchw_to_nhwc(torch.randn(B, 3, 32, 32, generator=g).cuda(), torch.float32, 4)
        t = torch.full((B,), 600.0).cuda()
        eb = mb._unet_eps(x_T, t, slots).float()
        ef = mf._unet_eps(x_T, t, slots).float()
        mb.use_graph, mf.use_graph = True, False
        zb = mb._dpm_sample(x_T, slots)[0].clone()
        zb2 = mb._dpm_sample(x_T, slots)[0].clone()       # graph replay
        zf = mf._dpm_sample(x_T, slots)[0].clone()
        ib = mb.dm_decoder.vae.quantize_indices(ops.nhwc_to_nchw(zb, 3))
        i_f = mf.dm_decoder.vae.quantize_indices(ops.nhwc_to_nchw(zf, 3))
    R = dict(eps_rel_l2=_rel(eb[..., :3], ef[..., :3]), latent_rel_l2=_rel(zb[..., :3], zf[..., :3]),
             code_agreement=float((ib == i_f).float().mean()), replay_equal=bool(torch.equal(zb, zb2)))
    print('bench-path 20-NFE pass, bf16 graph vs fp32:', R)
    assert torch.isfinite(zb).all() and R['replay_equal']
    assert R['eps_rel_l2'] < 0.02
    # measured on MI355X: eps rel-L2 0.99 %, final latents 0.10 %, VQ codes of the final latents 99.92 % equal
    assert R['latent_rel_l2'] < 0.02 and R['code_agreement'] > 0.99


def _bench_run(out_dir, steps, warmup, *flags):
    """One plain `bench.py` run (child process, B = 8) with --dump-outputs -> its result line."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--steps', str(steps), '--warmup', str(warmup),
                        '--batch', '8', '--dump-outputs', str(out_dir)] + list(flags),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])


def _dumped(d):
    import numpy as np
    arrays = {f[:-len('.npy')]: np.load(d / f) for f in sorted(p.name for p in d.iterdir())}
    assert all(a.dtype == np.float32 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return arrays


def test_plain_bench_run_dumps_its_last_timed_step(tmp_path):
    """A plain bench.py run reports none of the --full legs; --steps sets the number of timed steps and --dump-outputs
    writes the result of the last of them: 2 timed steps behind 1 warm-up step dump exactly what 1 timed step behind 2
    warm-up steps dumps (the same three optimiser steps, bit-repeatable), 8 timed steps dump something else, and
    ms_per_step stays the time of ONE step whether 1 or 8 are timed.  --mode sample dumps the final latents."""
    import numpy as np
    import bench
    runs, outs = {}, {}
    for tag, steps, warmup in (('s2w1', 2, 1), ('s1w2', 1, 2), ('s8w1', 8, 1)):
        out = outs[tag] = _bench_run(tmp_path / tag, steps, warmup)
        assert out['steps'] == steps and out['unit'] == 'images/s' and out['ms_per_step'] > 0 and out['finite']
        assert out['denoise'] is None and out['comm'] is None and 'roofline' not in out and 'cpu_baseline' not in out
        runs[tag] = _dumped(tmp_path / tag)
        assert sorted(runs[tag]) == ['grads', 'loss', 'params']
        assert float(runs[tag]['loss'][0]) == out['loss']
    a = runs['s2w1']
    assert a['params'].shape == a['grads'].shape == (bench.DUMP_SAMPLE,)
    assert np.isfinite(a['grads']).all() and np.abs(a['grads']).max() > 0
    for name in a:
        assert np.array_equal(a[name], runs['s1w2'][name]), name
    assert not np.array_equal(a['loss'], runs['s8w1']['loss'])
    assert not np.array_equal(a['params'], runs['s8w1']['params'])
    ratio = outs['s8w1']['ms_per_step'] / outs['s1w2']['ms_per_step']
    assert 1 / 3 < ratio < 3, ratio          # (a count that ignored --steps would move it by 8x)
    out = _bench_run(tmp_path / 'sample', 2, 1, '--mode', 'sample')
    assert out['steps'] == 2 and out['unit'] == 'image-denoise-steps/s' and out['ms_per_step'] > 0 and out['finite']
    lat = _dumped(tmp_path / 'sample')
    assert sorted(lat) == ['latents'] and lat['latents'].shape == (8, 3, 32, 32) and np.isfinite(lat['latents']).all()
