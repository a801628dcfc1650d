"""PhysionReadout on the GPU: the model against the reference's fixture, sdmi_readout_fwd / sdmi_readout_bwd against the
fp64 restatement (tests/readout_ref.py), tie rules, bf16 operands, the fused loss, the composed path and engagement,
repeatability, Method.fit (eager and HIP graph) against torch.optim.Adam on the CPU, and the rollout -> readout pipeline.

Bars: fp32 results 1e-5 absolute on logits and loss, gradients 1e-5 of each gradient tensor's largest magnitude (about
8 - 15 x the fp32-vs-fp64 noise of the reference's own arithmetic at these shapes, 10 x inside the project's 1e-4 bar).
Kernel-level gradient tests feed an explicit all-positive dlogit (with BCE at small B the bias gradients cancel)."""
import functools
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

from slotdiffusion_amd import kern, ops
from tests import common as C
from tests import readout_ref as R

pytestmark = pytest.mark.gpu

# (B, T, N, C, F): the minimum of everything; N = 3; an odd N; the shipped dimensions; the shipped T (frame-tile tails);
# every upper bound (P = 120)
SHAPES = [(1, 1, 2, 32, 32), (2, 3, 3, 64, 32), (4, 7, 5, 96, 64), (3, 5, 8, 192, 192), (2, 75, 8, 192, 192),
          (5, 33, 16, 256, 256)]
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def case(shape, agg):
    """Weights, gap-conditioned slots and the fp64 results of one (shape, agg), computed once per session."""
    B, T, N, Cc, Ff = shape
    W = R.det_weights(N, Cc, Ff)
    slots = R.gapped_slots(W, (B, T, N, Cc), agg, seed=100 * B + T)
    W64 = {k: v.double() for k, v in W.items()}
    fr = R.frame_logits(W64, slots.double(), agg)
    return W, slots, fr


def pack(W, op):
    w1 = W['linear1.weight']
    Ff, C2 = w1.shape
    idx = kern.readout_pack_index(C2 // 2, Ff, op, 'cuda')
    return w1.cuda().to(op).reshape(-1)[idx].contiguous()


def run_fwd(W, slots, agg, op=torch.float32, label=None, lw=1.0):
    f = lambda k: W[k].cuda().reshape(-1).contiguous()
    return ops.readout_fwd(slots, pack(W, op), f('linear1.bias'), f('linear2.weight'), f('linear2.bias'), agg, op,
                           label=label, loss_weight=lw)


def run_bwd(W, slots, agg, t_star, dlogit, op=torch.float32, **kw):
    f = lambda k: W[k].cuda().reshape(-1).contiguous()
    return ops.readout_bwd(slots, pack(W, op), f('linear1.bias'), f('linear2.weight'), t_star, dlogit, agg, op, **kw)


def gpu_model(agg='max', **over):
    m = R.build(agg_func=agg, **over).cuda()
    m.set_compute_dtype('fp32')
    return m


# ---- 1
@pytest.mark.parametrize('agg', R.AGGS)
def test_model_fp32_matches_the_reference_fixture(agg):
    G = C.load_golden('physion_readout_b3.npz')
    m = gpu_model(agg).train()
    data = {'slots': G['slots'].cuda(), 'label': G['label'].cuda()}
    m.grad_arena().zero_()
    out = m(data)
    loss = m.calc_train_loss(data, out)['vqa_loss']
    loss.backward()
    torch.cuda.synchronize()
    e_l = float((out['logits'].detach().cpu() - G[f'{agg}:logits']).abs().max())
    e_loss = abs(float(loss.detach()) - float(G[f'{agg}:vqa_loss']))
    print(f'{agg}: logits {e_l:.2e} loss {e_loss:.2e}')
    assert e_l <= TOL and e_loss <= TOL
    ev = m.calc_eval_loss(data, {k: v.detach() for k, v in out.items()})
    assert list(ev) == ['vqa_loss', 'acc_0.10', 'acc_0.30', 'acc_0.50', 'acc_0.70', 'acc_0.90']
    for k, v in ev.items():
        assert abs(float(v) - float(G[f'{agg}:{k}'])) <= TOL, k
    named = dict(m.named_parameters())
    for k in R.KEYS:
        got = named[k].grad.cpu()
        ref = G[f'{agg}:grad_rows4:{k}'] if k == 'linear1.weight' else G[f'{agg}:grad:{k}']
        got = got[::4] if k == 'linear1.weight' else got
        e = float((got - ref).abs().max())
        print(f'  grad {k}: {e:.2e} of {float(ref.abs().max()):.2e}')
        assert e <= TOL * float(ref.abs().max()), k


# ---- 2
@pytest.mark.parametrize('agg', R.AGGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_fwd_fp32_against_fp64(shape, agg):
    """The largest case, (5, 33, 16, 256, 256) with agg = sum, reaches |logit| = 103 (one fp32 ulp is 7.6e-6).  fp32
    arithmetic throughout -- the reference's own, or fp32 U, V under an fp64 aggregate -- is 2.6e-5 from fp64 there, which
    is why the kernel carries the 8-k chunks of its fp32 GEMM and the aggregate in fp64: 5.8e-6 measured on one MI355X,
    every other case within 2.3e-6."""
    W, slots, fr = case(shape, agg)
    tgap, pgap = R.gaps(W, slots, agg)
    assert tgap >= 1e-3 and pgap >= 1e-4                      # the inputs' gap condition
    r = run_fwd(W, slots.cuda(), agg)
    e_f = float((r['frame_logits'].cpu().double() - fr).abs().max())
    e_l = float((r['logits'].cpu().double() - fr.max(1)[0]).abs().max())
    print(f'{shape} {agg}: frame_logits {e_f:.2e} logits {e_l:.2e} (|logit| <= {float(fr.abs().max()):.1f})')
    assert e_f <= TOL and e_l <= TOL
    assert r['t_star'].dtype == torch.int32 and torch.equal(r['t_star'].cpu().long(), fr.argmax(1))
    assert r['loss'] is None and r['dlogit'] is None


# ---- 3
def test_tie_rules():
    W = R.det_weights(8, 192, 192)
    slots = torch.randn(3, 6, 8, 192, generator=torch.Generator().manual_seed(3))
    fr = R.frame_logits({k: v.double() for k, v in W.items()}, slots.double(), 'max')
    best = fr.argmax(1)
    for b in range(3):                                         # a copy of the winning frame at another position
        other = (int(best[b]) + 2) % 6
        slots[b, other] = slots[b, int(best[b])]
    slots[2] = slots[2, 0, 0]                                   # a sample whose slots are all equal
    r = run_fwd(W, slots.cuda(), 'max')
    want = [min(int(best[b]), (int(best[b]) + 2) % 6) for b in range(2)] + [0]
    assert r['t_star'].cpu().tolist() == want
    fl = r['frame_logits'].cpu()
    assert torch.equal(fl[2], fl[2, 0].expand(6)) and torch.isfinite(fl).all()
    g = run_bwd(W, slots.cuda(), 'max', r['t_star'], torch.ones(3, device='cuda'))
    assert all(torch.isfinite(x).all() for x in g)
    # all pairs tie in the all-equal sample: the first pair (0, 1) takes the gradient -- identical rows, so only
    # the total is observable: dW1[f] = w2[f] [s | s]
    g2 = run_bwd(W, slots[2:].cuda(), 'max', r['t_star'][2:], torch.ones(1, device='cuda'))
    s = slots[2, 0, 0]
    ref = W['linear2.weight'].reshape(-1, 1) * torch.cat([s, s]).reshape(1, -1)
    assert float((g2[0].cpu() - ref).abs().max()) <= TOL * float(ref.abs().max())


# ---- 4
@pytest.mark.parametrize('agg', R.AGGS)
@pytest.mark.parametrize('stored', ['fp32', 'bf16'])
@pytest.mark.parametrize('shape', [(4, 7, 5, 96, 64), (3, 5, 8, 192, 192)])
def test_bf16_operands_against_fp64_on_rounded_inputs(shape, stored, agg):
    W, slots, _ = case(shape, agg)
    Wr = {k: v.double() for k, v in W.items()}
    Wr['linear1.weight'] = W['linear1.weight'].bfloat16().double()
    fr = R.frame_logits(Wr, slots.bfloat16().double(), agg)
    x = slots.cuda().bfloat16() if stored == 'bf16' else slots.cuda()
    r = run_fwd(W, x, agg, op=torch.bfloat16)
    e_f = float((r['frame_logits'].cpu().double() - fr).abs().max())
    e_l = float((r['logits'].cpu().double() - fr.max(1)[0]).abs().max())
    print(f'{shape} {agg} slots stored {stored}: frame_logits {e_f:.2e} logits {e_l:.2e}')
    assert e_f <= TOL and e_l <= TOL


# ---- 5
@pytest.mark.parametrize('agg', R.AGGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_bwd_against_fp64_autograd(shape, agg):
    W, slots, fr = case(shape, agg)
    B = shape[0]
    dlogit = 0.25 + torch.rand(B, generator=torch.Generator().manual_seed(11))
    ref = R.grads({k: v.double() for k, v in W.items()}, slots.double(), None, agg, dlogit=dlogit.double())
    t_star = fr.argmax(1).int().cuda()
    got = run_bwd(W, slots.cuda(), agg, t_star, dlogit.cuda())
    for k, g in zip(R.KEYS, got):
        r = ref[k].reshape(g.shape)
        e = float((g.cpu().double() - r).abs().max())
        print(f'{shape} {agg} {k}: {e:.2e} of {float(r.abs().max()):.2e}')
        assert e <= TOL * float(r.abs().max()), k
    # accumulate adds to what is there; gscale is a device scalar on dlogit
    base = [torch.full_like(g, 0.5) for g in got]
    run_bwd(W, slots.cuda(), agg, t_star, dlogit.cuda(), gscale=torch.full((1,), 2.0, device='cuda'), out=base,
            accumulate=True)
    for g, b in zip(got, base):
        assert float((b - (0.5 + 2.0 * g)).abs().max()) <= 1e-6 * max(1.0, float(g.abs().max()))


# ---- 6
@pytest.mark.parametrize('labels', ['zeros', 'ones', 'mixed'])
def test_fused_loss_and_dlogit(labels):
    shape = (5, 33, 16, 256, 256)
    W, slots, fr = case(shape, 'mean')
    B = shape[0]
    y = {'zeros': torch.zeros(B), 'ones': torch.ones(B), 'mixed': torch.tensor([1., 0., 0., 1., 1.])}[labels]
    lw = 0.7
    r = run_fwd(W, slots.cuda(), 'mean', label=y.cuda(), lw=lw)
    x = r['logits'].cpu().double().requires_grad_(True)         # the loss of the logits the kernel produced
    ref = lw * F.binary_cross_entropy_with_logits(x, y.double())
    (dref,) = torch.autograd.grad(ref, x)
    assert abs(float(r['loss']) - float(ref)) <= 1e-6
    assert float((r['dlogit'].cpu().double() - dref).abs().max()) <= 1e-6
    # extreme logits through the finisher alone: the stable form neither overflows nor loses the tail
    big = torch.tensor([[-90., -100.], [50., 88.], [0., -1e-3], [30., 20.], [-20., -30.]], device='cuda')
    r2 = ops.readout_finish(big, y.cuda(), 1.0)
    x2 = big.cpu().double().max(1)[0].requires_grad_(True)
    ref2 = F.binary_cross_entropy_with_logits(x2, y.double())
    (d2,) = torch.autograd.grad(ref2, x2)
    assert r2['t_star'].cpu().tolist() == [0, 1, 0, 0, 0]
    assert abs(float(r2['loss']) - float(ref2)) <= 1e-6 * max(1.0, float(ref2))
    assert float((r2['dlogit'].cpu().double() - d2).abs().max()) <= 1e-6


# ---- 7
def _spy(fn):
    seen, orig = {}, kern.call

    def spy(fname, *a, **k):
        seen[fname] = seen.get(fname, 0) + 1
        return orig(fname, *a, **k)
    kern.call = ops.call = spy
    try:
        out = fn()
    finally:
        kern.call = ops.call = orig
    return out, seen


def _train_step(m, data):
    m.grad_arena().zero_()
    out = m(data)
    loss = m.calc_train_loss(data, out)['vqa_loss']
    loss.backward()
    torch.cuda.synchronize()
    return out['logits'].detach().clone(), loss.detach().clone(), m.grad_arena().clone()


@pytest.mark.parametrize('agg', R.AGGS)
def test_fused_matches_composed_and_engages(agg):
    G = C.load_golden('physion_readout_b3.npz')
    data = {'slots': G['slots'].cuda(), 'label': G['label'].cuda()}
    m = gpu_model(agg).train()
    assert kern._READOUT_FUSED is True
    (lf, lossf, gf), seen = _spy(lambda: _train_step(m, data))
    assert seen.get('sdmi_readout_fwd') == 1 and seen.get('sdmi_readout_bwd') == 1 and 'sdmi_igemm' not in seen
    kern._READOUT_FUSED = False
    try:
        (lc, lossc, gc), seen = _spy(lambda: _train_step(m, data))
    finally:
        kern._READOUT_FUSED = True
    assert 'sdmi_readout_fwd' not in seen and 'sdmi_readout_bwd' not in seen and seen.get('sdmi_igemm', 0) >= 1
    print(f'{agg}: fused vs composed logits {float((lf - lc).abs().max()):.2e} loss {abs(float(lossf - lossc)):.2e} '
          f'grads {float((gf - gc).abs().max()):.2e} of {float(gc.abs().max()):.2e}')
    assert float((lf - lc).abs().max()) <= TOL and abs(float(lossf - lossc)) <= TOL
    assert float((gf - gc).abs().max()) <= TOL * float(gc.abs().max())


def test_uncovered_geometry_runs_composed_and_matches():
    m = gpu_model('max', num_slots=20).train()                  # N = 20: outside the kernels' 2 <= N <= 16
    W = R.weights_of(m)
    g = torch.Generator().manual_seed(9)
    slots, label = torch.randn(2, 4, 20, 192, generator=g), torch.tensor([0., 1.])
    data = {'slots': slots.cuda(), 'label': label.cuda()}
    (logits, loss, grads), seen = _spy(lambda: _train_step(m, data))
    assert 'sdmi_readout_fwd' not in seen and 'sdmi_readout_bwd' not in seen and seen.get('sdmi_igemm', 0) >= 1
    W64 = {k: v.double() for k, v in W.items()}
    ref = R.forward_pairs(W64, slots.double(), 'max')
    assert float((logits.cpu().double() - ref).abs().max()) <= TOL
    assert abs(float(loss) - float(R.vqa_loss(ref, label.double()))) <= TOL
    gref = R.grads(W64, slots.double(), label.double(), 'max')
    for k, p in m.named_parameters():
        e = float((p.grad.cpu().double() - gref[k]).abs().max())
        assert e <= TOL * float(gref[k].abs().max()), k


# ---- 8
@pytest.mark.parametrize('op', [torch.float32, torch.bfloat16])
def test_forward_and_backward_are_bit_repeatable(op):
    shape = (2, 75, 8, 192, 192)
    W, slots, _ = case(shape, 'max')
    x, y = slots.cuda(), torch.tensor([1., 0.], device='cuda')
    runs = []
    for _ in range(2):
        r = run_fwd(W, x, 'max', op=op, label=y)
        g = run_bwd(W, x, 'max', r['t_star'], r['dlogit'], op=op)
        runs.append([r[k].clone() for k in ('frame_logits', 'logits', 't_star', 'loss', 'dlogit')] + list(g))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*runs))


# ---- 9
def _cpu_fit(P, steps):
    """The same steps with the restatement under torch.optim.Adam on the base schedule (cosine from lr to lr / 100 over
    max_epochs x steps-per-epoch optimiser steps, no warm-up; the scheduler steps after the optimiser)."""
    m = R.build(**{'train_batch_size': P.train_batch_size, 'video_len': P.video_len})
    W = {k: v.clone().requires_grad_(True) for k, v in R.weights_of(m).items()}
    dm = type(importlib.import_module('slotdiffusion.vp_vqa').build_dataset(P))(P, device='cpu')
    total = P.max_epochs * len(dm)
    opt = torch.optim.Adam([W[k] for k in R.KEYS], lr=P.lr)
    hist = []
    for it, batch in zip(range(steps), dm.train_loader(0)):
        for grp in opt.param_groups:
            grp['lr'] = P.lr * (0.01 + 0.99 * 0.5 * (1. + math.cos(math.pi * it / total)))
        opt.zero_grad()
        loss = R.vqa_loss(R.forward_pairs(W, batch['slots'], 'max'), batch['label'])
        loss.backward()
        opt.step()
        hist.append(float(loss.detach()))
    return hist


def test_fit_eager_and_graph_match_cpu_adam():
    task = importlib.import_module('slotdiffusion.vp_vqa')
    P = R.shipped_params(train_batch_size=4, video_len=6, max_epochs=1)
    hists = {}
    for graph in (False, True):
        m = gpu_model('max', train_batch_size=4, video_len=6)
        meth = task.build_method(model=m, datamodule=task.build_dataset(P), params=P)
        meth.use_graph = graph
        seen = []                                  # (a replayed graph hands back ONE loss tensor: read it step by step)
        m._training_step_end = lambda method=None: seen.append(float(method.history[-1]))
        meth.fit(max_steps=4)
        torch.cuda.synchronize()
        hists[graph] = seen
        assert len(seen) == 4 and meth.optimizer.step_count == 4
    ref = _cpu_fit(P, 4)
    print('eager', hists[False], 'graph', hists[True], 'cpu', ref)
    assert max(abs(a - b) for a, b in zip(hists[False], hists[True])) <= 1e-6
    for h in hists.values():
        assert max(abs(a - b) for a, b in zip(h, ref)) <= TOL


# ---- 10
def test_rollout_to_readout_pipeline():
    from tests import slotformer_ref as SF
    sf = SF.gpu_model(decoder=False)
    past = torch.randn(2, 15, 8, 192, generator=torch.Generator().manual_seed(21)).cuda()
    with torch.no_grad():
        slots = torch.cat([past, sf.rollout(past, 4)], 1)
    assert tuple(slots.shape) == (2, 19, 8, 192)
    m = gpu_model('max').eval()
    label = torch.tensor([1., 0.], device='cuda')
    with torch.no_grad():
        out = m({'slots': slots, 'label': label})
        ev = m.calc_eval_loss({'label': label}, out)
    W64 = {k: v.double() for k, v in R.weights_of(m).items()}
    fr = R.frame_logits(W64, slots.cpu().double(), 'max')
    assert float((out['frame_logits'].cpu().double() - fr).abs().max()) <= TOL
    assert float((out['logits'].cpu().double() - fr.max(1)[0]).abs().max()) <= TOL
    assert abs(float(ev['vqa_loss']) - float(R.vqa_loss(fr.max(1)[0], label.cpu().double()))) <= TOL
    assert not out['logits'].requires_grad and set(ev) >= {'vqa_loss', 'acc_0.50'}
