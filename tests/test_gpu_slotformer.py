"""LDMSlotFormer (vp_vqa) on the GPU: fp32 parity with the reference's fixture, the fused rollout layer
(sdmi.h: sdmi_rollout_layer; csrc/rollout_layer.hip) against the per-layer launches and the fp32 restatement, pad
invariance, repeatability, the whole rollout in bf16 (HIP graph, eager, per-layer), engagement, decoding, and loading
the decoder of a SAViDiffusion checkpoint."""
import contextlib

import pytest
import torch

from tests import common as C
from tests import slotformer_ref as R

pytestmark = pytest.mark.gpu

L0 = 'rollouter.transformer_encoder.layers.0'


def _rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / b.norm())


@contextlib.contextmanager
def _mode(m, dtype='bf16', fused=True, graph=True, train=False):
    """Compute dtype / ROLLOUT_FUSED / graph switch / train mode of the shared model for one block."""
    from slotdiffusion_amd import kern
    old = (kern._ROLLOUT_FUSED, m.use_graph, m.compute_dtype)
    kern._ROLLOUT_FUSED, m.use_graph = fused, graph
    m.set_compute_dtype(dtype)
    m.train(train)
    try:
        yield m
    finally:
        kern._ROLLOUT_FUSED, m.use_graph = old[0], old[1]
        m.set_compute_dtype(old[2])
        m.eval()


@contextlib.contextmanager
def _count_calls(name='sdmi_rollout_layer'):
    from slotdiffusion_amd import kern
    n, orig = [0], kern.call

    def spy(fname, *a, **k):
        n[0] += fname == name
        return orig(fname, *a, **k)
    kern.call = spy
    try:
        yield n
    finally:
        kern.call = orig


def _layer_input(history, slots, B=2, pad=0.0, seed=5):
    L = history * slots
    Lp = (L + 63) // 64 * 64
    g = torch.Generator().manual_seed(seed + L)
    x = torch.full((B, Lp, 256), pad).bfloat16()
    x[:, :L] = torch.randn(B, L, 256, generator=g).bfloat16()
    return x, L


def test_model_fp32_matches_the_reference_fixture():
    """pred_slots <= 1e-4, loss within 1e-4 (the standing fp32 bars); gradient norms of every trainable tensor and the
    stored gradient tensors within 2e-2 (the bars of test_gpu_model._video_parity)."""
    G = C.load_golden('ldmslotformer_b2.npz')
    m = R.gpu_model(decoder=True)
    with _mode(m, 'fp32', train=True):
        m.grad_arena().zero_()
        slots = G['slots'].cuda()
        out = m(dict(slots=slots))
        loss = m.calc_train_loss(dict(slots=slots), out)['slot_recon_loss']
        loss.backward()
        torch.cuda.synchronize()
        named = dict(m.named_parameters())
        names = [str(n) for n in G['grad_norms_names']]
        mine = torch.tensor([float(named[n].grad.norm()) for n in names])
        ref = G['grad_norms']
        rel = ((mine - ref).abs() / (ref.abs() + 1e-12))[ref > 1e-6]
        errs = {}
        for k in G:
            if k.startswith('grad:'):
                g = named[k[5:]].grad
            elif k.startswith('grad_rows4:'):
                g = named[k[11:]].grad[::4]
            else:
                continue
            errs[k] = float((g.float().cpu() - G[k]).abs().max() / G[k].abs().max())
        e_pred = float((out['pred_slots'].detach().cpu() - G['pred_slots']).abs().max())
        print(f'pred_slots max err {e_pred:.3e}, loss {float(loss.detach()):.6f} vs {float(G["slot_recon_loss"]):.6f}, '
              f'grad-norm max rel {float(rel.max()):.3e}, grad tensors {errs}')
        assert tuple(out['gt_slots'].shape) == tuple(out['pred_slots'].shape) == (2, 3, 8, 192)
        assert e_pred <= 1e-4
        assert abs(float(loss.detach()) - float(G['slot_recon_loss'])) <= 1e-4
        assert len(errs) == 3 and float(rel.max()) <= 2e-2 and max(errs.values()) <= 2e-2


@pytest.mark.parametrize('history,slots', [(15, 8), (6, 7), (8, 8), (2, 8), (21, 8), (25, 8)])
def test_fused_layer_matches_per_layer_launches_and_fp32(history, slots):
    """One layer at L = 120 (padded to 128, the shipped shape), 42 (a partly filled row tile), 64 (no padding), 16
    (less than one tile of keys), 168 (Lp = 192: keys / values staged four heads at a time, twelve pieces per thread)
    and 200 (Lp = 256: four heads at a time, sixteen pieces): rel-L2 against the fp32 restatement under the fused-block
    bars of test_gpu_st_fused.py, and no worse than the per-layer bf16 launches it replaces."""
    from slotdiffusion_amd import engine
    m = R.gpu_model(decoder=True)
    x, L = _layer_input(history, slots)
    ref = R.encoder_layer(R.rollouter_weights(m), x[:, :L].float(), L0, 8)
    with _mode(m, 'bf16'), torch.no_grad():
        K = m.K()
        fused = K.rollout_layer(x.cuda(), L0, L, 8)
        assert fused is not None, 'the layer must qualify for the fused path'
        per_layer = engine.transformer_predictor(K, x[:, :L].contiguous().cuda(), 1, 8, name='rollouter')
        torch.cuda.synchronize()
    e_f, e_p = _rel(fused[:, :L], ref), _rel(per_layer, ref)
    print(f'L={L} Lp={x.shape[1]}: fused vs fp32 {e_f:.3e}, per-layer bf16 vs fp32 {e_p:.3e}')
    assert torch.isfinite(fused.float()).all()
    assert e_f < 1.5e-2
    assert e_f < 2.0 * e_p + 2e-3


@pytest.mark.parametrize('history,slots', [(15, 8), (6, 7), (25, 8)])
def test_pad_rows_never_reach_a_real_row(history, slots):
    m = R.gpu_model(decoder=True)
    x0, L = _layer_input(history, slots, pad=0.0)
    x1, _ = _layer_input(history, slots, pad=1e4)
    assert torch.equal(x0[:, :L], x1[:, :L]) and not torch.equal(x0, x1)
    with _mode(m, 'bf16'), torch.no_grad():
        y0 = m.K().rollout_layer(x0.cuda(), L0, L, 8)
        y1 = m.K().rollout_layer(x1.cuda(), L0, L, 8)
        torch.cuda.synchronize()
    assert torch.equal(y0[:, :L], y1[:, :L])
    assert torch.isfinite(y0.float()).all() and torch.isfinite(y1.float()).all()


def test_fused_layer_and_rollout_are_repeatable():
    m = R.gpu_model(decoder=True)
    x, L = _layer_input(15, 8)
    past = C.load_golden('ldmslotformer_b2.npz')['slots'][:, :15].cuda()
    with _mode(m, 'bf16', graph=False), torch.no_grad():
        xd = x.cuda()
        ys = [m.K().rollout_layer(xd, L0, L, 8) for _ in range(3)]
        ps = [m.rollout(past, 3) for _ in range(3)]
        torch.cuda.synchronize()
    assert all(torch.equal(ys[0], y) for y in ys[1:]), 'fused layer is not repeatable run to run'
    assert all(torch.equal(ps[0], p) for p in ps[1:]), 'fused rollout is not repeatable run to run'


@pytest.mark.parametrize('history', [15, 2])
def test_whole_rollout_bf16(history):
    """pred_len = 3 from 15 x 8 tokens (the fixture's input) and from 2 x 8 (the window becomes fully predicted):
    fused-graph == fused-eager bit for bit; fused no worse than the per-layer bf16 launches against the fp32 path
    (errors compound over the steps, so the bar is relative).  Measured on MI355X (rel-L2 of pred_slots against the
    fp32 path): 15 x 8: fused 6.47e-3, per-layer 7.28e-3; 2 x 8: fused 6.71e-3, per-layer 7.40e-3."""
    m = R.gpu_model(decoder=True) if history == 15 else R.gpu_model(2, 8)
    past = C.load_golden('ldmslotformer_b2.npz')['slots'][:, :history].cuda()
    with _mode(m, 'fp32'):
        ref = m.rollout(past, 3).clone()
    with _mode(m, 'bf16', graph=True):
        g1 = m.rollout(past, 3).clone()
        g2 = m.rollout(past, 3).clone()          # the replay
    with _mode(m, 'bf16', graph=False):
        eager = m.rollout(past, 3).clone()
    with _mode(m, 'bf16', fused=False):
        per_layer = m.rollout(past, 3).clone()
    torch.cuda.synchronize()
    e_f, e_p = _rel(eager, ref), _rel(per_layer, ref)
    print(f'history {history} x 8, pred_len 3: fused vs fp32 {e_f:.3e}, per-layer bf16 vs fp32 {e_p:.3e}')
    assert tuple(ref.shape) == (2, 3, 8, 192) and torch.isfinite(eager).all()
    assert torch.equal(g1, eager) and torch.equal(g2, eager)
    assert e_f < 2.0 * e_p + 2e-3


def test_fused_layer_engages_only_in_bf16_evaluation():
    m = R.gpu_model(decoder=True)
    slots = C.load_golden('ldmslotformer_b2.npz')['slots'].cuda()
    past = slots[:, :15]
    with _mode(m, 'bf16', graph=False), _count_calls() as n:
        m.rollout(past, 3)
    assert n[0] == R.LAYERS * 3
    with _mode(m, 'bf16', fused=False), _count_calls() as n:
        m.rollout(past, 3)
    assert n[0] == 0
    with _mode(m, 'fp32'), _count_calls() as n:
        m.rollout(past, 3)
    assert n[0] == 0
    with _mode(m, 'bf16', train=True), _count_calls() as n:
        out = m(dict(slots=slots))
        loss = m.calc_train_loss(dict(slots=slots), out)['slot_recon_loss']
        loss.backward()
        torch.cuda.synchronize()
    assert n[0] == 0 and out['pred_slots'].requires_grad and torch.isfinite(loss.detach())


def test_rollout_decode_matches_the_sampler_on_the_predicted_slots():
    m = R.gpu_model(decoder=True)
    past = C.load_golden('ldmslotformer_b2.npz')['slots'][:, :15].cuda()
    orig = m.dm_decoder.generate_imgs
    m.dm_decoder.generate_imgs = lambda *a, **k: orig(*a, **dict(k, dpm_steps=2))     # (2 steps keep this fast)
    try:
        with _mode(m, 'bf16', graph=False):
            torch.manual_seed(3)
            out = m.rollout(past, 3, decode=True, with_gt=False)
            pred = m.rollout(past, 3)
            torch.manual_seed(3)
            z = m.dm_decoder.generate_imgs(pred.flatten(0, 1), batch_size=6, same_noise=True, use_dpm=True)
            want = m.dm_decoder.vae.decode(z)
            torch.cuda.synchronize()
    finally:
        m.dm_decoder.generate_imgs = orig
    assert tuple(out['recon_combined'].shape) == (2, 3, 3, 128, 128)
    assert torch.equal(out['slots'], pred)
    assert torch.equal(out['recon_combined'].flatten(0, 1), want) and torch.isfinite(want).all()


def test_decoder_checkpoint_loading(tmp_path):
    """dec_dict['dec_ckp_path'] (ldm_slotformer.py:114-134): the dm_decoder tensors of a saved SAViDiffusion of the
    physion config's shape."""
    import importlib
    import json
    import os
    from slotdiffusion_amd import compat
    from tests.detfill import det_fill_, is_buffer_name
    cfg = os.path.join(C.GOLD, 'configs', 'video_based__savi_ldm_physion_params-res128.json')
    src = importlib.import_module('slotdiffusion.video_based').build_model(compat.Params(**json.load(open(cfg))))
    det_fill_(((k, v) for k, v in src.state_dict().items()),
              skip=lambda n: is_buffer_name(n) or not n.startswith('dm_decoder.'), seed=77)
    path = str(tmp_path / 'savi_ldm.pth')
    torch.save({'state_dict': src.state_dict()}, path)
    P = R.shipped_params(num_layers=1)
    P.dec_dict['dec_ckp_path'] = path
    m = importlib.import_module('slotdiffusion.vp_vqa').build_model(P)
    want = {k: v for k, v in src.state_dict().items() if k.startswith('dm_decoder.')}
    got = m.state_dict()
    assert len(want) > 800 and all(torch.equal(got[k], v) for k, v in want.items())
    assert all(not p.requires_grad for k, p in m.named_parameters() if k.startswith('dm_decoder.'))
