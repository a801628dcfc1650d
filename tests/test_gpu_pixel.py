"""The image-space sampler tails on the GPU (sdmi_dpm_step_px, sdmi_unipc_step_px): data prediction, correction of x0
(none / clamp / dynamic thresholding by a radix select) and the solver update in one launch, bit for bit against the
composed chain ops.thresh_chain + the sdmi_lincomb updates, which is the reference's op sequence
(DPM_Solver.dynamic_thresholding_fn: torch abs / quantile / maximum / clamp / div)."""
import pytest
import torch

from slotdiffusion_amd import dpm
from tests.test_gpu_dpm_family import MODES, _update_of
from tests.test_gpu_unipc import _record, _same

pytestmark = pytest.mark.gpu

TARGETS = ('eps', 'x0', 'v')
CORRECT = ('none', 'clamp', 'dynamic')
DPM_MODES = ('none', 'first', 'single', 'multi3')
UNIPC_ORDERS = ((0, 1), (3, 3), (3, 0))                  # (corrector, predictor)
# rows per sample -> kernel: 256, 1024, 1023 -> one row per thread (fewer rows than threads, full, partial); 48 * 48 = 2304
# -> four rows per thread, the third row vector partial, the fourth empty; 100 * 100 = 10000 -> sixteen rows per thread, the
# tenth partial, the rest empty (128 * 128, all sixteen full: test_guard_row_and_limits)
SIZES = ((16, 16), (32, 32), (33, 31), (48, 48), (100, 100))
SMALL, HEAVY, EIGHTHS, CONST, NAN, PLAIN = range(6)      # the samples of a batch
RATIO, MAX_VAL = 0.995, 1.0


def _batch(h, w, target, e, g, B=6):
    """x, out [B,h,w,4] whose data predictions are, per sample: all |x0| < 1 (s is exactly max_val), heavy-tailed
    (s > 1), multiples of 1/8 (many duplicates straddle the two ranks), constant, one NaN, unconstrained."""
    x = torch.randn(B, h, w, 4, generator=g) * 2.
    out = torch.randn(B, h, w, 4, generator=g) * 2.
    want = {SMALL: torch.rand(h, w, 3, generator=g) * 1.8 - 0.9,
            EIGHTHS: torch.randint(-24, 25, (h, w, 3), generator=g).float() / 8.,
            CONST: torch.full((h, w, 3), 1.375)}
    for b, d in want.items():
        if b >= B:
            continue
        if target == 'eps':                              # x0 = (x - sigma * out) / alpha
            x[b, ..., :3], out[b, ..., :3] = d * e['alpha'], 0.
        elif target == 'x0':                             # x0 = out up to rounding
            out[b, ..., :3] = d
        else:                                            # x0 = alpha * x - sigma * out up to rounding
            x[b, ..., :3], out[b, ..., :3] = d / e['alpha'], 0.
    if B > HEAVY:
        x[HEAVY] *= torch.exp(torch.randn(h, w, 1, generator=g))
    if B > NAN:
        x[NAN, h // 2, w // 3, 1] = float('nan')
    x[..., 3] = 0.
    return x.cuda(), out.cuda()


def _rows(shape, g, std=0.5):
    t = torch.randn(*shape, generator=g) * std
    t[..., 3] = 0.
    return t.cuda()


def _nanpad(out):
    o = out.clone()
    o[..., 3] = float('nan')                             # the pad channel of the network output is never read
    return o


def _check_batch(ops, m0, m0_c, x, out, e, target, correct):
    """What the samples were built to exercise, read off the chain's result."""
    assert not torch.isnan(m0_c[[b for b in range(m0_c.shape[0]) if b != NAN]]).any()
    if correct != 'dynamic':
        return
    plain = ops.thresh_chain(x, out, e, target=target, correct='none')
    assert torch.equal(m0_c[SMALL], plain[SMALL])                        # s = max_val = 1: x / 1
    assert (m0_c[HEAVY].abs() == 1).any() and not torch.equal(m0_c[HEAVY], plain[HEAVY].clamp(-1, 1))   # s > 1
    assert torch.isnan(m0_c[NAN][..., :3]).all() and (m0_c[NAN][..., 3] == 0).all()
    assert torch.isnan(m0[NAN][..., :3]).all()


@pytest.mark.parametrize('correct', CORRECT)
@pytest.mark.parametrize('mode', DPM_MODES)
@pytest.mark.parametrize('target', TARGETS)
def test_dpm_step_px_equals_the_chain(target, mode, correct):
    from slotdiffusion_amd import ops
    upd, e = (None, _update_of(dpm.UPD_FIRST)[1]) if mode == 'none' else _update_of(MODES[mode])
    g = torch.Generator().manual_seed(101 + 7 * TARGETS.index(target) + DPM_MODES.index(mode))
    for h, w in SIZES:
        x, out = _batch(h, w, target, e, g)
        base, h1, h2 = (_rows(x.shape, g) for _ in range(3))
        kw = dict(target=target, correct=correct, ratio=RATIO, max_val=MAX_VAL, upd=upd, base=base, h1=h1, h2=h2)
        m0_c, y_c = ops.dpm_step_px(x, out, e, fused=False, **kw)
        m0, y = ops.dpm_step_px(x, _nanpad(out), e, **kw)
        torch.cuda.synchronize()
        assert _same(m0, m0_c) and (m0[..., 3] == 0).all()
        _check_batch(ops, m0, m0_c, x, out, e, target, correct)
        if upd is None:
            assert y is None and y_c is None
        else:
            assert _same(y, y_c) and (y[..., 3] == 0).all()
            assert _same(y[..., :3], dpm.update_expr(upd, base, m0_c, h1, h2)[..., :3])


@pytest.mark.parametrize('correct', CORRECT)
@pytest.mark.parametrize('orders', UNIPC_ORDERS, ids=[f'c{c}p{p}' for c, p in UNIPC_ORDERS])
@pytest.mark.parametrize('target', TARGETS)
def test_unipc_step_px_equals_the_chain(target, orders, correct):
    from slotdiffusion_amd import ops
    rec = _record(*orders)
    g = torch.Generator().manual_seed(211 + 7 * TARGETS.index(target) + UNIPC_ORDERS.index(orders))
    for h, w in SIZES:
        x, out = _batch(h, w, target, rec['e'], g)
        h1, h2, h3 = (_rows(x.shape, g) for _ in range(3))
        base = _rows(x.shape, g, 1.0) if rec['corr'] else x
        kw = dict(target=target, correct=correct, ratio=RATIO, max_val=MAX_VAL, base=base, h1=h1, h2=h2, h3=h3)
        m0_c, xc_c, y_c = ops.unipc_step_px(x, out, rec, fused=False, **kw)
        m0, xc, y = ops.unipc_step_px(x, _nanpad(out), rec, **kw)
        torch.cuda.synchronize()
        assert _same(m0, m0_c) and (m0[..., 3] == 0).all()
        _check_batch(ops, m0, m0_c, x, out, rec['e'], target, correct)
        for got, want, on in ((xc, xc_c, orders[0]), (y, y_c, orders[1])):
            if not on:
                assert got is None and want is None
                continue
            assert _same(got, want) and (got[..., 3] == 0).all()


@pytest.mark.parametrize('ratio', (0.995, 0.5, 1.0, 0.0))
def test_quantile_positions(ratio):
    """Other positions of the select: the median of an odd count (weight exactly 0), the maximum, the minimum."""
    from slotdiffusion_amd import ops
    e = _update_of(dpm.UPD_FIRST)[1]
    g = torch.Generator().manual_seed(5)
    for h, w in SIZES:
        x, out = _batch(h, w, 'eps', e, g, B=4)
        x[CONST] = torch.randn(h, w, 4, generator=g).cuda() * 3
        x[..., 3] = 0.
        for max_val in (1.0, 0.25):
            kw = dict(correct='dynamic', ratio=ratio, max_val=max_val)
            m0_c, _ = ops.dpm_step_px(x, out, e, fused=False, **kw)
            m0, _ = ops.dpm_step_px(x, out, e, **kw)
            assert _same(m0, m0_c)


def test_guard_row_and_limits():
    """B = 2 at 128 x 128, the register-resident limit (16 rows per thread), with a guard row past the end of every
    output; one row more per sample is refused with its own code before any launch, and the wrapper's fallback is the
    chain."""
    from slotdiffusion_amd import _lib, ops
    upd, e = _update_of(dpm.UPD_MULTI3)
    g = torch.Generator().manual_seed(9)
    x, out = _batch(128, 128, 'eps', e, g, B=2)
    base, h1, h2 = (_rows(x.shape, g) for _ in range(3))
    kw = dict(target='eps', correct='dynamic', ratio=RATIO, max_val=MAX_VAL, upd=upd, base=base, h1=h1, h2=h2)
    m0_c, y_c = ops.dpm_step_px(x, out, e, fused=False, **kw)
    R = x.numel() // 4
    assert R // 2 == ops.PX_MAX_ROWS
    gm, gy = torch.full((R + 1, 4), 7.0).cuda(), torch.full((R + 1, 4), 7.0).cuda()
    k, wq = ops.quantile_rank(3 * (R // 2), RATIO)
    _lib.call('sdmi_dpm_step_px', torch.cuda.current_stream().cuda_stream, x=x.data_ptr(), out=out.data_ptr(),
              m0=gm.data_ptr(), base=base.data_ptr(), h1=h1.data_ptr(), h2=h2.data_ptr(), y=gy.data_ptr(), R=R,
              rows_per_sample=R // 2, target=0, correct=2, q_k=k, q_w=wq, max_val=MAX_VAL, sigma=float(e['sigma']),
              alpha=float(e['alpha']), mode=upd['mode'],
              **{c: float(upd[c]) for c in ('c0', 'c1', 'c2', 'c3', 'k0', 'k1', 'g', 'k2')})
    torch.cuda.synchronize()
    assert _same(gm[:R].view_as(m0_c), m0_c) and _same(gy[:R].view_as(y_c), y_c)
    assert (gm[R] == 7.0).all() and (gy[R] == 7.0).all()
    rec = _record(3, 3)                                  # the same size through the other entry point
    h3, ub = _rows(x.shape, g), _rows(x.shape, g, 1.0)
    ukw = dict(target='eps', correct='dynamic', ratio=RATIO, max_val=MAX_VAL, base=ub, h1=h1, h2=h2, h3=h3)
    want = ops.unipc_step_px(x, out, rec, fused=False, **ukw)
    got = ops.unipc_step_px(x, _nanpad(out), rec, **ukw)
    assert all(_same(p, q) and (p[..., 3] == 0).all() for p, q in zip(got, want))

    xb, ob = _batch(129, 128, 'v', e, g, B=2)            # just past the limit
    Rb = xb.numel() // 4
    before = torch.full_like(xb, 3.0)
    with pytest.raises(_lib.SdmiError, match=r'sdmi_dpm_step_px failed \(-3\)'):
        _lib.call('sdmi_dpm_step_px', torch.cuda.current_stream().cuda_stream, x=xb.data_ptr(), out=ob.data_ptr(),
                  m0=before.data_ptr(), R=Rb, rows_per_sample=Rb // 2, target=2, correct=2, q_k=5, q_w=0.5, max_val=1.0,
                  sigma=float(e['sigma']), alpha=float(e['alpha']))
    torch.cuda.synchronize()
    assert (before == 3.0).all()                         # nothing was launched
    m0_c, y_c = ops.dpm_step_px(xb, ob, e, fused=False, target='v', correct='dynamic')
    m0, y = ops.dpm_step_px(xb, ob, e, target='v', correct='dynamic')
    assert _same(m0, m0_c) and y is None
    rec = _record(3, 3)
    hs = [_rows(xb.shape, g) for _ in range(4)]
    a = ops.unipc_step_px(xb, ob, rec, correct='dynamic', base=hs[0], h1=hs[1], h2=hs[2], h3=hs[3])
    b = ops.unipc_step_px(xb, ob, rec, correct='dynamic', base=hs[0], h1=hs[1], h2=hs[2], h3=hs[3], fused=False)
    assert all(_same(p, q) for p, q in zip(a, b))
    # without a quantile there is no limit: one row per thread
    a = ops.dpm_step_px(xb, ob, e, correct='clamp', upd=upd, base=hs[0], h1=hs[1], h2=hs[2])
    b = ops.dpm_step_px(xb, ob, e, correct='clamp', upd=upd, base=hs[0], h1=hs[1], h2=hs[2], fused=False)
    assert all(_same(p, q) for p, q in zip(a, b))


def test_refusals():
    """Before any launch: null pointers, orders / modes outside range, rows_per_sample that is not positive or does not
    divide R, a quantile position outside the sample, overlapping outputs."""
    from slotdiffusion_amd import _lib
    t = [torch.zeros(8, 4).cuda() for _ in range(8)]
    p = [v.data_ptr() for v in t]
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(x=p[0], out=p[1], m0=p[2], R=8, rows_per_sample=4, target=0, correct=2, q_k=3, q_w=0.5, max_val=1.0,
              sigma=0.5, alpha=0.5)
    _lib.call('sdmi_dpm_step_px', st, **ok)
    _lib.call('sdmi_unipc_step_px', st, **ok)
    bad = [dict(x=0), dict(m0=0), dict(rows_per_sample=0), dict(rows_per_sample=-4), dict(rows_per_sample=3),
           dict(correct=3), dict(target=3), dict(q_k=12), dict(q_k=-1), dict(q_k=11), dict(q_w=1.0), dict(max_val=0.0),
           dict(alpha=0.0), dict(m0=p[0])]
    dpm_bad = bad + [dict(mode=5), dict(mode=1), dict(mode=1, base=p[3], y=p[2]), dict(mode=4, base=p[3], y=p[4], h1=p[5]),
                     dict(mode=1, base=p[3], y=p[3])]
    uni_bad = bad + [dict(corr_order=4), dict(pred_order=-1), dict(pred_order=1, y=p[4]), dict(pred_order=1, base=p[3]),
                     dict(corr_order=3, base=p[3], xc=p[4], h1=p[5], h2=p[6]),
                     dict(corr_order=1, pred_order=1, base=p[3], h1=p[5], xc=p[4], y=p[4])]
    for name, cases in (('sdmi_dpm_step_px', dpm_bad), ('sdmi_unipc_step_px', uni_bad)):
        for over in cases:
            with pytest.raises(_lib.SdmiError, match=name + r' failed \(-1\)'):
                _lib.call(name, st, **dict(ok, **over))
    torch.cuda.synchronize()


# ---- the model surface: SADiffusion / SAViDiffusion with the image-space decoder (CondDDPM) at 32 x 32 --------------------
_cache = {}


def px_ctx(dtype=torch.float32):
    from slotdiffusion_amd.models import SADiffusion
    from tests import common as C
    from tests.detfill import det_fill_, is_buffer_name
    from tests.test_pixel_cpu import px_cfg
    if 'G' not in _cache:
        _cache['G'] = C.load_golden('sadiff_px_b2.npz')
    if dtype not in _cache:
        cfg = px_cfg()
        m = SADiffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['loss_dict'],
                        compute_dtype=dtype)
        det_fill_(m.state_dict().items(), skip=is_buffer_name)
        m.train_dropout = 0.0
        m = m.cuda().eval()
        m.use_graph = False
        _cache[dtype] = m
    return _cache[dtype], _cache['G']


def _maxerr(a, b):
    return float((a.float().cpu() - b.float()).abs().max())


SURFACE = {'default': {}, 'multistep': dict(dpm_method='multistep', dpm_order=3, dpm_steps=8),
           'unipc3': dict(use_unipc=True, unipc_steps=6, unipc_order=3)}


@pytest.mark.parametrize('name', list(SURFACE))
def test_model_surface_fused_chain_eager_graph_replay(name):
    """fp32, B = 2: the fused loop (one *_px launch per evaluation) equals the same loop driven through the composed
    chain, intermediates included; eager = HIP graph = replay, also when replays alternate with an unthresholded call
    (clip_denoised = False) and with a latent model's call in the same process."""
    from tests.test_gpu_model import ctx
    m, G = px_ctx()
    dm = m.dm_decoder
    kw = SURFACE[name]
    cond, x_T = G['slots'].cuda(), G['x_T'].cuda()
    run = lambda **o: dm.generate_imgs(cond=cond, batch_size=2, x_T=x_T, **kw, **o)
    fused = run(ret_intermed=True)
    assert torch.isfinite(fused[1]).all() and fused[0].shape == (2, 3, 32, 32)
    m.fused_px = False
    try:
        chain = run(ret_intermed=True)
    finally:
        m.fused_px = True
    assert torch.equal(fused[0], chain[0]) and torch.equal(fused[1], chain[1])
    eager = run().clone()
    assert torch.equal(eager, fused[0])
    dm.clip_denoised = False
    try:
        eager_off = run().clone()
    finally:
        dm.clip_denoised = True
    assert not torch.equal(eager_off, eager)                       # thresholding acts on this model
    assert torch.equal(run(**{('unipc_' if 'use_unipc' in kw else 'dpm_') + 'correcting_x0_fn': True}), eager)
    lat, GL, _ = ctx()
    lrun = lambda: lat.dm_decoder.generate_imgs(cond=GL['slots'].cuda(), batch_size=2, x_T=GL['x_T'].cuda(), **kw).clone()
    lat_eager = lrun()
    m.use_graph = lat.use_graph = True
    try:
        n0 = len(m._graph_cache)
        for i in range(2):
            assert torch.equal(run(), eager), i
            dm.clip_denoised = False
            try:
                assert torch.equal(run(), eager_off), i
            finally:
                dm.clip_denoised = True
            assert torch.equal(lrun(), lat_eager), i
        assert len(m._graph_cache) == n0 + 2                       # thresholded and unthresholded: two entries
        assert torch.equal(run(), eager)
    finally:
        m.use_graph = lat.use_graph = False
        m._graph_cache.clear()
        lat._graph_cache.clear()


def test_samplers_against_the_reference():
    """tests/golden/sadiff_px_b2.npz: every solver state of the default 20-evaluation run (thresholding on) within 1e-4,
    the bound the project asserts for fp32 solver states; ancestral and DDIM single steps restarted from the reference's
    states within the latent tests' bounds (>= 99.5 % of the elements within 1e-4, first logged DDIM state 1e-4)."""
    from slotdiffusion_amd import dpm, ops
    m, G = px_ctx()
    dm = m.dm_decoder
    slots = G['slots'].cuda()
    x, inter = dm.generate_imgs(cond=slots, batch_size=2, x_T=G['x_T'].cuda(), ret_intermed=True)
    errs = [_maxerr(inter[i], G['dpm_trace'][i]) for i in range(G['dpm_trace'].shape[0])]
    print('dpm trace max errors', errs, 'final', _maxerr(x, G['dpm_final']))
    assert inter.shape == G['dpm_trace'].shape
    assert max(errs) <= 1e-4 and _maxerr(x, G['dpm_final']) <= 1e-4
    # ancestral: clip_denoised clamps the predicted x0
    nz = G['anc_noise'].cuda()
    x_in, agree = G['x_T'], 1.0
    for j, tv in enumerate(int(v) for v in G['anc_t'].tolist()):
        xd = next(m._ancestral_steps(ops.nchw_to_nhwc(x_in.cuda(), torch.float32, 4), slots, [tv], noises=[nz]))[0]
        d = (ops.nhwc_to_nchw(xd, 3).cpu() - G['anc_x'][j]).abs()
        print('ancestral step', tv, 'max error', float(d.max()))
        agree = min(agree, float((d <= 1e-4).float().mean()))
        x_in = G['anc_x'][j]
    assert agree >= 0.995
    # DDIM, 10 steps: the first logged state, then single steps from the reference's states
    steps = G['ddim_inter'].shape[0] - 1
    plan = dpm.ddim_plan(dm.alphas_bar.detach().float().cpu(), steps)
    out, di = dm.generate_imgs(slots, batch_size=2, ret_intermed=True, use_dpm=False, use_ddim=True, x_T=G['x_T'].cuda(),
                               ddim_steps=steps, log_every_t=1)
    assert di.shape == G['ddim_inter'].shape
    assert _maxerr(di[0], G['ddim_inter'][0]) == 0.0 and _maxerr(di[1], G['ddim_inter'][1]) <= 1e-4
    worst = 1.0
    for k in range(1, steps):
        st = [s for s in plan if s['index'] == steps - 1 - k]
        xd = next(m._ddim_steps(ops.nchw_to_nhwc(G['ddim_inter'][k].cuda(), torch.float32, 4), slots, st))[0]
        d = (ops.nhwc_to_nchw(xd, 3).cpu() - G['ddim_inter'][k + 1]).abs()
        print('ddim step', k, 'max error', float(d.max()))
        worst = min(worst, float((d <= 1e-4).float().mean()))
    assert worst >= 0.995


def test_loss_and_gradients_against_the_reference():
    """x0 is the image itself (no encode, no z_scale_factor): loss within 1e-4 and per-parameter gradient norms within
    1e-2 of the reference's fp32 ones, global norm within 1e-3 -- test_gpu_train.py's bounds for sadiff_b2.npz."""
    import math
    m, G = px_ctx()
    m.train()
    try:
        m.grad_arena().zero_()
        img = G['img'].cuda()
        out = m(dict(img=img))
        loss = m.calc_train_loss(dict(img=img, t=G['t'].cuda(), noise=G['noise'].cuda()), out)['denoise_loss']
        loss.backward()
        named = dict(m.named_parameters())
        names = [str(n) for n in G['grad_norms_names']]
        mine = torch.tensor([float(named[n].grad.norm()) for n in names])
        gn = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in named.values() if p.requires_grad))
    finally:
        m.eval()
    big = G['grad_norms'] > 1e-6
    rel = ((mine - G['grad_norms']).abs() / (G['grad_norms'].abs() + 1e-12))[big]
    print('loss', float(loss), 'ref', float(G['denoise_loss']), 'grad norm max rel', float(rel.max()), 'global', gn,
          float(G['grad_global_norm']))
    assert abs(float(loss) - float(G['denoise_loss'])) <= 1e-4
    assert float(rel.max()) <= 1e-2
    from slotdiffusion_amd import ops
    with torch.no_grad():                                # q-sample of the image itself and the UNet on it, 1e-4 as for latents
        xt = ops.nchw_to_nhwc(G['x_t'].cuda(), torch.float32, 4)
        x0 = m.dm_decoder.encode_x0(img)
        nz = ops.nchw_to_nhwc(G['noise'].cuda(), torch.float32, 4)
        dmd = m.dm_decoder
        mine_xt = ops.row_lincomb(x0, nz, dmd.sqrt_alphas_bar[G['t'].cuda()].contiguous(),
                                  dmd.sqrt_one_minus_alphas_bar[G['t'].cuda()].contiguous())
        assert _maxerr(ops.nhwc_to_nchw(mine_xt, 3), G['x_t']) <= 1e-4
        pred = ops.nhwc_to_nchw(m._unet_eps(xt, G['t'].float().cuda(), G['slots'].cuda()), 3)
        print('eps max error', _maxerr(pred, G['pred']))
        assert _maxerr(pred, G['pred']) <= 1e-4
    # the x0 target (the same weights: the loss target is the image), test_gpu_model.py's bounds for anc_x0_b2.npz
    m.dm_decoder.pred_target = 'x0'
    m.train()
    try:
        m.grad_arena().zero_()
        out = m(dict(img=img))
        l0 = m.calc_train_loss(dict(img=img, t=G['t'].cuda(), noise=G['noise'].cuda()), out)['denoise_loss']
        l0.backward()
        named = dict(m.named_parameters())
        mine0 = torch.tensor([float(named[str(n)].grad.norm()) for n in G['x0_grad_norms_names']])
        gn0 = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in named.values() if p.requires_grad))
    finally:
        m.dm_decoder.pred_target = 'eps'
        m.eval()
    rel0 = (mine0 - G['x0_grad_norms']).abs() / (G['x0_grad_norms'].abs() + 1e-12)
    print('x0 loss', float(l0), float(G['x0_denoise_loss']), 'grad norm max rel', float(rel0.max()))
    assert abs(float(l0) - float(G['x0_denoise_loss'])) <= 1e-5 * max(1.0, float(G['x0_denoise_loss']))
    assert float(rel0.max()) <= 2e-3
    assert abs(gn0 - float(G['x0_grad_global_norm'])) <= 1e-3 * float(G['x0_grad_global_norm'])
    assert abs(gn - float(G['grad_global_norm'])) <= 1e-3 * float(G['grad_global_norm'])
    with torch.no_grad():
        ev = m.calc_eval_loss(dict(img=img, t=G['t'].cuda(), noise=G['noise'].cuda()), dict(slots=G['slots'].cuda()))
    assert abs(float(ev['denoise_loss']) - float(G['denoise_loss'])) <= 1e-4


def test_video_twin_against_the_reference():
    """SAViDiffusion with the image-space decoder, B = 1, T = 2 (tests/golden/savidiff_px_b1t2.npz): loss (eps and v
    targets) within 1e-4, the final sample of the default run within 1e-4; log_images returns NCHW frames."""
    from slotdiffusion_amd.models import CondDDPM, SAViDiffusion
    from tests import common as C
    from tests.detfill import det_fill_, is_buffer_name
    from tests.test_pixel_cpu import px_cfg
    V = C.load_golden('savidiff_px_b1t2.npz')
    cfg = px_cfg(video=True)
    m = SAViDiffusion(cfg['resolution'], 2, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'],
                      cfg['loss_dict'], compute_dtype=torch.float32)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    m.train_dropout = m.pred_dropout = 0.0
    m = m.cuda().eval()
    m.use_graph = False
    assert type(m.dm_decoder) is CondDDPM
    img = V['img'].cuda()
    out = m(dict(img=img))
    assert _maxerr(out['slots'], V['slots']) <= 1e-4
    batch = dict(img=img, t=V['t'].cuda(), noise=V['noise'].cuda())
    loss = m.calc_eval_loss(batch, dict(slots=V['slots'].cuda()))['denoise_loss']
    m.dm_decoder.pred_target = 'v'
    try:
        vloss = m.calc_eval_loss(batch, dict(slots=V['slots'].cuda()))['denoise_loss']
    finally:
        m.dm_decoder.pred_target = 'eps'
    print('video loss', float(loss), float(V['denoise_loss']), 'v', float(vloss), float(V['v_denoise_loss']))
    assert abs(float(loss) - float(V['denoise_loss'])) <= 1e-4
    assert abs(float(vloss) - float(V['v_denoise_loss'])) <= 1e-4
    x = m.dm_decoder.generate_imgs(cond=V['slots'].flatten(0, 1).cuda(), batch_size=2, x_T=V['x_T'].cuda())
    print('video final max error', _maxerr(x, V['dpm_final']))
    assert _maxerr(x, V['dpm_final']) <= 1e-4
    log = m.log_images(dict(img=img), x_T=V['x_T'].cuda())
    assert log['samples'].shape == (1, 2, 3, 32, 32) and torch.isfinite(log['samples']).all()


def test_unet_forward_at_a_pixel_shape():
    """One UNet forward at 64 x 64, B = 1, fp32, against oracle.unet_forward within 1e-4 (the latent-shape bound): the one
    place where the UNet kernels meet new shapes (attention over 32 * 32 and 16 * 16 tokens, GroupNorm over 4096
    positions)."""
    from oracle import slotdiff_oracle as O
    from slotdiffusion_amd import ops, spec
    from tests import common as C
    from tests.test_pixel_cpu import px_cfg
    m, G = px_ctx()
    cfg = px_cfg()
    W = C.oracle_weights(cfg)
    uplan = spec.unet_plan(cfg['dec_dict']['unet_dict'])
    g = torch.Generator().manual_seed(64)
    x = torch.randn(1, 3, 64, 64, generator=g)
    t = torch.tensor([417])
    slots = G['slots'][:1]
    with torch.no_grad():
        want = O.unet_forward(W, uplan, x, t, slots)
    got = ops.nhwc_to_nchw(m._unet_eps(ops.nchw_to_nhwc(x.cuda(), torch.float32, 4), t.float().cuda(), slots.cuda()), 3)
    print('unet 64x64 max error', _maxerr(got, want), 'scale', float(want.abs().max()))
    assert got.shape == (1, 3, 64, 64) and _maxerr(got, want) <= 1e-4


def test_graphed_train_step_changes_the_weights():
    """B = 2 at 32 x 32 through the HIP-graph train step: the weights change, and its loss equals the eager path's bit for
    bit."""
    from slotdiffusion_amd.models import SADiffusion
    from slotdiffusion_amd.optim import FusedAdam, GraphedTrainStep
    from tests.detfill import det_fill_, is_buffer_name
    from tests.test_pixel_cpu import px_cfg
    _, G = px_ctx()
    batch = dict(img=G['img'].cuda(), t=G['t'].cuda(), noise=G['noise'].cuda())
    losses, finals = [], []
    for graphed in (False, True):
        cfg = px_cfg()
        m = SADiffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['loss_dict'],
                        compute_dtype=torch.float32)
        det_fill_(m.state_dict().items(), skip=is_buffer_name)
        m.train_dropout = 0.0
        m = m.cuda().train()
        before = m.arena().detach().clone()
        opt = FusedAdam(m, lr=1e-4, dec_lr=2e-4, clip_grad=1.0, total_steps=50, warmup_pct=0.2)
        if graphed:
            gs = GraphedTrainStep(m, opt, batch)
            ls = [float(gs(batch)) for _ in range(2)]
        else:
            ls = []
            for _ in range(2):
                opt.zero_grad()
                loss = m.calc_train_loss(batch, m(batch))['denoise_loss']
                loss.backward()
                opt.step()
                ls.append(float(loss))
        assert not torch.equal(m.arena().detach(), before)
        losses.append(ls)
        finals.append(m.arena().detach().clone())
    assert losses[0] == losses[1] and torch.equal(finals[0], finals[1])
    assert abs(losses[0][0] - float(G['denoise_loss'])) <= 1e-4


def test_bf16_final_sample_deviation():
    """bf16 compute path (the tail itself is fp32 either way): the final sample of the default 20-evaluation run within
    2 % rel-L2 of the fp32 path's, the bound tests/test_gpu_model.py::test_bf16_path_deviation sets for the image
    model's bf16 tensors."""
    m32, G = px_ctx()
    m16, _ = px_ctx(torch.bfloat16)
    cond, x_T = G['slots'].cuda(), G['x_T'].cuda()
    a = m32.dm_decoder.generate_imgs(cond=cond, batch_size=2, x_T=x_T)
    b = m16.dm_decoder.generate_imgs(cond=cond, batch_size=2, x_T=x_T)
    rel = float((b - a).norm() / a.norm())
    print('bf16 vs fp32 rel-L2 of the final sample, 20 evaluations', rel)
    assert torch.isfinite(b).all() and rel < 0.02
