"""UniPC on the GPU: the fused tail kernel (sdmi_unipc_step) against the chain of sdmi_lincomb / sdmi_vq_nearest launches
that include/sdmi.h spells, the model surface (fused loop = chain-driven loop, eager = HIP graph = replay, alternating
with a DPM configuration), the bf16 deviation next to the multistep solver's, and the video model."""
import pytest
import torch

from slotdiffusion_amd import unipc
from tests import common as C
from tests.test_dpm_family_cpu import betas
from tests.test_gpu_model import ctx

pytestmark = pytest.mark.gpu

TARGETS = ('eps', 'x0', 'v')
ORDERS = [(0, 1), (1, 2), (2, 3), (3, 3), (3, 2), (2, 1), (3, 0), (0, 0)]       # (corrector, predictor)
NAN_ROW, TIE_ROW, TIE_LO, TIE_HI = 777, 1500, 17, 3000


def _record(corr_order, pred_order):
    """A realistic record with the two orders, pieced from the steps of a 10-evaluation third-order plan."""
    prog = unipc.program(unipc.build_plan(betas().double(), steps=10, order=3))
    corr = next(r['corr'] for r in prog[1:] if r['corr']['order'] == corr_order) if corr_order else None
    pred = next(r['pred'] for r in prog if r['pred']['order'] == pred_order) if pred_order else None
    return dict(e=prog[5]['e'], corr=corr, pred=pred)


def _chain(ops, x, out, code, rec, *, scale=1.0, target='eps', base=None, h1=None, h2=None, h3=None, m0=None, xc=None,
           y=None, want_idx=False):
    """ops.unipc_step's signature and results, made of the launches the fused kernel replaces (sdmi.h lists them)."""
    e, c, p = rec['e'], rec['corr'], rec['pred']
    if target == 'x0':
        eps = ops.lincomb(1.0, x, -e['alpha'], out, div=e['sigma'])
    elif target == 'v':
        eps = ops.lincomb(e['alpha'], out, e['sigma'], x)
    else:
        eps = out
    x0 = ops.lincomb(1.0, x, -e['sigma'], eps, div=e['alpha'])
    idx, m0 = ops.vq_nearest(x0, code, scale=scale)
    xc = y = None
    if c is not None:
        v = ops.lincomb(c['c0'], base, c['c1'], h1, c['w1'], h2, h1) if c['order'] >= 2 else \
            ops.lincomb(c['c0'], base, c['c1'], h1)
        if c['order'] == 3:
            v = ops.lincomb(1.0, v, c2=c['w2'], x2=h3, x3=h1)
        xc = ops.lincomb(1.0, v, c2=c['wn'], x2=m0, x3=h1)
    if p is not None:
        s = base if xc is None else xc
        y = ops.lincomb(p['c0'], s, p['c1'], m0, p['q1'], h1, m0) if p['order'] >= 2 else \
            ops.lincomb(p['c0'], s, p['c1'], m0)
        if p['order'] == 3:
            y = ops.lincomb(1.0, y, c2=p['q2'], x2=h2, x3=m0)
    return m0, xc, y, idx


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.), b.nan_to_num(nan=0.))


@pytest.mark.parametrize('orders', ORDERS, ids=[f'c{c}p{p}' for c, p in ORDERS])
@pytest.mark.parametrize('target', TARGETS)
def test_unipc_step_equals_the_launch_chain(target, orders):
    """Indices = sdmi_vq_nearest's on the same prediction; m0, the corrected and the predicted state bit-identical to the
    chain; one row holds a NaN, one lands on a duplicated code (an exact distance tie: the lower index wins)."""
    from slotdiffusion_amd import ops
    m, _, _ = ctx()
    scale = m.z_scale
    code = m.bank().f(m.vq_key).clone()
    code[TIE_HI] = code[TIE_LO]
    rec = _record(*orders)
    e = rec['e']
    g = torch.Generator().manual_seed(11 + 7 * TARGETS.index(target) + ORDERS.index(orders))

    def rows(std=1.0):
        t = torch.randn(2, 32, 32, 4, generator=g) * std
        t[..., 3] = 0.
        return t.cuda()
    x, out, h1, h2, h3 = rows(), rows(), rows(0.5), rows(0.5), rows(0.5)
    base = rows() if rec['corr'] else x                  # without corrector the carried state IS the evaluated state
    c = code[TIE_LO].cpu() / scale                       # the data prediction that lands on the duplicated code
    xf, of = x.view(-1, 4), out.view(-1, 4)
    if target == 'eps':                                  # x0 = (x - sigma * out) / alpha
        xf[TIE_ROW, :3], of[TIE_ROW, :3] = (c * e['alpha']).cuda(), 0.
    elif target == 'x0':                                 # x0 = out up to rounding
        of[TIE_ROW, :3] = c.cuda()
    else:                                                # x0 = alpha * x - sigma * out up to rounding
        xf[TIE_ROW, :3], of[TIE_ROW, :3] = (c / e['alpha']).cuda(), 0.
    xf[NAN_ROW, 1] = float('nan')
    kw = dict(scale=scale, target=target, base=base, h1=h1, h2=h2, h3=h3, want_idx=True)
    m0_c, xc_c, y_c, idx_c = _chain(ops, x, out, code, rec, **kw)
    out_nanpad = out.clone()
    out_nanpad[..., 3] = float('nan')                    # the pad channel of the network output is never read
    m0, xc, y, idx = ops.unipc_step(x, out_nanpad, code, rec, **kw)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx_c)
    assert int(idx.view(-1)[TIE_ROW]) == TIE_LO
    assert torch.isnan(m0.view(-1, 4)[NAN_ROW, :3]).any() and not torch.isnan(m0.view(-1, 4)[NAN_ROW + 1]).any()
    assert _same(m0, m0_c) and (m0[..., 3] == 0).all()
    ref_c, ref_y = unipc.update_expr(rec, base, m0_c, h1, h2, h3)       # and the chain is the documented expression
    for got, want, ref, on in ((xc, xc_c, ref_c, orders[0]), (y, y_c, ref_y, orders[1])):
        if not on:
            assert got is None and want is None
            continue
        assert _same(got, want) and (got[..., 3] == 0).all()
        assert _same(got[..., :3], ref[..., :3])
        assert torch.isnan(got.view(-1, 4)[NAN_ROW, :3]).any()


def test_unipc_step_partial_block():
    from slotdiffusion_amd import ops
    m, _, _ = ctx()
    code = m.bank().f(m.vq_key)
    rec = _record(3, 3)
    g = torch.Generator().manual_seed(3)
    x, out, base, h1, h2, h3 = (torch.randn(7, 11, 4, generator=g).cuda() for _ in range(6))   # 77 rows: 1 1/4 blocks
    kw = dict(scale=m.z_scale, base=base, h1=h1, h2=h2, h3=h3, want_idx=True)
    m0_c, xc_c, y_c, idx_c = _chain(ops, x, out, code, rec, **kw)
    guard = torch.full((78, 4), 7.0).cuda()              # the row past the end keeps its contents
    m0, xc, y, idx = ops.unipc_step(x, out, code, rec, y=guard[:77].view(7, 11, 4), **kw)
    assert torch.equal(idx, idx_c)
    for got, want in ((m0, m0_c), (xc, xc_c), (y, y_c)):
        assert torch.equal(got[..., :3], want[..., :3]) and (got[..., 3] == 0).all()
    assert (guard[77] == 7.0).all()


def _kw(**kw):
    return dict({'unipc_' + k: v for k, v in kw.items()}, use_unipc=True)


def test_model_surface_fused_chain_eager_graph_replay(monkeypatch):
    """fp32, B = 2, 5 evaluations at order 3, from x_T and from noise_latent at t_start = 0.6: the fused loop equals the
    same loop driven through the launch chain (same UNet calls), intermediates included; eager = HIP graph = replay =
    replay alternated with a DPM multistep configuration, bit for bit."""
    from slotdiffusion_amd import ops
    m, G, _ = ctx()
    dm = m.dm_decoder
    cond = G['slots'].cuda()
    x_T = G['x_T'].cuda()
    x_06 = dm.noise_latent(G['x0'].cuda(), 0.6, G['noise'].cuda())
    A = _kw(steps=5, order=3)
    Bc = _kw(steps=5, order=3, t_start=0.6)
    D = dict(dpm_method='multistep', dpm_order=3, dpm_steps=5)
    run = lambda kw, x, **o: dm.generate_imgs(cond=cond, batch_size=2, x_T=x, **kw, **o)
    assert not m.use_graph
    fused = {k: run(kw, x, ret_intermed=True) for k, kw, x in (('a', A, x_T), ('b', Bc, x_06))}
    for k in fused:
        assert fused[k][1].shape[0] == 6 and torch.isfinite(fused[k][1]).all()
    calls = []
    real = ops.unipc_step
    with monkeypatch.context() as mp:
        mp.setattr(ops, 'unipc_step', lambda *a, **kw: (calls.append(1), _chain(ops, *a, **kw))[1])
        chain = {k: run(kw, x, ret_intermed=True) for k, kw, x in (('a', A, x_T), ('b', Bc, x_06))}
    assert ops.unipc_step is real and len(calls) == 10
    for k in fused:
        assert torch.equal(fused[k][0], chain[k][0]) and torch.equal(fused[k][1], chain[k][1]), k
    assert not torch.equal(fused['a'][0], fused['b'][0])
    eager = {'a': run(A, x_T).clone(), 'b': run(Bc, x_06).clone(), 'd': run(D, x_T).clone()}
    assert torch.equal(eager['a'], fused['a'][0]) and torch.equal(eager['b'], fused['b'][0])   # ring buffers = fresh ones
    assert not torch.equal(eager['a'], eager['d'])
    m.use_graph = True
    try:
        n0 = len(m._graph_cache)
        seq = [('a', A, x_T), ('a', A, x_T), ('d', D, x_T), ('b', Bc, x_06), ('a', A, x_T), ('d', D, x_T), ('b', Bc, x_06)]
        got = [(k, run(kw, x).clone()) for k, kw, x in seq]
        assert len(m._graph_cache) == n0 + 3
        for k, v in got:
            assert torch.equal(v, eager[k]), k
    finally:
        m.use_graph = False
        m._graph_cache.clear()


def test_bf16_deviation_next_to_the_multistep_solver():
    """bf16 compute path against the fp32 one, 10 evaluations at order 3: finite, and the rel-L2 of the final latent at
    most twice what dpm_method='multistep' shows between the same two models (the margin covers a VQ snap that flips
    between dtypes on one path and not on the other)."""
    m32, G, _ = ctx()
    m16, _, _ = ctx(torch.bfloat16)
    cond, x_T = G['slots'].cuda(), G['x_T'].cuda()
    U = _kw(steps=10, order=3)
    D = dict(dpm_method='multistep', dpm_order=3, dpm_steps=10)
    rel = {}
    for k, kw in (('unipc', U), ('multistep', D)):
        a = m32.dm_decoder.generate_imgs(cond=cond, batch_size=2, x_T=x_T, **kw)
        b = m16.dm_decoder.generate_imgs(cond=cond, batch_size=2, x_T=x_T, **kw)
        assert torch.isfinite(b).all()
        rel[k] = float((b - a).norm() / a.norm())
    print('bf16 vs fp32 rel-L2 of the final latent at 10 evaluations: UniPC-3 bh2', rel['unipc'], 'multistep-3',
          rel['multistep'])
    assert rel['unipc'] <= 2. * rel['multistep']


def test_video_log_images_graph_equals_eager():
    """SAViDiffusion.log_images forwards the UniPC keywords through the flattened B*T frames; the HIP graph gives the
    eager samples bit for bit (the model of tests/golden/savidiff_b1t3.npz: MOVi-E config, T = 3)."""
    from slotdiffusion_amd.models import SAViDiffusion
    from tests.detfill import det_fill_, is_buffer_name
    cfg = C.movie_cfg()
    T = 3
    m = SAViDiffusion(cfg['resolution'], T, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'],
                      cfg['loss_dict'], compute_dtype=torch.float32)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    m = m.cuda().eval()
    img = C.make_inputs(T, seed=11)[0].view(1, T, 3, 128, 128).cuda()
    x_T = torch.randn(T, 3, 32, 32, generator=torch.Generator().manual_seed(23)).cuda()
    kw = _kw(steps=4, order=3, denoise_to_zero=True)
    m.use_graph = False
    eager = m.log_images(dict(img=img), x_T=x_T, **kw)['samples'].clone()
    assert eager.shape == (1, T, 3, 128, 128) and torch.isfinite(eager).all()
    m.use_graph = True
    first = m.log_images(dict(img=img), x_T=x_T, **kw)['samples'].clone()
    replay = m.log_images(dict(img=img), x_T=x_T, **kw)['samples'].clone()
    assert torch.equal(first, eager) and torch.equal(replay, eager)
