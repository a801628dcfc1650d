"""DPM-Solver++ family on the GPU: the fused tail kernel (sdmi_dpm_step) against the chain of launches it replaces,
the five reference configurations of tests/golden/dpm_family_b2.npz through the model surface, HIP-graph replay with
alternating configurations, and the video model."""
import pytest
import torch

from slotdiffusion_amd import dpm
from tests import common as C
from tests.test_dpm_family_cpu import BAR, CONFIGS, betas, family
from tests.test_gpu_model import ctx

pytestmark = pytest.mark.gpu

TARGETS = ('eps', 'x0', 'v')
MODES = {'none': dpm.UPD_NONE, 'first': dpm.UPD_FIRST, 'single': dpm.UPD_SINGLE, 'multi2': dpm.UPD_MULTI2,
         'multi3': dpm.UPD_MULTI3}
NAN_ROW, TIE_ROW, TIE_LO, TIE_HI = 777, 1500, 17, 3000


def _kw(kw):
    return {'dpm_' + k: v for k, v in kw.items()}


def _update_of(mode):
    """A realistic update record of each form, from the plans that use it."""
    b = betas()
    prog = dpm.program(dpm.build_plan(b, steps=15, order=3, method='multistep')) + \
        dpm.program(dpm.build_plan(b, steps=12, order=3))
    return next(op['upd'] for op in prog if op['upd']['mode'] == mode), prog[5]['e']


def _chain(ops, x, out, code, e, scale, target, upd, base, h1, h2):
    """The launches the fused kernel replaces, spelling the reference's expressions with sdmi_lincomb / sdmi_vq_nearest
    (model_wrapper 358-365, data_prediction_fn 529, the updates of dpm.update_expr)."""
    if target == 'x0':
        eps = ops.lincomb(1.0, x, -e['alpha'], out, div=e['sigma'])
    elif target == 'v':
        eps = ops.lincomb(e['alpha'], out, e['sigma'], x)
    else:
        eps = out
    x0 = ops.lincomb(1.0, x, -e['sigma'], eps, div=e['alpha'])
    idx, m0 = ops.vq_nearest(x0, code, scale=scale)
    if upd is None:
        return idx, m0, None
    u = upd
    if u['mode'] == dpm.UPD_FIRST:
        return idx, m0, ops.lincomb(u['c0'], base, u['c1'], m0)
    if u['mode'] == dpm.UPD_SINGLE:
        return idx, m0, ops.lincomb(u['c0'], base, u['c1'], h1, u['c2'], m0, h1)
    D1_0 = ops.lincomb(c2=u['k0'], x2=m0, x3=h1)
    if u['mode'] == dpm.UPD_MULTI2:
        return idx, m0, ops.lincomb(u['c0'], base, u['c1'], m0, u['c2'], D1_0)
    D1_1 = ops.lincomb(c2=u['k1'], x2=h1, x3=h2)
    D1 = ops.lincomb(1.0, D1_0, c2=u['g'], x2=D1_0, x3=D1_1)
    D2 = ops.lincomb(c2=u['k2'], x2=D1_0, x3=D1_1)
    y1 = ops.lincomb(u['c0'], base, u['c1'], m0, u['c2'], D1)
    return idx, m0, ops.lincomb(1.0, y1, u['c3'], D2)


def _same(a, b):
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.), b.nan_to_num(nan=0.))


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('target', TARGETS)
def test_dpm_step_equals_the_launch_chain(target, mode):
    """Indices = sdmi_vq_nearest's on the same prediction; m0 and the updated state bit-identical to the chain; one row
    holds a NaN, one lands on a duplicated code (an exact distance tie: the lower index wins)."""
    from slotdiffusion_amd import ops
    m, _, _ = ctx()
    scale = m.z_scale
    code = m.bank().f(m.vq_key).clone()
    code[TIE_HI] = code[TIE_LO]
    upd, e = (None, _update_of(dpm.UPD_FIRST)[1]) if mode == 'none' else _update_of(MODES[mode])
    g = torch.Generator().manual_seed(5 + 7 * TARGETS.index(target) + list(MODES).index(mode))

    def rows(std=1.0):
        t = torch.randn(2, 32, 32, 4, generator=g) * std
        t[..., 3] = 0.
        return t.cuda()
    x, base, h1, h2 = rows(), rows(), rows(0.5), rows(0.5)
    out = rows()
    c = code[TIE_LO].cpu() / scale                       # the data prediction that lands on the duplicated code
    xf, of = x.view(-1, 4), out.view(-1, 4)
    if target == 'eps':                                  # x0 = (x - sigma * out) / alpha
        xf[TIE_ROW, :3], of[TIE_ROW, :3] = (c * e['alpha']).cuda(), 0.
    elif target == 'x0':                                 # x0 = out up to rounding
        of[TIE_ROW, :3] = c.cuda()
    else:                                                # x0 = alpha * x - sigma * out up to rounding
        xf[TIE_ROW, :3], of[TIE_ROW, :3] = (c / e['alpha']).cuda(), 0.
    xf[NAN_ROW, 1] = float('nan')
    idx_c, m0_c, y_c = _chain(ops, x, out, code, e, scale, target, upd, base, h1, h2)
    out_nanpad = out.clone()
    out_nanpad[..., 3] = float('nan')                    # the pad channel of the network output is never read
    m0, y, idx = ops.dpm_step(x, out_nanpad, code, e, scale=scale, target=target, upd=upd, base=base, h1=h1, h2=h2,
                              want_idx=True)
    torch.cuda.synchronize()
    assert torch.equal(idx, idx_c)
    assert int(idx.view(-1)[TIE_ROW]) == TIE_LO
    assert torch.isnan(m0.view(-1, 4)[NAN_ROW, :3]).any() and not torch.isnan(m0.view(-1, 4)[NAN_ROW + 1]).any()
    assert _same(m0, m0_c)
    assert (m0[..., 3] == 0).all()
    if upd is None:
        assert y is None
    else:
        assert _same(y, y_c)
        assert (y[..., 3] == 0).all()
        ref = dpm.update_expr(upd, base, m0_c, h1, h2)   # and the chain is the reference's expression
        assert _same(y[..., :3], ref[..., :3])


def test_dpm_step_partial_block_and_bad_arguments():
    from slotdiffusion_amd import _lib, ops
    m, _, _ = ctx()
    code = m.bank().f(m.vq_key)
    upd, e = _update_of(dpm.UPD_MULTI2)
    g = torch.Generator().manual_seed(3)
    x, out, base, h1 = (torch.randn(7, 11, 4, generator=g).cuda() for _ in range(4))        # 77 rows: 1 1/4 blocks
    idx_c, m0_c, y_c = _chain(ops, x, out, code, e, m.z_scale, 'eps', upd, base, h1, None)
    m0, y, idx = ops.dpm_step(x, out, code, e, scale=m.z_scale, upd=upd, base=base, h1=h1, want_idx=True)
    assert torch.equal(idx, idx_c) and torch.equal(m0[..., :3], m0_c[..., :3]) and torch.equal(y[..., :3], y_c[..., :3])
    with pytest.raises(_lib.SdmiError):
        _lib.call('sdmi_dpm_step', None, x=16, out=16, codebook=16, m0=16, R=4, n_codes=16, alpha=1., scale=1.,
                  mode=dpm.UPD_MULTI3, base=16, y=16, h1=16)                                 # third order without h2
    with pytest.raises(_lib.SdmiError):
        _lib.call('sdmi_dpm_step', None, x=16, out=16, codebook=16, m0=16, R=4, n_codes=9000, alpha=1., scale=1.)


@pytest.mark.parametrize('tag,kw', CONFIGS, ids=[t for t, _ in CONFIGS])
def test_reference_configurations_fp32(tag, kw):
    """Every stored state and the final latent within 1e-4 of the reference's, identical final VQ indices, recon PSNR
    within 1e-4 dB (the bars of test_dpm_solver_sampling_fp32)."""
    from oracle import slotdiff_oracle as O
    m, G, img = ctx()
    F = family()
    dm = m.dm_decoder
    if 't_start' in kw:
        noise = F[tag + '/noise'] if tag + '/noise' in F else G['noise']
        x_T = dm.noise_latent(G['x0'].cuda(), kw['t_start'], noise.cuda())
        err = float((x_T.cpu() - F[tag + '/x_T']).abs().max())
        print(tag, 'noise_latent max-abs error', err)
        assert err <= 1e-6                     # two fp32 products and a sum of O(1) values: a few ulp at most
    else:
        x_T = (F[tag + '/x_T'] if tag + '/x_T' in F else G['x_T']).cuda()
    x, inter = dm.generate_imgs(cond=G['slots'].cuda(), batch_size=2, x_T=x_T, ret_intermed=True, **_kw(kw))
    assert inter.shape[0] == int(F[tag + '/n_inter'])
    errs = [float((inter[int(i)].cpu() - F[tag + '/inter'][j]).abs().max()) for j, i in enumerate(F[tag + '/inter_idx'])]
    final = float((x.cpu() - F[tag + '/final']).abs().max())
    idx = dm.vae.quantize_indices(x).cpu()
    agree = float((idx == F[tag + '/final_idx'].long()).float().mean())
    ps = O.psnr(dm.vae.decode(x).cpu(), img.cpu())
    dps = float((ps.double() - F[tag + '/recon_psnr'].double()).abs().max())
    print(tag, 'state errors', errs, 'final', final, 'code agreement', agree, 'recon psnr diff (dB)', dps)
    assert max(errs) <= BAR and final <= BAR
    assert agree == 1.0
    assert dps <= 1e-4
    x2 = dm.generate_imgs(cond=G['slots'].cuda(), batch_size=2, x_T=x_T, **_kw(kw))          # without intermediates
    assert torch.equal(x2, x)


@pytest.mark.parametrize('target', TARGETS)
def test_default_equals_the_parent_launch_chain(target):
    """The default (omitting the keywords, or spelling them) runs one sdmi_dpm_step per evaluation, and its final latent
    and every intermediate state are bit-identical to the launches it ran before the fused tail: the same program with
    sdmi_lincomb / sdmi_vq_nearest (_chain) behind the same UNet evaluator."""
    from slotdiffusion_amd import _lib, ops
    m, G, _ = ctx()
    dm = m.dm_decoder
    cond, x_T = G['slots'].cuda(), G['x_T'].cuda()
    assert not m.use_graph                               # (the graph and plan caches do not key on the target)
    calls = []
    real = _lib._call

    def spy(fname, stream, **kw):
        calls.append(fname)
        return real(fname, stream, **kw)
    x_in = ops.nchw_to_nhwc(x_T, torch.float32, 4)
    m._evaluator(cond, [0.], zero_pad=False)(x_in)       # one evaluation: the lazy weight preparation is no launch list
    was = dm.pred_target
    dm.pred_target = target
    _lib._call = spy
    try:
        a = dm.generate_imgs(cond=cond, batch_size=2, x_T=x_T)
        n_default = list(calls)
        del calls[:]
        b = dm.generate_imgs(cond=cond, batch_size=2, x_T=x_T, dpm_steps=20, dpm_order=3, dpm_method='singlestep',
                             dpm_skip_type='time_uniform')
        n_spelled = list(calls)
        del calls[:]
        dm.generate_imgs(cond=cond, batch_size=2, x_T=x_T, dpm_method='multistep', dpm_order=2, dpm_steps=10)
        n_multi = list(calls)
        _lib._call = real
        x, inter = m._dpm_sample(x_in, cond, ret_intermed=True)
        plan = dpm.build_plan(dm.betas.detach().cpu())
        ev = m._evaluator(cond, dpm.plan_t_inputs(plan), zero_pad=False)

        def tail(xc, e, upd, base, h1, h2):
            return _chain(ops, xc, ev(xc), ev.code, e, m.z_scale, target, upd, base, h1, h2)[1:]
        x_c, inter_c = dpm.run_program(dpm.program(plan), x_in, tail)
        torch.cuda.synchronize()
    finally:
        _lib._call = real
        dm.pred_target = was
    assert torch.equal(a, b) and n_default == n_spelled
    assert n_default.count('sdmi_dpm_step') == 20 and 'sdmi_vq_nearest' not in n_default
    assert n_multi.count('sdmi_dpm_step') == 10 and 'sdmi_vq_nearest' not in n_multi
    assert ev.n == 20 and len(inter) == len(inter_c) == 7          # one state per outer step, no initial state
    assert _same(ops.nhwc_to_nchw(x, 3), a)                      # with and without intermediates: the same latent
    for got, want in zip([x] + inter, [x_c] + inter_c):
        assert _same(got[..., :3], want[..., :3])
        assert (got[..., 3] == 0).all()
    if target == 'eps':
        assert float((a.cpu() - G['dpm_final']).abs().max()) <= BAR


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['fp32', 'bf16'])
def test_graph_replay_alternating_configurations(dtype):
    """Two configurations used alternately, and the default before and after: every replay equals the eager loop of the
    same configuration and dtype bit for bit -- no entry evicts or aliases another's static buffers."""
    m, G, _ = ctx(dtype)
    dm = m.dm_decoder
    cond, x_T = G['slots'].cuda(), G['x_T'].cuda()
    A = _kw(dict(method='multistep', order=2, steps=10))
    Bc = _kw(dict(method='singlestep_fixed', order=3, steps=9, skip_type='logSNR', denoise_to_zero=True))
    run = lambda kw, x=x_T: dm.generate_imgs(cond=cond, batch_size=2, x_T=x, **kw).clone()
    assert not m.use_graph
    eager = {k: run(kw) for k, kw in (('d', {}), ('a', A), ('b', Bc))}
    x_T2 = torch.flip(x_T, [0])
    eager_a2 = run(A, x_T2)
    m.use_graph = True
    try:
        n0 = len(m._graph_cache)
        seq = [('d', {}), ('a', A), ('b', Bc), ('a', A), ('b', Bc), ('d', {})]
        got = [(k, run(kw)) for k, kw in seq]
        assert len(m._graph_cache) == n0 + 3
        for k, v in got:
            assert torch.equal(v, eager[k]), k
        assert torch.equal(run(A, x_T2), eager_a2) and torch.equal(run(A), eager['a'])       # replay with new inputs
    finally:
        m.use_graph = False
        m._graph_cache.clear()
    assert not torch.equal(eager['a'], eager['b']) and torch.isfinite(eager['b']).all()


def test_video_log_images_multistep():
    """SAViDiffusion.log_images forwards the solver keywords through the flattened B*T frames: [B,T,3,H,W] samples that
    match the per-frame sampler calls with the same slots and noise (latent bar 1e-4 -> decoded images far above the
    80 dB PSNR the default sampler test asks of a matching decode)."""
    from oracle import slotdiff_oracle as O
    from slotdiffusion_amd.models import SAViDiffusion
    from tests.detfill import det_fill_, is_buffer_name
    cfg = C.movie_cfg()
    T = 3
    m = SAViDiffusion(cfg['resolution'], T, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'],
                      cfg['loss_dict'], compute_dtype=torch.float32)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    m = m.cuda().eval()
    m.use_graph = False
    img = C.make_inputs(T, seed=11)[0].view(1, T, 3, 128, 128).cuda()
    x_T = torch.randn(T, 3, 32, 32, generator=torch.Generator().manual_seed(23)).cuda()
    kw = dict(dpm_method='multistep', dpm_order=2, dpm_steps=10)
    log = m.log_images(dict(img=img), x_T=x_T, **kw)
    assert log['samples'].shape == (1, T, 3, 128, 128) and torch.isfinite(log['samples']).all()
    with torch.no_grad():
        slots = m(dict(img=img))['slots']
    dm = m.dm_decoder
    for t in range(T):
        z = dm.generate_imgs(cond=slots[:, t].contiguous(), batch_size=1, x_T=x_T[t:t + 1], **kw)
        frame = dm.vae.decode(z)
        ps = float(O.psnr(log['samples'][:, t].cpu(), frame.cpu()).min())
        print('frame', t, 'max-abs', float((log['samples'][:, t] - frame).abs().max()), 'psnr', ps)
        assert ps > 80.
