"""Generate the image-space (CondDDPM) fixtures under tests/golden/ from the REAL reference (build container only).

    python tools/gen_golden_px.py [dyn|img|video]        # default: all three

dyn_thresh.npz      DPM_Solver.dynamic_thresholding_fn on hand-made x0 [B,3,h,w] -> corrected x0 and s
sadiff_px_b2.npz    img_based SADiffusion, CLEVRTex config with an EMPTY vae_dict (decoder = CondDDPM) at image and decoder
                    resolution 32 x 32, num_slots 7: state_dict keys, loss and gradient norms at fixed t / noise (eps and
                    x0), every state of the default 20-evaluation DPM-Solver++ run (dynamic thresholding on:
                    clip_denoised = True), five ancestral steps, a 10-step DDIM run
savidiff_px_b1t2.npz  the video twin at B = 1, T = 2: keys, loss (eps and v targets), final sample
Weights are tests/detfill.py's on both sides and never stored; only data is written (no reference code).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))
import ref_harness as rh                      # noqa: E402
from tests.detfill import det_fill_, is_buffer_name   # noqa: E402

OUT = os.path.join(HERE, '..', 'tests', 'golden')
RES = 32
THRESH_RATIOS = (0.995, 0.5, 1.0)
THRESH_SIZES = ((16, 16), (32, 32), (33, 31))


def thresh_inputs(h, w, seed=3):
    """x0 [5,3,h,w]: all |x0| < 1, heavy-tailed, multiples of 1/8, constant, plain normal."""
    g = torch.Generator().manual_seed(seed + 131 * h + w)
    x = torch.randn(5, 3, h, w, generator=g)
    x[0] = torch.rand(3, h, w, generator=g) * 1.8 - 0.9
    x[1] = x[1] * torch.exp(torch.randn(3, h, w, generator=g))
    x[2] = torch.randint(-24, 25, (3, h, w), generator=g).float() / 8.
    x[3] = 1.375
    return x


def px_inputs(B, seed=7, res=RES):
    g = torch.Generator().manual_seed(seed)
    img = (torch.randn(B, 3, res, res, generator=g) * 0.5).clamp(-1, 1)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, res), torch.linspace(-1, 1, res), indexing='ij')
    for b in range(B):
        for k in range(3):
            cy, cx = torch.rand(2, generator=g) * 1.6 - 0.8
            col = torch.rand(3, generator=g) * 2 - 1
            blob = (((yy - cy) ** 2 + (xx - cx) ** 2) < 0.1).float()
            img[b] = img[b] * (1 - blob) + (col[:, None, None] + 0.1 * img[b]) * blob
    img = img.clamp(-1, 1)
    t = torch.tensor(([37, 812] + [500, 3, 999, 250, 640, 77])[:B])
    noise = torch.randn(B, 3, res, res, generator=g)
    x_T = torch.randn(B, 3, res, res, generator=g)
    return img, t, noise, x_T


def _save(name, G):
    arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in G.items()}
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, name), **arrs)
    print('wrote', name, {k: (tuple(v.shape), str(v.dtype)) for k, v in arrs.items()})


def main_dyn():
    rh.install()
    from slotdiffusion.img_based.models.ddpm import dpm_solver as ds
    ns = ds.NoiseScheduleVP(betas=torch.linspace(0.0015, 0.0195, 1000))
    G = {}
    for h, w in THRESH_SIZES:
        x0 = thresh_inputs(h, w)
        G[f'x0_{h}x{w}'] = x0
        for q in THRESH_RATIOS:
            for mv in (1.0, 0.25):
                sol = ds.DPM_Solver(lambda x, t: x, ns, algorithm_type='dpmsolver++', correcting_x0_fn='dynamic_thresholding',
                                    dynamic_thresholding_ratio=q, thresholding_max_val=mv, vq_denoised=False)
                got = sol.dynamic_thresholding_fn(x0.clone(), None)
                s = torch.quantile(torch.abs(x0).reshape((x0.shape[0], -1)), q, dim=1)
                G[f'out_{h}x{w}_q{q}_m{mv}'] = got
                G[f's_{h}x{w}_q{q}_m{mv}'] = torch.maximum(s, mv * torch.ones_like(s))
    _save('dyn_thresh.npz', G)


def _img_params(target):
    P = rh.ref_params('img_based', 'sa_ldm', 'sa_ldm_clevrtex_params-res128')
    P.resolution = (RES, RES)
    P.slot_dict['num_slots'] = 7
    P.dec_dict['resolution'] = (RES, RES)
    P.dec_dict.pop('vae_dict')                       # (CondDDPM takes no such keyword: absent, not empty)
    P.dec_dict['diffusion_dict'].pop('z_scale_factor', None)   # (an LDM-only entry: DDPM.register_schedule refuses it)
    P.dec_dict['diffusion_dict']['pred_target'] = target
    return P


def _loss_and_grads(model, dm, img, t, noise, target, G, pre, every=1):
    model.train()
    dm.model.eval()                   # disables the ResBlock dropout only
    for p in model.parameters():
        p.grad = None
    out = model(dict(img=img))
    x0 = img
    xt = dm._sample_xt_from_x0(x0=x0, t=t, noise=noise)
    pred = dm.forward(xt, t, context=out['slots'])
    if target == 'eps':
        gt = noise
    elif target == 'v':                                # ldm.py:74-78: v = alpha_t * noise - sigma_t * x0
        a = dm.sqrt_alphas_bar[t].view(-1, 1, 1, 1)
        s = dm.sqrt_one_minus_alphas_bar[t].view(-1, 1, 1, 1)
        gt = a * noise - s * x0
    else:
        gt = x0
    loss = torch.nn.functional.mse_loss(pred, gt)
    loss.backward()
    G[pre + 'denoise_loss'] = loss.detach()
    if target == 'eps':
        G['x_t'], G['pred'] = xt.detach(), pred.detach()
    named = dict(model.named_parameters())
    names = sorted(n for n, p in named.items() if p.grad is not None)[::every]
    G[pre + 'grad_norms_names'] = np.array(names)
    G[pre + 'grad_norms'] = torch.tensor([float(named[n].grad.norm()) for n in names])
    G[pre + 'grad_global_norm'] = torch.tensor(sum(float((p.grad.double() ** 2).sum()) for p in named.values()
                                                   if p.grad is not None) ** 0.5)
    model.eval()


def main_img():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    im = rh.ref_models('img_based')
    import slotdiffusion.img_based.models.ddpm.cond_ddpm as cd
    from slotdiffusion.img_based.models.ddpm import dpm_solver as ds
    img, t, noise, x_T = px_inputs(2)
    G = dict(img=img, t=t, noise=noise, x_T=x_T)
    for target in ('eps', 'x0'):                      # (only video_based accepts 'v': ddpm.py:79; see main_video)
        model = im.build_model(_img_params(target))
        dm = model.dm_decoder
        assert type(dm).__name__ == 'CondDDPM' and dm.clip_denoised and not dm.vq_denoised and not hasattr(dm, 'vae')
        assert dm.pred_target == target
        det_fill_(model.state_dict().items(), skip=is_buffer_name)
        pre = '' if target == 'eps' else 'x0_'
        _loss_and_grads(model, dm, img, t, noise, target, G, pre, every=1 if target == 'eps' else 16)
        if target != 'eps':
            continue
        G['keys'] = np.array(list(model.state_dict().keys()))
        with torch.no_grad():
            slots, _ = model.encode(img)
        G['slots'] = slots
        # the default sampler of CondDDPM.generate_imgs (cond_ddpm.py:155-193): 20 evaluations, thresholding on
        ns = ds.NoiseScheduleVP(betas=dm.betas)
        with torch.no_grad():
            model_fn = ds.model_wrapper(model=dm.model, noise_schedule=ns, model_type='noise',
                                        guidance_type='classifier-free', condition=slots)
            sampler = ds.DPM_Solver(model_fn, ns, algorithm_type='dpmsolver++', correcting_x0_fn=dm.clip_denoised,
                                    vq_denoised=dm.vq_denoised)
            x, inter = sampler.sample(x_T.clone(), steps=20, order=3, method='singlestep', return_intermediate=True)
        G['dpm_trace'], G['dpm_final'] = torch.stack(inter, 0), x
        # the first five ancestral steps (explicit noise), clip_denoised = True
        nz = torch.randn(x_T.shape, generator=torch.Generator().manual_seed(77))
        G['anc_noise'] = nz
        cd.noise_like = lambda shape, device, repeat=False: nz.clone()
        ts = [999, 998, 997, 996, 995]
        G['anc_t'] = torch.tensor(ts)
        outs, xx = [], x_T.clone()
        with torch.no_grad():
            for tv in ts:
                xx = dm._p_sample(xx, torch.full((2,), tv, dtype=torch.long), slots, clip_denoised=True,
                                  vq_denoised=False)
                outs.append(xx)
        G['anc_x'] = torch.stack(outs, 0)
        # DDIM, 10 steps, eta = 0
        from slotdiffusion.video_based.models.ddpm import ddim as dd      # (img_based's ddim.py re-exports this module)
        dd.DDIMSampler.register_buffer = lambda self, name, attr: setattr(self, name, attr)
        dsamp = dd.DDIMSampler(dm, schedule=dm.beta_schedule)
        dd.noise_like = lambda shape, device, repeat=False: x_T.clone()
        with torch.no_grad():
            xd, interd = dsamp.generate_imgs(10, tuple(x_T.shape), conditioning=slots, eta=0., verbose=False,
                                             log_every_t=1, ret_intermed=True)
        G['ddim_inter'] = interd                         # (its last entry is the final sample)
    _save('sadiff_px_b2.npz', G)


def main_video(T=2):
    torch.manual_seed(0)
    torch.set_num_threads(8)
    vm = rh.ref_models('video_based')
    from slotdiffusion.video_based.models.ddpm import dpm_solver as ds
    P = rh.ref_params('video_based', 'savi_ldm', 'savi_ldm_movie_params-res128')
    P.resolution = (RES, RES)
    P.slot_dict['num_slots'] = 7
    P.dec_dict['resolution'] = (RES, RES)
    P.dec_dict.pop('vae_dict')                       # (CondDDPM takes no such keyword: absent, not empty)
    P.dec_dict['diffusion_dict'].pop('z_scale_factor', None)   # (an LDM-only entry: DDPM.register_schedule refuses it)
    P.n_sample_frames = P.input_frames = T
    model = vm.build_model(P)
    dm = model.dm_decoder
    assert type(dm).__name__ == 'CondDDPM' and dm.clip_denoised and not dm.vq_denoised
    det_fill_(model.state_dict().items(), skip=is_buffer_name)
    img, t, noise, x_T = px_inputs(T)
    vid = img[None]                                                  # [1,T,3,H,W]
    G = dict(img=vid, t=t, noise=noise, x_T=x_T, keys=np.array(list(model.state_dict().keys())))
    model.eval()
    with torch.no_grad():
        out = model(dict(img=vid))
        slots = out['slots'] if 'slots' in out else out['post_slots']
        G['slots'] = slots
        s2 = slots.flatten(0, 1)
        xt = dm._sample_xt_from_x0(x0=img, t=t, noise=noise)
        pred = dm.forward(xt, t, context=s2)
        G['denoise_loss'] = torch.nn.functional.mse_loss(pred, noise)
        # the same weights as a v-prediction model (the loss target of ldm.py:74-78 on the image itself)
        dm.pred_target = 'v'
        a = dm.sqrt_alphas_bar[t].view(-1, 1, 1, 1)
        s = dm.sqrt_one_minus_alphas_bar[t].view(-1, 1, 1, 1)
        G['v_denoise_loss'] = torch.nn.functional.mse_loss(dm.forward(xt, t, context=s2), a * noise - s * img)
        dm.pred_target = 'eps'
        ns = ds.NoiseScheduleVP(betas=dm.betas)
        model_fn = ds.model_wrapper(model=dm.model, noise_schedule=ns, model_type='noise',
                                    guidance_type='classifier-free', condition=s2)
        sampler = ds.DPM_Solver(model_fn, ns, algorithm_type='dpmsolver++', correcting_x0_fn=dm.clip_denoised,
                                vq_denoised=dm.vq_denoised)
        G['dpm_final'] = sampler.sample(x_T.clone(), steps=20, order=3, method='singlestep')
    _save('savidiff_px_b1t2.npz', G)


if __name__ == '__main__':
    what = sys.argv[1:] or ['dyn', 'img', 'video']
    for w in what:
        {'dyn': main_dyn, 'img': main_img, 'video': main_video}[w]()
