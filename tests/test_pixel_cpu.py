"""The image-space decoder (CondDDPM) without a device: parameter layouts against the reference's state-dict key lists, the
decoder class build_model chooses, the host restatement of dynamic thresholding -- the (k, w) quantile position the
kernels are given, two order statistics and ATen's lerp -- against torch.quantile and against the reference's
DPM_Solver.dynamic_thresholding_fn (tests/golden/dyn_thresh.npz), and the option checks / cache keys."""
import copy
from fractions import Fraction

import numpy as np
import pytest
import torch

from slotdiffusion_amd import dpm, spec, unipc
from tests import common as C

RATIOS = (0.995, 0.5, 1.0)
SIZES = ((16, 16), (32, 32), (33, 31))


def px_cfg(video=False):
    """The CLEVRTex / MOVi-E configuration with the image-space decoder at 32 x 32: no `vae_dict`, no z_scale_factor."""
    cfg = C.movie_cfg() if video else C.clevrtex_cfg()
    cfg = copy.deepcopy(cfg)
    cfg['resolution'] = (32, 32)
    cfg['slot_dict']['num_slots'] = 7
    cfg['dec_dict']['resolution'] = (32, 32)
    del cfg['dec_dict']['vae_dict']
    cfg['dec_dict']['diffusion_dict'].pop('z_scale_factor', None)
    return cfg


def test_spec_key_order_equals_the_reference():
    G = np.load(C.GOLD + '/sadiff_px_b2.npz')
    cfg = px_cfg()
    sp = spec.sa_diffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'])
    assert [p.name for p in sp] == list(G['keys'])
    assert not any('.vae.' in k for k in G['keys'])
    V = np.load(C.GOLD + '/savidiff_px_b1t2.npz')
    cfg = px_cfg(video=True)
    sp = spec.savi_diffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'])
    assert [p.name for p in sp] == list(V['keys'])
    # and with an EMPTY vae_dict, the reference's other spelling of "no VAE" (sa_diffusion.py:144)
    cfg['dec_dict']['vae_dict'] = {}
    sp2 = spec.savi_diffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'])
    assert [p.name for p in sp2] == list(V['keys'])


def test_build_model_chooses_the_decoder():
    from slotdiffusion_amd import models
    for vae in ('absent', {}, None):
        cfg = px_cfg()
        if vae != 'absent':
            cfg['dec_dict']['vae_dict'] = vae
        m = models.build_model(C.Params(model='SADiffusion', **cfg))
        dm = m.dm_decoder
        assert type(dm) is models.CondDDPM and dm.clip_denoised and not dm.vq_denoised and not hasattr(dm, 'vae')
        assert m.latent_res == (32, 32) and m.z_scale == 1.0
    mv = models.build_model(C.Params(model='SAViDiffusion', input_frames=2, **px_cfg(video=True)))
    assert type(mv.dm_decoder) is models.CondDDPM
    m = models.build_model(C.make_params('SADiffusion'))
    assert type(m.dm_decoder) is models.LDM and m.dm_decoder.vq_denoised and hasattr(m.dm_decoder, 'vae')
    # refused by name
    cfg = px_cfg()
    cfg['dec_dict']['unet_dict']['in_channels'] = 4
    with pytest.raises(ValueError, match='in_channels'):
        models.build_model(C.Params(model='SADiffusion', **cfg))
    cfg = px_cfg()
    cfg['dec_dict']['unet_dict']['out_channels'] = 6
    with pytest.raises(ValueError, match='out_channels'):
        models.build_model(C.Params(model='SADiffusion', **cfg))
    cfg = px_cfg()
    cfg['dec_dict']['conditioning_key'] = 'concat'
    with pytest.raises(ValueError, match='conditioning_key'):
        models.build_model(C.Params(model='SADiffusion', **cfg))
    for ch in (3, 4):                                    # the reason given is the rollouter's, whatever else is off
        cfg = px_cfg()
        cfg['dec_dict']['unet_dict']['in_channels'] = ch
        with pytest.raises(ValueError, match='LDMSlotFormer'):
            models.LDMSlotFormer((32, 32), 6, cfg['slot_dict'], cfg['dec_dict'],
                                 dict(num_slots=7, slot_size=192, history_len=6, d_model=256, num_layers=4, num_heads=8,
                                      ffn_dim=1024, norm_first=True, t_pe='sin', slots_pe=''), dict(rollout_len=4))
    dm = models.CondDDPM.__new__(models.CondDDPM)
    object.__setattr__(dm, '_root_ref', None)
    with pytest.raises(ValueError, match='ret_intermed'):
        models.CondDDPM.log_images(dm, dict(slots=torch.zeros(1, 7, 192)), ret_intermed=True)


# ---- host restatement of the correction ---------------------------------------------------------------------------------
def _round32(fr):
    """Fraction -> the nearest float32 (ties to even): one rounding, as an fma makes."""
    c = np.float32(float(fr))
    best = None
    for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        d = abs(Fraction(float(v)) - fr)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even and not best[2]):
            best = (d, v, even)
    return np.float32(best[1])


def thresh_host(x0, ratio, max_val):
    """x0 [B, ...] float32 numpy -> (corrected x0, s): what sdmi_dpm_step_px computes, restated on the host (sdmi.h)."""
    from slotdiffusion_amd import ops
    B = x0.shape[0]
    a = np.sort(np.abs(x0.reshape(B, -1)), axis=1)
    n = a.shape[1]
    k, w = ops.quantile_rank(n, ratio)
    w = np.float32(w)
    s = np.empty(B, np.float32)
    for b in range(B):
        lo = a[b, k]
        hi = a[b, k + 1] if w != 0 else lo
        d = np.float32(hi - lo)
        if w < np.float32(0.5):
            v = _round32(Fraction(float(w)) * Fraction(float(d)) + Fraction(float(lo)))
        else:
            v = _round32(Fraction(float(hi)) - Fraction(float(d)) * Fraction(float(np.float32(1) - w)))
        s[b] = max(v, np.float32(max_val))
    sb = s.reshape((B,) + (1,) * (x0.ndim - 1))
    return (np.clip(x0, -sb, sb) / sb).astype(np.float32), s


def _thresh_torch(x0, ratio, max_val):
    """dpm_solver.py:506-515, op for op."""
    s = torch.quantile(torch.abs(x0).reshape((x0.shape[0], -1)), ratio, dim=1)
    s = torch.maximum(s, max_val * torch.ones_like(s))
    sb = s.view((-1,) + (1,) * (x0.dim() - 1))
    return torch.clamp(x0, -sb, sb) / sb, s


@pytest.mark.parametrize('ratio', RATIOS)
def test_host_restatement_equals_torch_quantile_thresholding(ratio):
    g = torch.Generator().manual_seed(int(ratio * 1000))
    for h, w in SIZES:
        x0 = torch.randn(6, 3, h, w, generator=g)
        x0[1] *= torch.exp(2 * torch.randn(3, h, w, generator=g))      # wide gaps between neighbouring order statistics
        x0[2] = torch.randint(-24, 25, (3, h, w), generator=g).float() / 8.
        x0[3] = torch.exp(4 * torch.randn(3, h, w, generator=g))
        x0[4] = 0.3
        for mv in (1.0, 0.01):
            want, s_want = _thresh_torch(x0, ratio, mv)
            got, s = thresh_host(x0.numpy(), ratio, mv)
            assert np.array_equal(s, s_want.numpy()) and np.array_equal(got, want.numpy())
    if ratio == 0.5:
        from slotdiffusion_amd import ops
        assert ops.quantile_rank(3 * 33 * 31, 0.5) == (1534, 0.0)       # odd n: the weight is exactly 0
    if ratio == 1.0:
        from slotdiffusion_amd import ops
        assert ops.quantile_rank(3 * 32 * 32, 1.0) == (3071, 0.0)       # the maximum


def test_host_restatement_equals_the_reference_fixture():
    G = np.load(C.GOLD + '/dyn_thresh.npz')
    for h, w in SIZES:
        x0 = G[f'x0_{h}x{w}']
        assert x0.shape[1:] == (3, h, w)
        for ratio in RATIOS:
            for mv in (1.0, 0.25):
                got, s = thresh_host(x0, ratio, mv)
                assert np.array_equal(s, G[f's_{h}x{w}_q{ratio}_m{mv}'])
                assert np.array_equal(got, G[f'out_{h}x{w}_q{ratio}_m{mv}'])
        assert (G[f's_{h}x{w}_q0.995_m1.0'][[0]] == 1.0).all() and G[f's_{h}x{w}_q0.995_m1.0'][1] > 1.0


# ---- options and keys -----------------------------------------------------------------------------------------------------
def test_option_checks_and_cache_keys():
    from slotdiffusion_amd.models import SADiffusion
    for mod in (dpm, unipc):
        for fn in ('dynamic_thresholding', True, False, None):
            mod.check_options(correcting_x0_fn=fn, vq_denoised=False)
        for fn in ('dynamic_thresholding', True):                  # the latent decoder: refused as before
            with pytest.raises(ValueError, match='correcting_x0_fn'):
                mod.check_options(correcting_x0_fn=fn)
            with pytest.raises(ValueError, match='correcting_x0_fn'):
                mod.check_options(correcting_x0_fn=fn, vq_denoised=True)
        with pytest.raises(ValueError, match='correcting_x0_fn'):
            mod.check_options(correcting_x0_fn='clip', vq_denoised=False)
        for bad in (0.0, -0.1, 1.5):
            with pytest.raises(ValueError, match='dynamic_thresholding_ratio'):
                mod.check_options(vq_denoised=False, dynamic_thresholding_ratio=bad)
        for bad in (0.0, -1.0):
            with pytest.raises(ValueError, match='thresholding_max_val'):
                mod.check_options(vq_denoised=False, thresholding_max_val=bad)
        mod.check_options(vq_denoised=False, dynamic_thresholding_ratio=1.0, thresholding_max_val=0.5)
    # the correction is not in the plan key (the time grid does not depend on it) ...
    assert dpm.plan_key() == (20, 3, 'singlestep', 'time_uniform', None, None, True, False)
    assert dpm.plan_key(15, 2, 'multistep', 'logSNR', 0.6, 1e-3, False, True) == \
        (15, 2, 'multistep', 'logSNR', 0.6, 1e-3, False, True)
    assert unipc.plan_key()[1:3] == (20, 3) and len(unipc.plan_key()) == len(unipc.plan_key(steps=7, order=2))
    # ... but an extra element of the graph key; every existing key is what it was
    on = dpm.correct_key(True)
    off = dpm.correct_key(False)
    assert on == ('dynamic', 0.995, 1.0) and off == ('none', 0., 0.)
    assert dpm.correct_key(False, 'dynamic_thresholding', 0.9, 2.0) == ('dynamic', 0.9, 2.0)
    assert dpm.correct_key(False, True) == on and dpm.correct_key(True, False) == on and dpm.correct_key(True, None) == on
    for keyfn, pk in ((SADiffusion.dpm_cache_key, dpm.plan_key), (SADiffusion.unipc_cache_key, unipc.plan_key)):
        plain = keyfn(2, (2, 7, 192), 20)
        assert plain == (2, pk(20), (2, 7, 192))
        assert keyfn(2, (2, 7, 192), 20, correct=on) == plain + (on,)
        assert len({plain, keyfn(2, (2, 7, 192), 20, correct=on), keyfn(2, (2, 7, 192), 20, correct=off),
                    keyfn(2, (2, 7, 192), 20, correct=('dynamic', 0.9, 1.0))}) == 4


def test_generate_imgs_checks_follow_the_decoder():
    """On a bare CondDDPM the thresholding keywords pass the check (and bad values are refused by name) before anything
    touches the device; a bare LDM still refuses them (tests/test_dpm_family_cpu.py pins that)."""
    from slotdiffusion_amd.models import LDM, CondDDPM
    cond = torch.zeros(1, 7, 192)
    for cls in (LDM, CondDDPM):
        dm = cls.__new__(cls)
        object.__setattr__(dm, '_root_ref', None)
        for kw, name in ((dict(dpm_dynamic_thresholding_ratio=0.), 'dynamic_thresholding_ratio'),
                         (dict(dpm_thresholding_max_val=-1.), 'thresholding_max_val'),
                         (dict(use_unipc=True, unipc_dynamic_thresholding_ratio=2.), 'dynamic_thresholding_ratio'),
                         (dict(use_unipc=True, unipc_thresholding_max_val=0.), 'thresholding_max_val'),
                         (dict(guidance_scale=3.), 'guidance_scale')):
            with pytest.raises(ValueError, match=name):
                cls.generate_imgs(dm, cond, batch_size=1, **kw)
    dm = LDM.__new__(LDM)
    object.__setattr__(dm, '_root_ref', None)
    with pytest.raises(ValueError, match='correcting_x0_fn'):
        LDM.generate_imgs(dm, cond, batch_size=1, dpm_correcting_x0_fn=True)
