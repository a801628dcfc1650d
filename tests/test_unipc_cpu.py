"""Host side of UniPC (slotdiffusion_amd/unipc.py) on an analytic problem: the exact denoiser of a 1-D Gaussian
N(MU, S^2) on the shipped linear schedule, whose probability-flow ODE has a closed-form solution.  Local order of the
predictor and the corrector, the constant-model identity, the order / corrector sequences, the whole-trajectory error
against the shipped third-order multistep DPM-Solver++, refusals, cache keys and the entry point's argument checks.
No GPU; everything in float64."""
import inspect
import math

import pytest
import torch

from slotdiffusion_amd import _lib, dpm, module, unipc

MU, S = 0.7, 0.5
F64 = torch.float64
# the configurations whose cache keys must differ from the default's, and the other plans the tests below build
KEYED = [dict(steps=10), dict(order=2), dict(variant='bh1'), dict(skip_type='logSNR'),
         dict(skip_type='time_quadratic'), dict(t_start=0.6), dict(t_end=1e-4), dict(lower_order_final=False),
         dict(corrector=False), dict(denoise_to_zero=True)]
BUILT = [dict(steps=10, order=3), dict(steps=10, order=3, denoise_to_zero=True), dict(steps=10, order=3, corrector=False),
         dict(steps=5, t_start=0.6, t_end=0.01), dict(steps=20, order=3, variant='bh2', skip_type='logSNR'),
         dict(steps=40, order=3, variant='bh2', skip_type='logSNR')]


def betas64():
    return torch.tensor(module.ddpm_schedule(1000, 'linear', 0.0015, 0.0195)['betas'], dtype=F64)


def sched():
    return dpm.DiscreteSchedule(betas64(), dtype=F64)


def _t(v):
    return torch.as_tensor(v, dtype=F64).reshape(1)


def toy_m(ns, x, t):
    """E[x_0 | x_t = x] for x_0 ~ N(MU, S^2)."""
    a, sg = float(ns.alpha(_t(t))), float(ns.std(_t(t)))
    return MU + a * S * S / (a * a * S * S + sg * sg) * (x - a * MU)


def toy_exact(ns, x_ref, t_ref, t):
    """The ODE solution through (t_ref, x_ref), at t."""
    a, sg = float(ns.alpha(_t(t))), float(ns.std(_t(t)))
    ar, sr = float(ns.alpha(_t(t_ref))), float(ns.std(_t(t_ref)))
    return a * MU + (x_ref - ar * MU) * math.sqrt((a * a * S * S + sg * sg) / (ar * ar * S * S + sr * sr))


def _one_step(ns, h, o, variant, x_s=0.3):
    """One step of width h in lambda from lambda = -0.5 with exact history -> (|x_p - exact|, |x_c - exact|)."""
    lam_s = -0.5
    t_hist = [float(ns.inverse_lambda(_t(lam_s - k * h))) for k in range(o)]
    t = float(ns.inverse_lambda(_t(lam_s + h)))
    rec = unipc.step_record(ns, t_hist, t, o, variant, corrector=True)
    xs = [toy_exact(ns, x_s, t_hist[0], tk) for tk in t_hist]
    ms = [toy_m(ns, xk, tk) for xk, tk in zip(xs, t_hist)]
    x_ = rec['c0'] * x_s + rec['c1'] * ms[0]
    x_p = x_ + sum(q * (ms[k + 1] - ms[0]) for k, q in enumerate(rec['q']))
    m_new = toy_m(ns, x_p, t)
    x_c = x_ + sum(w * (ms[k + 1] - ms[0]) for k, w in enumerate(rec['w'])) + rec['wn'] * (m_new - ms[0])
    exact = toy_exact(ns, x_s, t_hist[0], t)
    return abs(x_p - exact), abs(x_c - exact)


@pytest.mark.parametrize('variant', unipc.VARIANTS)
@pytest.mark.parametrize('o', [1, 2, 3])
def test_local_order_of_predictor_and_corrector(o, variant):
    """Local error slope per halving of h (0.2 -> 0.1): theory o + 1 (predictor) and o + 2 (with corrector); the bar is
    theory less 0.2, a wrong coefficient costs a whole order."""
    ns = sched()
    p2, c2 = _one_step(ns, 0.2, o, variant)
    p1, c1 = _one_step(ns, 0.1, o, variant)
    sp, sc = math.log2(p2 / p1), math.log2(c2 / c1)
    print(f'order {o} {variant}: predictor error {p2:.3e} -> {p1:.3e} slope {sp:.2f}; '
          f'corrector {c2:.3e} -> {c1:.3e} slope {sc:.2f}')
    assert sp >= o + 0.8
    assert sc >= o + 1.8


def _run_unipc(ns, prog, x, model):
    def tail(xe, rec, base, h1, h2, h3):
        m0 = model(xe, rec['e']['t'])
        xc, y = unipc.update_expr(rec, base, m0, h1, h2, h3)
        return m0, xc, y
    return unipc.run_program(prog, x, tail)


@pytest.mark.parametrize('corrector', [True, False])
@pytest.mark.parametrize('variant', unipc.VARIANTS)
@pytest.mark.parametrize('order', [1, 2, 3])
def test_constant_model_is_integrated_exactly(order, variant, corrector):
    """m = c: every difference of predictions vanishes and the steps telescope to
    x_N = std_N / std_0 * x + alpha_N * (1 - exp(-(lambda_N - lambda_0))) * c."""
    ns = sched()
    c = 0.37
    x0 = torch.tensor([-1.3, 0.2, 2.1], dtype=F64)
    for skip in dpm.SKIP_TYPES:
        plan = unipc.build_plan(betas64(), steps=7, order=order, variant=variant, skip_type=skip, corrector=corrector)
        x, inter = _run_unipc(ns, unipc.program(plan), x0, lambda xe, t: torch.full_like(xe, c))
        t0, tN = plan['outer'][0].reshape(1), plan['outer'][-1].reshape(1)
        want = ns.std(tN) / ns.std(t0) * x0 + ns.alpha(tN) * (1. - torch.exp(-(ns.lam(tN) - ns.lam(t0)))) * c
        assert float((x - want).abs().max()) <= 1e-12, (skip, float((x - want).abs().max()))
        assert len(inter) == 8


def test_order_and_corrector_sequences():
    b = betas64()
    plan = unipc.build_plan(b, steps=10, order=3)
    assert plan['orders'] == [1, 2, 3, 3, 3, 3, 3, 3, 2, 1] == unipc.step_orders(10, 3)
    assert unipc.step_orders(10, 3, lower_order_final=False) == [1, 2] + [3] * 8
    assert unipc.step_orders(5, 2) == [1, 2, 2, 2, 1] and unipc.step_orders(3, 3) == [1, 2, 1]
    prog = unipc.program(plan)
    assert len(prog) == 10 and len(unipc.plan_t_inputs(plan)) == 10
    assert prog[0]['corr'] is None                                   # nothing to correct before the first step
    assert [r['corr']['order'] for r in prog[1:]] == plan['orders'][:9]
    assert [r['pred']['order'] for r in prog] == plan['orders']
    assert plan['steps'][-1]['wn'] is None and all(st['wn'] is not None for st in plan['steps'][:-1])
    d0 = unipc.build_plan(b, steps=10, order=3, denoise_to_zero=True)
    pd = unipc.program(d0)
    assert len(pd) == 11 and pd[-1]['corr'] is None and pd[-1]['pred'] is None and pd[:10] == prog
    assert pd[-1]['e']['t'] == float(d0['outer'][-1]) == 1. / 1000
    off = unipc.program(unipc.build_plan(b, steps=10, order=3, corrector=False))
    assert len(off) == 10 and all(r['corr'] is None for r in off)
    assert [r['pred'] for r in off] == [r['pred'] for r in prog]      # UniP alone: the same predictors
    z = torch.zeros(1, dtype=F64)
    for p, n in ((prog, 11), (pd, 12), (off, 11)):
        _, inter = unipc.run_program(p, z, lambda xe, rec, base, h1, h2, h3: (
            z, z if rec['corr'] else None, z if rec['pred'] else None))
        assert len(inter) == n
    t06 = unipc.build_plan(b, steps=5, t_start=0.6, t_end=0.01)
    assert float(t06['outer'][0]) == 0.6 and float(t06['outer'][-1]) == 0.01 and t06['outer'].dtype == F64


def test_plan_from_key_builds_the_plan_of_the_keywords():
    """plan_key -> plan_from_key gives build_plan's program and model times for every configuration of this file: the
    key's order and the keyword names agree."""
    b = betas64()
    for kw in [{}] + KEYED + BUILT:
        got, want = unipc.plan_from_key(b, unipc.plan_key(**kw)), unipc.build_plan(b, **kw)
        assert unipc.program(got) == unipc.program(want), kw
        assert unipc.plan_t_inputs(got) == unipc.plan_t_inputs(want), kw


@pytest.mark.parametrize('nfe', [20, 40])
def test_trajectory_error_is_below_the_multistep_solvers(nfe):
    """logSNR grid from t = 1 to 1 / T on the toy: UniPC (order 3, bh2, corrector) ends closer to the exact solution than
    dpm's own third-order multistep plan with as many evaluations."""
    ns = sched()
    x_T = torch.linspace(-2., 2., 9, dtype=F64)
    model = lambda xe, t: toy_m(ns, xe, t)
    plan = unipc.build_plan(betas64(), steps=nfe, order=3, variant='bh2', skip_type='logSNR')
    xu, _ = _run_unipc(ns, unipc.program(plan), x_T, model)
    dplan = dpm.build_plan(betas64().float(), steps=nfe, order=3, method='multistep', skip_type='logSNR')

    def dtail(xe, e, upd, base, h1, h2):
        m0 = model(xe, e['t'])
        return m0, dpm.update_expr(upd, base, m0, h1, h2)
    xd, _ = dpm.run_program(dpm.program(dplan), x_T, dtail)
    exact = torch.stack([torch.as_tensor(toy_exact(ns, float(v), 1.0, 1. / 1000), dtype=F64) for v in x_T])
    eu, ed = float((xu - exact).abs().max()), float((xd - exact).abs().max())
    print(f'{nfe} evaluations: UniPC-3 bh2 error {eu:.3e}, multistep-3 error {ed:.3e}, ratio {ed / eu:.2f}')
    assert eu < ed


def test_refused_options_raise_value_error_naming_the_argument():
    b = betas64()
    for kw, name in ((dict(order=4), 'order'), (dict(order=0), 'order'), (dict(variant='vary_coeff'), 'variant'),
                     (dict(variant='bh3'), 'variant'), (dict(skip_type='cosine'), 'skip_type'),
                     (dict(steps=2, order=3), 'steps')):
        with pytest.raises(ValueError, match=name):
            unipc.build_plan(b, **kw)
    for kw, name in ((dict(method='singlestep'), 'method'), (dict(solver_type='taylor'), 'solver_type'),
                     (dict(algorithm_type='dpmsolver'), 'algorithm_type'),
                     (dict(correcting_x0_fn='dynamic_thresholding'), 'correcting_x0_fn'),
                     (dict(guidance_scale=2.0), 'guidance_scale'), (dict(steps=1, order=2), 'steps')):
        with pytest.raises(ValueError, match=name):
            unipc.check_options(**kw)
    unipc.check_options()
    sig = inspect.signature(unipc.build_plan)
    assert list(sig.parameters) == ['betas', 'steps', 'order', 'variant', 'skip_type', 't_start', 't_end',
                                    'lower_order_final', 'corrector', 'denoise_to_zero']
    assert [p.default for p in list(sig.parameters.values())[1:]] == [20, 3, 'bh2', 'time_uniform', None, None, True,
                                                                      True, False]


def test_generate_imgs_refuses_before_touching_the_gpu():
    """The model surface forwards the refusals (no device needed: the check precedes every launch), and use_unipc takes
    precedence over use_dpm, which stays on by default."""
    from slotdiffusion_amd.models import LDM
    sig = inspect.signature(LDM.generate_imgs).parameters
    want = dict(use_unipc=False, unipc_steps=None, unipc_order=3, unipc_variant='bh2', unipc_skip_type='time_uniform',
                unipc_t_start=None, unipc_t_end=None, unipc_lower_order_final=True, unipc_corrector=True,
                unipc_denoise_to_zero=False, use_dpm=True)
    assert {k: sig[k].default for k in want} == want
    dm = LDM.__new__(LDM)
    object.__setattr__(dm, '_root_ref', None)
    cond = torch.zeros(1, 7, 192)
    for kw, name in ((dict(unipc_variant='vary_coeff'), 'variant'), (dict(unipc_order=4), 'order'),
                     (dict(unipc_skip_type='cosine'), 'skip_type'), (dict(unipc_steps=2), 'steps'),
                     (dict(unipc_method='singlestep'), 'method'), (dict(unipc_solver_type='taylor'), 'solver_type'),
                     (dict(unipc_algorithm_type='dpmsolver'), 'algorithm_type'),
                     (dict(unipc_correcting_x0_fn='dynamic_thresholding'), 'correcting_x0_fn'),
                     (dict(guidance_scale=3.), 'guidance_scale')):
        with pytest.raises(ValueError, match=name):
            LDM.generate_imgs(dm, cond, batch_size=1, use_unipc=True, **kw)
    with pytest.raises(ValueError, match='variant'):                 # ... over a DPM configuration given alongside
        LDM.generate_imgs(dm, cond, batch_size=1, use_unipc=True, dpm_method='multistep', unipc_variant='vary_coeff')


def test_cache_keys_are_distinct_across_unipc_and_dpm_configurations():
    from slotdiffusion_amd.models import SADiffusion
    ukey, dkey = SADiffusion.unipc_cache_key, SADiffusion.dpm_cache_key
    shape = (64, 7, 192)
    base = ukey(64, shape)
    assert base == ukey(64, shape, steps=20, order=3, variant='bh2', corrector=True)
    ukeys = [base] + [ukey(64, shape, **kw) for kw in KEYED] + [ukey(32, (32, 7, 192)), ukey(64, (64, 11, 192))]
    dkeys = [dkey(64, shape), dkey(64, shape, method='multistep'), dkey(64, shape, method='multistep', steps=10),
             dkey(64, shape, method='multistep', skip_type='logSNR'), dkey(64, shape, denoise_to_zero=True)]
    assert len(set(ukeys + dkeys)) == len(ukeys) + len(dkeys)
    # not by luck of the values: no UniPC plan key can equal a DPM plan key
    assert unipc.plan_key()[0] == 'unipc' and isinstance(dpm.plan_key()[0], int)
    assert unipc.plan_key(t_start=0.6) == unipc.plan_key(t_start=torch.tensor(0.6, dtype=F64).item())
    hash(base)


def test_unipc_step_rejects_bad_arguments_without_launch():
    """Fake (non-null, non-overlapping) addresses: every refusal comes from the argument checks, before any launch."""
    R = 64
    a = lambda i: 0x10000 * i                                        # 64 KiB apart: R * 16 bytes never overlap
    ok = dict(x=a(1), out=a(2), codebook=a(3), m0=a(4), base=a(5), h1=a(6), h2=a(7), h3=a(8), xc=a(9), y=a(10),
              idx=a(11), R=R, n_codes=4096, target=0, scale=1., sigma=0.5, alpha=0.8, corr_order=3, pred_order=3)
    bad = [dict(x=0), dict(out=0), dict(codebook=0), dict(m0=0), dict(base=0), dict(xc=0), dict(y=0),      # null pointers
           dict(h1=0), dict(h2=0), dict(h3=0), dict(h2=0, corr_order=1), dict(h1=0, corr_order=0, pred_order=2),
           dict(corr_order=4), dict(corr_order=-1), dict(pred_order=4), dict(pred_order=-1),               # orders
           dict(n_codes=8193), dict(n_codes=0), dict(R=0), dict(target=3), dict(alpha=0.), dict(scale=0.),
           dict(m0=a(1)), dict(xc=a(5)), dict(y=a(6)), dict(y=a(2)), dict(m0=a(8) + 16), dict(xc=a(3)),    # aliases
           dict(y=a(9)), dict(m0=a(10)), dict(idx=a(1)), dict(idx=a(4) + 8)]
    for over in bad:
        with pytest.raises(_lib.SdmiError, match='sdmi_unipc_step') as err:
            _lib.call('sdmi_unipc_step', None, **dict(ok, **over))
        assert 'launch failed' not in str(err.value), over             # refused by a check, not by the runtime
        assert len(_lib.lib().sdmi_last_error()) > 0, over
