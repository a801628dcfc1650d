"""Host side of the DPM-Solver++ family (slotdiffusion_amd/dpm.py) against tests/golden/dpm_family_b2.npz, the
reference's DPM_Solver run by tools/gen_golden.py (`dpm_family`): time grids, model times, and -- through a small
pure-torch executor of the SAME flat program the device loop runs -- the toy trajectories.  No GPU."""
import inspect
import json
import os

import pytest
import torch

from slotdiffusion_amd import dpm, module
from tests import common as C

# the five configurations of the fixture (method, order, steps, other), as DPM_Solver.sample keywords
CONFIGS = [
    ('ms2_10', dict(method='multistep', order=2, steps=10)),
    ('ms3_15_logsnr', dict(method='multistep', order=3, steps=15, skip_type='logSNR')),
    ('ms3_8_lof', dict(method='multistep', order=3, steps=8)),
    ('ss2_10_quad_d0', dict(method='singlestep', order=2, steps=10, skip_type='time_quadratic', denoise_to_zero=True)),
    ('ss3_12_t06', dict(method='singlestep', order=3, steps=12, t_start=0.6)),
]
BAR = 1e-4                # the project's fp32 bar on solver states
# (configuration, number of intermediates) and the configurations whose cache keys must differ from the default's
COUNTS = ((dict(method='multistep', order=2, steps=10), 11),
          (dict(method='singlestep', order=3, steps=20), 7),
          (dict(method='singlestep_fixed', order=2, steps=10, denoise_to_zero=True), 6),
          (dict(method='multistep', order=3, steps=8, denoise_to_zero=True), 10))
KEYED = [dict(steps=10), dict(order=2), dict(method='multistep'), dict(method='singlestep_fixed'),
         dict(skip_type='logSNR'), dict(skip_type='time_quadratic'), dict(t_start=0.6), dict(t_end=1e-4),
         dict(denoise_to_zero=True), dict(method='multistep', lower_order_final=False)]


def betas():
    return torch.tensor(module.ddpm_schedule(1000, 'linear', 0.0015, 0.0195)['betas'], dtype=torch.float32)


def family():
    G = C.load_golden('dpm_family_b2.npz')
    assert [[t, k] for t, k in CONFIGS] == json.loads(str(G['configs']))
    return G


def toy_eps(G, x, t_input):
    """The fixture's toy noise model (tools/gen_golden.py: toy_eps): A * x + C + D * (t_input / 1000), elementwise."""
    return G['toy_A'] * x + G['toy_C'] + G['toy_D'] * (t_input.reshape(-1, 1, 1, 1) / 1000.)


def toy_quantize(G, x0):
    step, clamp = float(G['toy_grid'][0]), float(G['toy_grid'][1])
    return torch.clamp(torch.round(x0 / step) * step, -clamp, clamp)


def test_default_plan_is_the_parents_plan():
    """build_plan(betas, 20, 3) key for key, float for float what it returned before the family was added (recorded
    from that code in tests/golden/dpm_plan_default.json; json floats round-trip exactly)."""
    want = json.load(open(os.path.join(C.GOLD, 'dpm_plan_default.json')))
    for plan in (dpm.build_plan(betas(), 20, 3), dpm.build_plan(betas())):
        assert set(plan) == {'steps', 'outer', 'orders'}
        assert plan['steps'] == want['steps'] and plan['orders'] == want['orders']
        assert [float(v) for v in plan['outer']] == want['outer'] and plan['outer'].dtype == torch.float32
    sig = inspect.signature(dpm.build_plan)
    assert list(sig.parameters) == ['betas', 'steps', 'order', 'method', 'skip_type', 't_start', 't_end',
                                    'lower_order_final', 'denoise_to_zero']
    assert [p.default for p in list(sig.parameters.values())[1:]] == [20, 3, 'singlestep', 'time_uniform', None, None,
                                                                      True, False]


@pytest.mark.parametrize('tag,kw', CONFIGS, ids=[t for t, _ in CONFIGS])
def test_time_grid_and_model_times_equal_the_reference(tag, kw):
    """All three grids and t_start: the grid the reference's sampler walks and the model time of EVERY evaluation it made
    (recorded inside its model function), exactly."""
    G = family()
    plan = dpm.build_plan(betas(), **kw)
    assert torch.equal(plan['outer'], G[tag + '/grid'])
    if kw['method'] != 'multistep':
        assert plan['orders'] == G[tag + '/orders'].tolist()
    tin = torch.tensor(dpm.plan_t_inputs(plan), dtype=torch.float32)
    assert torch.equal(tin, G[tag + '/t_input'])
    assert len(tin) == kw['steps'] + int(kw.get('denoise_to_zero', False))
    if 't_start' in kw:
        assert float(plan['outer'][0]) == float(torch.tensor(kw['t_start']))


def test_multistep_orders_follow_sample():
    assert dpm.multistep_orders(10, 2) == [1] + [2] * 9
    assert dpm.multistep_orders(8, 3) == [1, 2, 3, 3, 3, 3, 2, 1]                # lower_order_final, steps < 10
    assert dpm.multistep_orders(8, 3, lower_order_final=False) == [1, 2] + [3] * 6
    assert dpm.multistep_orders(15, 3) == [1, 2] + [3] * 13                       # not taken from 10 steps on


@pytest.mark.parametrize('tag,kw', CONFIGS, ids=[t for t, _ in CONFIGS])
def test_program_reproduces_the_reference_toy_trajectory(tag, kw):
    """dpm.program(plan) -- the records the device loop consumes -- run by dpm.run_program with torch expressions in
    place of the launches: every intermediate state and the final one within 1e-4 of the reference's.
    Measured maxima: 0 in all five configurations."""
    G = family()
    plan = dpm.build_plan(betas(), **kw)
    prog = dpm.program(plan)

    def tail(x, e, upd, base, h1, h2):
        eps = toy_eps(G, x, torch.tensor([e['t_input']], dtype=torch.float32))
        m0 = toy_quantize(G, (x - e['sigma'] * eps) / e['alpha'])
        return m0, (dpm.update_expr(upd, base, m0, h1, h2) if upd is not None else None)

    x, inter = dpm.run_program(prog, G[tag + '/toy_x_T'], tail, emit_initial=kw['method'] == 'multistep')
    want = G[tag + '/toy_inter']
    assert len(inter) == want.shape[0]
    errs = [float((a - b).abs().max()) for a, b in zip(inter, want)]
    final = float((x - G[tag + '/toy_final']).abs().max())
    print(tag, 'toy trajectory max-abs error per state', errs, 'final', final)
    assert float(want.abs().max()) < 10.                       # the toy keeps the reference's states O(1)
    assert max(errs) <= BAR and final <= BAR


def test_intermediates_count_per_method():
    b = betas()
    for kw, n in COUNTS:
        prog = dpm.program(dpm.build_plan(b, **kw))
        z = torch.zeros(1)
        _, inter = dpm.run_program(prog, z, lambda x, e, u, base, h1, h2: (z, z if u is not None else None),
                                   emit_initial=kw['method'] == 'multistep')
        assert len(inter) == n, (kw, len(inter))
        assert len(prog) == kw['steps'] + int(kw.get('denoise_to_zero', False))


def test_plan_from_key_builds_the_plan_of_the_keywords():
    """plan_key -> plan_from_key gives build_plan's program and model times for every configuration of this file: the
    key's order and the keyword names agree."""
    b = betas()
    for kw in [{}] + [kw for _, kw in CONFIGS] + [kw for kw, _ in COUNTS] + KEYED:
        got, want = dpm.plan_from_key(b, dpm.plan_key(**kw)), dpm.build_plan(b, **kw)
        assert dpm.program(got) == dpm.program(want), kw
        assert dpm.plan_t_inputs(got) == dpm.plan_t_inputs(want), kw
        assert got.get('method') == want.get('method'), kw


def test_refused_options_raise_value_error_naming_the_argument():
    b = betas()
    with pytest.raises(ValueError, match='method'):
        dpm.build_plan(b, method='adaptive')
    with pytest.raises(ValueError, match='order'):
        dpm.build_plan(b, order=4)
    with pytest.raises(ValueError, match='skip_type'):
        dpm.build_plan(b, skip_type='cosine')
    with pytest.raises(ValueError, match='solver_type'):
        dpm.check_options(solver_type='taylor')
    with pytest.raises(ValueError, match='algorithm_type'):
        dpm.check_options(algorithm_type='dpmsolver')
    with pytest.raises(ValueError, match='correcting_x0_fn'):
        dpm.check_options(correcting_x0_fn='dynamic_thresholding')
    with pytest.raises(ValueError, match='guidance_scale'):
        dpm.check_options(guidance_scale=2.0)
    with pytest.raises(ValueError, match='steps'):
        dpm.build_plan(b, method='multistep', order=3, steps=2)
    dpm.check_options()


def test_generate_imgs_refuses_before_touching_the_gpu():
    """The model surface forwards the refusals (no device needed: the check precedes every launch)."""
    from slotdiffusion_amd.models import LDM
    sig = inspect.signature(LDM.generate_imgs).parameters
    want = dict(dpm_steps=None, dpm_order=3, dpm_method='singlestep', dpm_skip_type='time_uniform', dpm_t_start=None,
                dpm_t_end=None, dpm_denoise_to_zero=False, dpm_lower_order_final=True)
    assert {k: sig[k].default for k in want} == want
    assert hasattr(LDM, 'noise_latent')
    dm = LDM.__new__(LDM)
    object.__setattr__(dm, '_root_ref', None)
    cond = torch.zeros(1, 7, 192)
    for kw, name in ((dict(dpm_method='adaptive'), 'method'), (dict(dpm_solver_type='taylor'), 'solver_type'),
                     (dict(dpm_algorithm_type='dpmsolver'), 'algorithm_type'),
                     (dict(dpm_correcting_x0_fn='dynamic_thresholding'), 'correcting_x0_fn'),
                     (dict(guidance_scale=3.), 'guidance_scale')):
        with pytest.raises(ValueError, match=name):
            LDM.generate_imgs(dm, cond, batch_size=1, **kw)


def test_distinct_configuration_distinct_cache_key():
    from slotdiffusion_amd.models import SADiffusion
    key = SADiffusion.dpm_cache_key
    base = key(64, (64, 7, 192))
    assert base == key(64, (64, 7, 192), steps=20, order=3, method='singlestep')
    keys = [key(64, (64, 7, 192), **kw) for kw in KEYED] + [key(32, (32, 7, 192)), key(64, (64, 11, 192))]
    assert len(set(keys + [base])) == len(keys) + 1
    assert dpm.plan_key(t_start=0.6) == dpm.plan_key(t_start=torch.tensor(0.6, dtype=torch.float64).item())
    hash(base)
