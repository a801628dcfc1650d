"""UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"):
multistep predictor-corrector updates in the data-prediction form, orders 1-3, variants bh1 / bh2, on the schedule and
the time grids of dpm.py.

One step goes from s = t_{i-1} to t = t_i with order o, from the carried state x at s and the stored (quantised)
predictions m_{i-1} .. m_{i-o}:

    h = lambda(t) - lambda(s);  hh = -h
    r_k = (lambda(t_{i-1-k}) - lambda(s)) / h            k = 1 .. o-1;  r_o = 1
    D_k = (m_{i-1-k} - m_{i-1}) / r_k                    k = 1 .. o-1
    h_phi_1 = expm1(hh);  B = hh ('bh1') | expm1(hh) ('bh2')
    R[j][k] = r_k^(j-1),  b[j] = hh * phi_{j+1}(hh) * j! / B          j, k = 1 .. o
    x_  = std(t) / std(s) * x - alpha(t) * h_phi_1 * m_{i-1}
    predictor  rho_p = [] (o = 1) | [0.5] (o = 2) | solve(R[:o-1,:o-1], b[:o-1]) (o = 3)
               x_p = x_ - alpha(t) * B * sum_k rho_p[k] * D_k
    evaluate the network at (x_p, t) -> m_i             (m_i stays in the history as it is)
    corrector  rho_c = [0.5] (o = 1) | solve(R, b)
               x_c = x_ - alpha(t) * B * (sum_{k<o} rho_c[k] * D_k + rho_c[o] * (m_i - m_{i-1}))

The corrector of step i needs m_i, which the predictor of step i + 1 needs anyway: it costs no evaluation.  It runs on
every step but the last, so a pass makes exactly `steps` evaluations, at t_0 .. t_{steps-1}.

Every coefficient is computed on the host in float64 (dpm.DiscreteSchedule with dtype float64) and folded so that the
device sees plain weights of differences of predictions:

    q_k = -alpha(t) * B * rho_p[k] / r_k,   w_k = -alpha(t) * B * rho_c[k] / r_k,   wn = -alpha(t) * B * rho_c[o]
    x_p = ((c0 * x + c1 * m_{i-1}) + q_1 * (m_{i-2} - m_{i-1})) + q_2 * (m_{i-3} - m_{i-1})
    x_c = (((c0 * x + c1 * m_{i-1}) + w_1 * (m_{i-2} - m_{i-1})) + w_2 * (m_{i-3} - m_{i-1})) + wn * (m_i - m_{i-1})

The device loop makes one sdmi_unipc_step launch per evaluation (include/sdmi.h): the data prediction and the VQ snap of
the evaluated state, the corrector of the step just taken and the predictor of the next one.
"""
import math

import torch

from . import dpm

VARIANTS = ('bh1', 'bh2')


def check_options(order=3, variant='bh2', skip_type='time_uniform', steps=None, method='multistep',
                  solver_type='dpmsolver', algorithm_type='dpmsolver++', correcting_x0_fn=None, guidance_scale=1.,
                  vq_denoised=True, dynamic_thresholding_ratio=0.995, thresholding_max_val=1.0):
    """ValueError naming the argument for everything this sampler does not build.  What dpm.check_options refuses
    (taylor, the noise-prediction form, dynamic thresholding on a latent decoder, guidance, orders outside 1..3, unknown grids) is refused
    by it; on top of that only the multistep form and the variants bh1 / bh2 exist, and steps >= order."""
    if method != 'multistep':
        raise ValueError(f"method={method!r}: only multistep UniPC is built")
    dpm.check_options(method='multistep', order=order, skip_type=skip_type, solver_type=solver_type,
                      algorithm_type=algorithm_type, correcting_x0_fn=correcting_x0_fn, guidance_scale=guidance_scale,
                      vq_denoised=vq_denoised, dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                      thresholding_max_val=thresholding_max_val)
    if variant not in VARIANTS:
        raise ValueError(f"variant={variant!r}: built are {VARIANTS} ('vary_coeff' is not)")
    if steps is not None and steps < order:
        raise ValueError(f'steps={steps!r}: UniPC needs steps >= order')


def step_orders(steps, order, lower_order_final=True):
    """Order of step 1..steps: min(order, i), with lower_order_final also capped at steps + 1 - i."""
    return [min(order, i, steps + 1 - i) if lower_order_final else min(order, i) for i in range(1, steps + 1)]


def step_record(ns, t_hist, t, order, variant, corrector=True):
    """Float64 coefficients of the step from s = t_hist[0] to t with the predictions at t_hist[0 .. order-1]:
    dict(order, c0, c1, q=[q_1 .. q_{o-1}], w=[w_1 .. w_{o-1}] or None, wn or None) in the folded form of the module
    docstring (w, wn None without corrector)."""
    f64 = lambda v: torch.as_tensor(v, dtype=torch.float64).reshape(1)
    lam = lambda v: float(ns.lam(f64(v).to(ns.dtype)))
    s = t_hist[0]
    lam_s = lam(s)
    h = lam(t) - lam_s
    hh = -h
    rks = [(lam(t_hist[k]) - lam_s) / h for k in range(1, order)] + [1.0]
    h_phi_1 = math.expm1(hh)
    B = hh if variant == 'bh1' else math.expm1(hh)
    b = []
    g, f = h_phi_1 / hh - 1., 1.
    for j in range(1, order + 1):
        b.append(g * f / B)
        f *= j + 1
        g = g / hh - 1. / f
    R = torch.tensor([[rk ** j for rk in rks] for j in range(order)], dtype=torch.float64)
    bt = torch.tensor(b, dtype=torch.float64)
    alpha_t = float(ns.alpha(f64(t).to(ns.dtype)))
    c0 = float(ns.std(f64(t).to(ns.dtype))) / float(ns.std(f64(s).to(ns.dtype)))
    if order == 1:
        rho_p = []
    elif order == 2:
        rho_p = [0.5]
    else:
        rho_p = torch.linalg.solve(R[:-1, :-1], bt[:-1]).tolist()
    rec = dict(order=order, c0=c0, c1=-alpha_t * h_phi_1, q=[-alpha_t * B * rho_p[k] / rks[k] for k in range(order - 1)],
               w=None, wn=None)
    if corrector:
        rho_c = [0.5] if order == 1 else torch.linalg.solve(R, bt).tolist()
        rec['w'] = [-alpha_t * B * rho_c[k] / rks[k] for k in range(order - 1)]
        rec['wn'] = -alpha_t * B * rho_c[-1]
    return rec


def build_plan(betas, steps=20, order=3, variant='bh2', skip_type='time_uniform', t_start=None, t_end=None,
               lower_order_final=True, corrector=True, denoise_to_zero=False):
    """-> dict(steps=[step_record ...], evals=[dict(t, t_input, sigma, alpha) ...], outer (the time grid, float64),
    orders, denoise (the evaluation record at t_end, only when asked))."""
    check_options(order=order, variant=variant, skip_type=skip_type, steps=steps)
    ns = dpm.DiscreteSchedule(torch.as_tensor(betas).double(), dtype=torch.float64)
    t_0 = 1.0 / ns.N if t_end is None else float(t_end)
    t_T = ns.T if t_start is None else float(t_start)
    if not (t_0 > 0 and t_T > 0):
        raise ValueError(f't_start={t_start!r}, t_end={t_end!r}: times must lie in [1 / N, 1]')
    ts = [float(v) for v in dpm.time_steps(ns, skip_type, t_T, t_0, steps)]

    def ev(t):
        tt = torch.tensor([t], dtype=torch.float64)
        return dict(t=t, t_input=(t - 1. / ns.N) * 1000., sigma=float(ns.std(tt)), alpha=float(ns.alpha(tt)))

    orders = step_orders(steps, order, lower_order_final)
    recs = [step_record(ns, ts[i - 1::-1], ts[i], od, variant, corrector and i < steps)
            for i, od in zip(range(1, steps + 1), orders)]
    plan = dict(steps=recs, evals=[ev(t) for t in ts[:-1]], outer=torch.tensor(ts, dtype=torch.float64), orders=orders)
    if denoise_to_zero:
        plan['denoise'] = ev(ts[-1])
    return plan


def program(plan):
    """The plan as one record per function evaluation n = 0 .. steps-1 (at t_n), as the device loop runs them:
      e    : the evaluation record (t_input, sigma, alpha)
      corr : None, or the corrector of step n, the step just taken: dict(order, c0, c1, w1, w2, wn)
      pred : None, or the predictor of step n + 1: dict(order, c0, c1, q1, q2)
    The `denoise` record comes last with neither: its prediction is the result."""
    prog = []
    for n, e in enumerate(plan['evals']):
        corr = None
        if n >= 1 and plan['steps'][n - 1]['wn'] is not None:
            st = plan['steps'][n - 1]
            w = st['w'] + [0., 0.]
            corr = dict(order=st['order'], c0=st['c0'], c1=st['c1'], w1=w[0], w2=w[1], wn=st['wn'])
        st = plan['steps'][n]
        q = st['q'] + [0., 0.]
        prog.append(dict(e=e, corr=corr, pred=dict(order=st['order'], c0=st['c0'], c1=st['c1'], q1=q[0], q2=q[1])))
    if 'denoise' in plan:
        prog.append(dict(e=plan['denoise'], corr=None, pred=None))
    return prog


def update_expr(rec, base, m0, h1, h2, h3):
    """The tail's two updates as tensor expressions, op by op in sdmi_unipc_step's order (any torch dtype).  m0 is the
    prediction just made, h1 / h2 / h3 the one, two and three evaluations back; base is the carried state at the
    previous time when rec has a corrector, else the carried state at this time.  -> (x_c or None, x_p_next or None)."""
    xc = None
    c = rec['corr']
    if c is not None:
        xc = c['c0'] * base + c['c1'] * h1
        if c['order'] >= 2:
            xc = xc + c['w1'] * (h2 - h1)
        if c['order'] == 3:
            xc = xc + c['w2'] * (h3 - h1)
        xc = xc + c['wn'] * (m0 - h1)
    y = None
    p = rec['pred']
    if p is not None:
        y = p['c0'] * (base if xc is None else xc) + p['c1'] * m0
        if p['order'] >= 2:
            y = y + p['q1'] * (h1 - m0)
        if p['order'] == 3:
            y = y + p['q2'] * (h2 - m0)
    return xc, y


def run_program(prog, x, tail):
    """Drive `prog` (program()) from state x.  tail(x, rec, base, h1, h2, h3) -> (m0, xc, y) is one function evaluation
    with its tail: the quantised data prediction m0 of the evaluated state x, the corrected state xc of the step just
    taken (None without corrector) and the predicted state y at the next time (None for the denoise record).
    -> (final state, [initial state, the carried state after every step, the denoise_to_zero state when asked]).
    The CPU tests pass torch expressions, the model one HIP launch: one control flow for both."""
    ms = [None, None, None]
    inter = [x]
    carried = x
    y = x
    for n, rec in enumerate(prog):
        x = y
        base = carried if rec['corr'] is not None else x
        m0, xc, y = tail(x, rec, base, ms[-1], ms[-2], ms[-3])
        ms.append(m0)
        carried = x if xc is None else xc
        if n >= 1:
            inter.append(carried)                       # the state after step n
    if prog[-1]['pred'] is None:                        # denoise_to_zero: the state BECOMES the prediction
        y = ms[-1]
    inter.append(y)
    return y, inter


def plan_key(steps=20, order=3, variant='bh2', skip_type='time_uniform', t_start=None, t_end=None,
             lower_order_final=True, corrector=True, denoise_to_zero=False):
    """Hashable identity of a UniPC configuration; the leading tag keeps it apart from every dpm.plan_key."""
    return ('unipc', int(steps), int(order), str(variant), str(skip_type),
            None if t_start is None else float(t_start), None if t_end is None else float(t_end),
            bool(lower_order_final), bool(corrector), bool(denoise_to_zero))


def plan_from_key(betas, key):
    """build_plan of the configuration a plan_key names (the key's order is spelled here and in plan_key alone)."""
    tag, steps, order, variant, skip_type, t_start, t_end, lower_order_final, corrector, denoise_to_zero = key
    assert tag == 'unipc'
    return build_plan(betas, steps=steps, order=order, variant=variant, skip_type=skip_type, t_start=t_start,
                      t_end=t_end, lower_order_final=lower_order_final, corrector=corrector,
                      denoise_to_zero=denoise_to_zero)


def plan_t_inputs(plan):
    return [e['t_input'] for e in plan['evals']] + ([plan['denoise']['t_input']] if 'denoise' in plan else [])
