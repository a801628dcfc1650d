"""DPM-Solver++ (singlestep / singlestep_fixed / multistep, orders 1-3, three time grids) for the discrete LDM schedule.

Reference: video_based/models/ddpm/dpm_solver.py -- NoiseScheduleVP('discrete') 160-235,
model_wrapper 238-416, DPM_Solver.sample singlestep branch 1310-1328 with the dpmsolver++
second/third updates 716-732 / 804-831, as driven by CondDDPM.generate_imgs
(cond_ddpm.py:155-193: steps=20, order=3, method='singlestep', vq_denoised=True).

MI355X-side design: every scalar the solver needs (alpha, sigma, lambda, expm1 coefficients,
intermediate times) depends only on the beta table, so the whole 20-NFE plan is computed ONCE on
the host -- with fp32 torch CPU tensor ops, i.e. the same arithmetic the reference performs on its
schedule tensors -- and the device loop is a fixed sequence of kernels with no host<->device
synchronisation (the reference calls `.item()` per outer step, dpm_solver.py:1319).  The device
updates are single fused `sdmi_lincomb` launches that round like the reference's op-by-op tensor
expressions.
"""
import torch


class DiscreteSchedule:
    """log(alpha_t) table on t_i = (i+1)/N with piecewise-linear interpolation (fp32; unipc.py asks for float64)."""

    def __init__(self, betas, dtype=torch.float32):
        betas = torch.as_tensor(betas, dtype=dtype).cpu()
        self.dtype = dtype
        self.log_alpha = (0.5 * torch.log(1 - betas).cumsum(dim=0)).to(dtype)
        self.N = int(self.log_alpha.numel())
        self.t_array = torch.linspace(0., 1., self.N + 1, dtype=dtype)[1:]
        self.T = 1.0

    @staticmethod
    def _interp(x, xp, yp):
        # keypoint segment containing x (outermost segments extrapolate), then the two-point form
        K = xp.numel()
        idx = torch.searchsorted(xp, x.contiguous(), right=False)
        lo = torch.where(idx == 0, torch.zeros_like(idx),
                         torch.where(idx == K, torch.full_like(idx, K - 2), idx - 1))
        xa, xb, ya, yb = xp[lo], xp[lo + 1], yp[lo], yp[lo + 1]
        return ya + (x - xa) * (yb - ya) / (xb - xa)

    def log_mean_coeff(self, t):
        return self._interp(t.reshape(-1), self.t_array, self.log_alpha)

    def alpha(self, t):
        return torch.exp(self.log_mean_coeff(t))

    def std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self.log_mean_coeff(t)))

    def lam(self, t):
        lm = self.log_mean_coeff(t)
        return lm - 0.5 * torch.log(1. - torch.exp(2. * lm))

    def inverse_lambda(self, lamb):
        la = -0.5 * torch.logaddexp(torch.zeros((1,), dtype=self.dtype), -2. * lamb)
        return self._interp(la.reshape(-1), torch.flip(self.log_alpha, [0]),
                            torch.flip(self.t_array, [0]))


def singlestep_orders(steps, order):
    """How `steps` function evaluations are split over solver orders (dpm_solver.py:597-616)."""
    if order == 3:
        K = steps // 3 + 1
        if steps % 3 == 0:
            return [3] * (K - 2) + [2, 1]
        if steps % 3 == 1:
            return [3] * (K - 1) + [1]
        return [3] * (K - 1) + [2]
    if order == 2:
        return [2] * (steps // 2) + ([1] if steps % 2 else [])
    return [1] * steps


METHODS = ('singlestep', 'singlestep_fixed', 'multistep')
SKIP_TYPES = ('time_uniform', 'logSNR', 'time_quadratic')
# options of the reference's sampler that are not built: asking for one raises a ValueError naming it
REFUSED = dict(method=('adaptive',), solver_type=('taylor',), algorithm_type=('dpmsolver',))

# update forms of one function evaluation's tail (include/sdmi.h: SDMI_DPM_UPD_*)
UPD_NONE, UPD_FIRST, UPD_SINGLE, UPD_MULTI2, UPD_MULTI3 = 0, 1, 2, 3, 4


def check_options(method='singlestep', order=3, skip_type='time_uniform', solver_type='dpmsolver',
                  algorithm_type='dpmsolver++', correcting_x0_fn=None, guidance_scale=1., vq_denoised=True,
                  dynamic_thresholding_ratio=0.995, thresholding_max_val=1.0):
    """ValueError for everything of DPM_Solver.sample / model_wrapper this sampler does not build.  correcting_x0_fn
    (dynamic thresholding) belongs to the image-space decoder: with vq_denoised (the latent decoder, the default) it is
    refused, as the reference refuses the pair (dpm_solver.py:503-504)."""
    if method not in METHODS:
        raise ValueError(f"method={method!r}: built are {METHODS} ('adaptive' needs a host decision per step)")
    if solver_type != 'dpmsolver':
        raise ValueError(f"solver_type={solver_type!r}: only 'dpmsolver' is built")
    if algorithm_type != 'dpmsolver++':
        raise ValueError(f"algorithm_type={algorithm_type!r}: only 'dpmsolver++' (data prediction) is built")
    if correcting_x0_fn and vq_denoised:
        raise ValueError(f'correcting_x0_fn={correcting_x0_fn!r}: dynamic thresholding is for the image-space decoder; '
                         'the latent decoder quantises its prediction instead (vq_denoised)')
    if correcting_x0_fn not in (None, False, True, 'dynamic_thresholding'):
        raise ValueError(f"correcting_x0_fn={correcting_x0_fn!r}: only 'dynamic_thresholding' is built")
    if not 0. < float(dynamic_thresholding_ratio) <= 1.:
        raise ValueError(f'dynamic_thresholding_ratio={dynamic_thresholding_ratio!r}: must be in (0, 1]')
    if not float(thresholding_max_val) > 0.:
        raise ValueError(f'thresholding_max_val={thresholding_max_val!r}: must be positive')
    if guidance_scale != 1.:
        raise ValueError(f'guidance_scale={guidance_scale!r}: only 1 (no classifier-free guidance) is built')
    if order not in (1, 2, 3):
        raise ValueError(f'order={order!r}: must be 1, 2 or 3')
    if skip_type not in SKIP_TYPES:
        raise ValueError(f'skip_type={skip_type!r}: must be one of {SKIP_TYPES}')


def time_steps(ns, skip_type, t_T, t_0, N):
    """get_time_steps (dpm_solver.py:545-572): N + 1 times from t_T down to t_0."""
    dt = ns.dtype
    if skip_type == 'logSNR':
        lam_T, lam_0 = ns.lam(torch.tensor(t_T, dtype=dt)), ns.lam(torch.tensor(t_0, dtype=dt))
        return ns.inverse_lambda(torch.linspace(lam_T.item(), lam_0.item(), N + 1, dtype=dt))
    if skip_type == 'time_uniform':
        return torch.linspace(t_T, t_0, N + 1, dtype=dt)
    if skip_type == 'time_quadratic':
        return torch.linspace(t_T ** (1. / 2), t_0 ** (1. / 2), N + 1, dtype=dt).pow(2)
    raise ValueError(f'skip_type={skip_type!r}: must be one of {SKIP_TYPES}')


def build_plan(betas, steps=20, order=3, method='singlestep', skip_type='time_uniform',
               t_start=None, t_end=None, lower_order_final=True, denoise_to_zero=False):
    """-> dict(steps=[...], outer, orders): host-side plan driving the device loop.

    Singlestep methods: each outer step has `order` evaluations; every evaluation record carries
      t_input : model time (t - 1/N) * 1000                (model_wrapper, 345-346)
      sigma, alpha : x0 = (x - sigma*eps) / alpha            (data_prediction_fn, 523-534)
    plus the lincomb coefficients (to_s1, to_s2, final) of the exponential-integrator updates.
    Multistep (sample() 1267-1309; plan['method'] == 'multistep'): every step has ONE evaluation, at the
    step's start time, and `final` holds the coefficients of the first / second / third order multistep
    update (639-672, 888-944, 946-996) from the predictions of this and the previous one or two steps.
    denoise_to_zero adds plan['denoise'], one more evaluation record at t_0 (633-637).  The default
    arguments return exactly the three keys above; `method` and `denoise` appear only when asked for.
    """
    check_options(method=method, order=order, skip_type=skip_type)
    ns = DiscreteSchedule(betas)
    t_0 = 1.0 / ns.N if t_end is None else t_end
    t_T = ns.T if t_start is None else t_start
    if not (t_0 > 0 and t_T > 0):
        raise ValueError(f't_start={t_start!r}, t_end={t_end!r}: times must lie in [1 / N, 1]')
    f = lambda v: float(v.reshape(-1)[0])

    def rec(tc):
        tc = tc.reshape(1)
        return dict(t=f(tc), t_input=f((tc - 1. / ns.N) * 1000.), sigma=f(ns.std(tc)),
                    alpha=f(ns.alpha(tc)))

    if method == 'multistep':
        plan = _multistep_plan(ns, steps, order, skip_type, t_T, t_0, lower_order_final, rec, f)
    else:
        plan = _singlestep_plan(ns, steps, order, method, skip_type, t_T, t_0, rec, f)
    if denoise_to_zero:
        plan['denoise'] = rec(torch.ones((1,)) * t_0)
    return plan


def _singlestep_plan(ns, steps, order, method, skip_type, t_T, t_0, rec, f):
    if method == 'singlestep':          # get_orders_and_timesteps_for_singlestep_solver, 574-631
        orders = singlestep_orders(steps, order)
        if skip_type == 'logSNR':
            if order == 1 and steps > 1:
                raise ValueError("skip_type='logSNR' with method='singlestep', order=1: the reference's grid has one "
                                 "interval for `steps` first-order steps; use method='singlestep_fixed'")
            outer = time_steps(ns, skip_type, t_T, t_0, len(orders))
        else:
            grid = time_steps(ns, skip_type, t_T, t_0, steps)
            outer = grid[torch.cumsum(torch.tensor([0] + orders), 0)]
    else:                               # 'singlestep_fixed', 1313-1316
        if steps < order:
            raise ValueError(f'steps={steps!r}: singlestep_fixed needs at least `order` evaluations')
        orders = [order] * (steps // order)
        outer = time_steps(ns, skip_type, t_T, t_0, len(orders))
    plan = []
    for i, od in enumerate(orders):
        s, t = outer[i], outer[i + 1]
        inner = time_steps(ns, skip_type, s.item(), t.item(), od)
        lam_in = ns.lam(inner)
        h_in = lam_in[-1] - lam_in[0]
        r1 = None if od <= 1 else (lam_in[1] - lam_in[0]) / h_in
        r2 = None if od <= 2 else (lam_in[2] - lam_in[0]) / h_in
        s1d, t1d = s.reshape(1), t.reshape(1)
        lam_s, lam_t = ns.lam(s1d), ns.lam(t1d)
        h = lam_t - lam_s
        sig_s, sig_t = ns.std(s1d), ns.std(t1d)
        alpha_t = torch.exp(ns.log_mean_coeff(t1d))
        phi_1 = torch.expm1(-h)

        step = dict(order=od, evals=[rec(s1d)])
        if od == 1:
            step['final'] = dict(c0=f(sig_t / sig_s), c1=f(-(alpha_t * phi_1)))
        else:
            if r1 is None:
                r1 = torch.tensor(0.5)
            s1 = ns.inverse_lambda(lam_s + r1 * h)
            sig_s1 = ns.std(s1)
            alpha_s1 = torch.exp(ns.log_mean_coeff(s1))
            phi_11 = torch.expm1(-r1 * h)
            step['evals'].append(rec(s1))
            step['to_s1'] = dict(c0=f(sig_s1 / sig_s), c1=f(-(alpha_s1 * phi_11)))
            if od == 2:
                step['final'] = dict(c0=f(sig_t / sig_s), c1=f(-(alpha_t * phi_1)),
                                     c2=f(-((0.5 / r1) * (alpha_t * phi_1))), which=1)
            else:
                s2 = ns.inverse_lambda(lam_s + r2 * h)
                sig_s2 = ns.std(s2)
                alpha_s2 = torch.exp(ns.log_mean_coeff(s2))
                phi_12 = torch.expm1(-r2 * h)
                phi_22 = torch.expm1(-r2 * h) / (r2 * h) + 1.
                phi_2 = phi_1 / h + 1.
                step['evals'].append(rec(s2))
                step['to_s2'] = dict(c0=f(sig_s2 / sig_s), c1=f(-(alpha_s2 * phi_12)),
                                     c2=f(r2 / r1 * (alpha_s2 * phi_22)))
                step['final'] = dict(c0=f(sig_t / sig_s), c1=f(-(alpha_t * phi_1)),
                                     c2=f((1. / r2) * (alpha_t * phi_2)), which=2)
        plan.append(step)
    return dict(steps=plan, outer=outer, orders=orders)


def multistep_orders(steps, order, lower_order_final=True):
    """Order of the update that ends step 1..steps (sample() 1281-1298): the warm-up climbs 1..order-1, and
    with lower_order_final the last steps fall back to lower orders -- only when steps < 10."""
    out = []
    for step in range(1, steps + 1):
        if step < order:
            out.append(step)
        elif lower_order_final and steps < 10:
            out.append(min(order, steps + 1 - step))
        else:
            out.append(order)
    return out


def _multistep_plan(ns, steps, order, skip_type, t_T, t_0, lower_order_final, rec, f):
    if steps < order:
        raise ValueError(f'steps={steps!r}: multistep needs steps >= order')
    ts = time_steps(ns, skip_type, t_T, t_0, steps)
    orders = multistep_orders(steps, order, lower_order_final)
    lam = [ns.lam(ts[i].reshape(1)) for i in range(steps + 1)]
    plan = []
    for i, od in enumerate(orders):          # evaluate at ts[i], update to ts[i + 1]
        p0, t = ts[i].reshape(1), ts[i + 1].reshape(1)
        h = lam[i + 1] - lam[i]
        sig_0, sig_t = ns.std(p0), ns.std(t)
        alpha_t = torch.exp(ns.log_mean_coeff(t))
        phi_1 = torch.expm1(-h)
        fin = dict(c0=f(sig_t / sig_0), c1=f(-(alpha_t * phi_1)))
        if od >= 2:
            h_0 = lam[i] - lam[i - 1]
            r0 = h_0 / h
            fin['k0'] = f(1. / r0)                                   # D1_0 = k0 * (m_0 - m_1)
        if od == 2:                          # multistep_dpm_solver_second_update, 'dpmsolver' form
            fin['c2'] = f(-(0.5 * (alpha_t * phi_1)))
        elif od == 3:                        # multistep_dpm_solver_third_update
            h_1 = lam[i - 1] - lam[i - 2]
            r1 = h_1 / h
            phi_2 = phi_1 / h + 1.
            phi_3 = phi_2 / h - 0.5
            fin.update(k1=f(1. / r1),                                # D1_1 = k1 * (m_1 - m_2)
                       g=f(r0 / (r0 + r1)),                          # D1 = D1_0 + g * (D1_0 - D1_1)
                       k2=f(1. / (r0 + r1)),                         # D2 = k2 * (D1_0 - D1_1)
                       c2=f(alpha_t * phi_2), c3=f(-(alpha_t * phi_3)))
        plan.append(dict(order=od, evals=[rec(p0)], final=fin))
    return dict(steps=plan, outer=ts, orders=orders, method='multistep')


def program(plan):
    """The plan as the flat list of function evaluations the device loop runs, one record each:
      e    : the evaluation record (t_input, sigma, alpha)
      src  : name of the state that is evaluated ('x', or the singlestep inner states 's1', 's2')
      upd  : None, or the solver update done in the evaluation's tail: dict(mode=UPD_*, base, dst (state names),
             h1, h2 (indices of earlier evaluations whose prediction is read, or None), coefficients)
      emit : the state after this evaluation is one of the reference's `intermediates`
    The `denoise` record comes last with upd None: its prediction is the final state."""
    prog = []
    n = 0
    multi = plan.get('method') == 'multistep'
    for st in plan['steps']:
        ev, fin = st['evals'], st['final']
        if multi:
            mode = (UPD_FIRST, UPD_MULTI2, UPD_MULTI3)[st['order'] - 1]
            upd = dict(fin, mode=mode, base='x', dst='x', h1=(n - 1 if st['order'] >= 2 else None),
                       h2=(n - 2 if st['order'] == 3 else None))
            prog.append(dict(e=ev[0], src='x', upd=upd, emit=True))
            n += 1
            continue
        n0 = n
        if st['order'] == 1:
            prog.append(dict(e=ev[0], src='x', emit=True,
                             upd=dict(fin, mode=UPD_FIRST, base='x', dst='x', h1=None, h2=None)))
        else:
            prog.append(dict(e=ev[0], src='x', emit=False,
                             upd=dict(st['to_s1'], mode=UPD_FIRST, base='x', dst='s1', h1=None, h2=None)))
            last = dict(fin, mode=UPD_SINGLE, base='x', dst='x', h1=n0, h2=None)
            last.pop('which')
            if st['order'] == 2:
                prog.append(dict(e=ev[1], src='s1', emit=True, upd=last))
            else:
                prog.append(dict(e=ev[1], src='s1', emit=False,
                                 upd=dict(st['to_s2'], mode=UPD_SINGLE, base='x', dst='s2', h1=n0, h2=None)))
                prog.append(dict(e=ev[2], src='s2', emit=True, upd=last))
        n += st['order']
    if 'denoise' in plan:
        prog.append(dict(e=plan['denoise'], src='x', upd=None, emit=True))
    return prog


def run_program(prog, x, tail, emit_initial=False):
    """Drive `prog` (dpm.program) from state x.  tail(state, e, upd, base, h1, h2) -> (m0, y) is one function
    evaluation with its tail: the quantised data prediction m0 of `state` at record e and, when upd is not None, the
    updated state y.  -> (x, intermediates).  The CPU tests pass torch expressions, the model one HIP launch: one
    control flow for both."""
    st = {'x': x}
    ms = []
    inter = [x] if emit_initial else []
    for op in prog:
        u = op['upd']
        h1 = ms[u['h1']] if u and u['h1'] is not None else None
        h2 = ms[u['h2']] if u and u['h2'] is not None else None
        m0, y = tail(st[op['src']], op['e'], u, st[u['base']] if u else None, h1, h2)
        ms.append(m0)
        st[u['dst'] if u else 'x'] = y if u else m0     # denoise_to_zero: the state BECOMES the prediction
        if op['emit']:
            inter.append(st['x'])
    return st['x'], inter


def update_expr(u, x, m0, h1, h2):
    """The solver updates as the reference's tensor expressions, op by op (works on any fp32 torch tensors)."""
    if u['mode'] == UPD_FIRST:              # dpm_solver_first_update 665-668 (also the singlestep x_s1, 722-725)
        return u['c0'] * x + u['c1'] * m0
    if u['mode'] == UPD_SINGLE:             # singlestep second / third order forms, 728-732, 820-831
        return (u['c0'] * x + u['c1'] * h1) + u['c2'] * (m0 - h1)
    D1_0 = u['k0'] * (m0 - h1)
    if u['mode'] == UPD_MULTI2:             # 915-923
        return (u['c0'] * x + u['c1'] * m0) + u['c2'] * D1_0
    D1_1 = u['k1'] * (h1 - h2)              # 972-985
    D1 = D1_0 + u['g'] * (D1_0 - D1_1)
    D2 = u['k2'] * (D1_0 - D1_1)
    return ((u['c0'] * x + u['c1'] * m0) + u['c2'] * D1) + u['c3'] * D2


def plan_key(steps=20, order=3, method='singlestep', skip_type='time_uniform', t_start=None, t_end=None,
             lower_order_final=True, denoise_to_zero=False):
    """Hashable identity of a solver configuration (plan and HIP-graph caches are keyed by it)."""
    return (int(steps), int(order), str(method), str(skip_type),
            None if t_start is None else float(t_start), None if t_end is None else float(t_end),
            bool(lower_order_final), bool(denoise_to_zero))


def correct_key(clip_denoised, correcting_x0_fn=None, dynamic_thresholding_ratio=0.995, thresholding_max_val=1.0):
    """The correction of x0 an image-space solver call applies, as the extra element of its HIP-graph cache key (the
    time grid does not depend on it, so plan_key does not hold it): ('dynamic', ratio, max_val) when the keyword asks
    for thresholding or -- for False / None, as CondDDPM.generate_imgs passes clip_denoised there (cond_ddpm.py:174-180)
    -- the decoder clips; otherwise ('none', 0., 0.)."""
    if correcting_x0_fn or clip_denoised:
        return ('dynamic', float(dynamic_thresholding_ratio), float(thresholding_max_val))
    return ('none', 0., 0.)


def plan_from_key(betas, key):
    """build_plan of the configuration a plan_key names (the key's order is spelled here and in plan_key alone)."""
    steps, order, method, skip_type, t_start, t_end, lower_order_final, denoise_to_zero = key
    return build_plan(betas, steps=steps, order=order, method=method, skip_type=skip_type, t_start=t_start, t_end=t_end,
                      lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero)


def plan_t_inputs(plan):
    tin = [e['t_input'] for st in plan['steps'] for e in st['evals']]
    return tin + ([plan['denoise']['t_input']] if 'denoise' in plan else [])


def ddim_plan(alphas_bar, steps, eta=0.):
    """Per-step scalars of the reference's DDIM sampler (video_based/models/ddpm/ddim.py:36-218,
    utils.py:50-97; uniform discretisation), computed with the same fp32 torch-CPU expressions.
    Steps are listed in sampling order (largest timestep first)."""
    ab = torch.as_tensor(alphas_bar, dtype=torch.float32).cpu()
    T = ab.shape[0]
    ts = torch.arange(0, T, T // steps) + 1
    a = ab[ts]
    a_prev = torch.cat([ab[:1], ab[ts[:-1]]])
    sig = eta * torch.sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev))
    som = torch.sqrt(1. - a)
    out = []
    n = ts.shape[0]
    for i in range(n):
        index = n - i - 1
        out.append(dict(index=index, t=int(ts[index]), som=float(som[index]),
                        sqrt_a=float(a[index].sqrt()), sqrt_a_prev=float(a_prev[index].sqrt()),
                        dir=float((1. - a_prev[index] - sig[index] ** 2).sqrt()),
                        sigma=float(sig[index])))
    return out
