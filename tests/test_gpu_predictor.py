"""The residual-MLP and LSTM-wrapped slot transitions on the GPU: sdmi_lstm_cell / sdmi_lstm_cell_bwd / sdmi_pred_step
through the C ABI, pinned element by element to float64 references (tests/predictor_ref.py) computed from the tensors
the kernels read, and the video models that use them.

Tolerances, per element, no norms, no share of elements excused (U = 2^-24, BF = 2^-8, the discipline of
test_gpu_igemm_pins.py / test_gpu_bwd_helpers.py):

  expf      a sigmoid or tanh evaluated in fp32 is within e(v) = r |v| + a of its exact value v; one (r, a) row per form
            in EXPF, measured here against float64 (the activated gates sdmi_lstm_cell stores are the direct measure).
  cell      forward, from the pre-activations z (exact inputs):
              gates   e(gate)
              c       |c_prev| e(f) + |g| e(i) + |i| e(g) + e(i) e(g) + 4 U (|f c_prev| + |i g|)
              h       |tanh c| e(o) + |o| (d_c + e(tanh c)) + e(o) (d_c + e(tanh c)) + 4 U |h|
            backward, from the stored gates (exact inputs), t = tanh c, d_t = e(t), dc = dh o (1 - t^2) + dc_next:
              d_dc    |dh o| (2 |t| d_t + d_t^2 + 3 U) + 3 U (|dh o (1 - t^2)| + |dc_next|)
              dz_i    |g i (1 - i)| d_dc + 6 U |dz_i|          dz_f  |c_prev f (1 - f)| d_dc + 6 U |dz_f|
              dz_g    |i| (|1 - g^2| d_dc + 2 U |dc|) + 6 U |dz_g|   dz_o  |dh o (1 - o)| d_t + 6 U |dz_o|
              dc_prev |f| d_dc + 2 U |dc_prev|
  transition (sdmi_pred_step and the composed chain; _ref_and_bound): every product stage with K terms adds
              (K + c) U A,  A = |a| |W|^T + |bias| (+ |residual|),  c = 3 (the fused kernel's bias and residual adds) or
              24 (the composed chain: up to 16 split-K slices summed by the second stage, bias, residual, the second
              GEMM of z adding onto the first)
            on top of the error of its input carried through |W|: d_out = d_in |W|^T.  The stages between are carried by
            their Lipschitz constants: ReLU 1, sigmoid 1/4, tanh 1 (+ the expf row), the cell as above with the gates'
            own errors; LayerNorm in fp32 (two-pass): |g| rstd D U max_row |x| + (D + 8) U |g (x - m) rstd| + 2 U |xn|.
            Every value rounded to bf16 where it feeds an MFMA adds `feed` |v|:
              2 BF   against the reference that rounds there too (both round: they differ by at most one bf16 ulp)
              BF'    against the reference that does not round (half an ulp of the kernel's own value, BF' = 1.01 BF)
              0      the fp32 composed chain; and a value both sides round from the same fp32 input (x in rnn mode, the
                     state) against the rounding reference.

Poison and edges as in test_gpu_igemm_pins.py: inputs live in rows wider than the row with a guard row before and after,
gaps and guards filled with 8192.0; outputs have guard rows of -3.0 that must be unchanged; a second launch gives the same
bits; inputs are unchanged.

Measured on an MI355X, every case of this file: neither EXPF row needed its r (the largest (err - a) / |exact| was 0 for
the sigmoid form and for tanhf).  Largest share of its bound any element used: cell forward 0.158 (the stored gates,
33 x 96), cell backward 0.333 (dz, 33 x 96 with c_prev and dc_next); sdmi_pred_step against the rounding reference 0.014
(y in rnn mode, where one bf16 rounding of h flipped: err 2.4e-4; where no rounding flips the error is ~1e-7 and the
share 0.000 -- the bound is dominated by its 2 BF feed terms); fused against the unrounded reference 0.047; the composed
chain 0.002."""
import functools

import pytest
import torch

from slotdiffusion_amd import engine, kern, ops, spec
from tests import predictor_ref as R
from tests.detfill import det_fill_, is_buffer_name
from tests.test_gpu_bwd_helpers import (BF, DEV, U, _call, _end_the_session_on_a_gpu_fault,  # noqa: F401
                                        _gen, _same_bits, _worst)

pytestmark = pytest.mark.gpu

# (r, a) per evaluated form.  "needs r" = the largest (err - a) / |exact| over every case of this file on an MI355X.
EXPF = {
    'sigmoid': (4e-7, 2e-7),     # 1 / (1 + __expf(-x)): needs r 0
    'tanh': (4e-7, 2e-7),        # tanhf: needs r 0
}
assert all(r <= 4e-6 and a <= 1e-6 for r, a in EXPF.values())
NEED, SHARE = {}, {}
POISON_IN, POISON_OUT = 8192.0, -3.0
F32 = torch.float32


def _e(key, v):
    r, a = EXPF[key]
    return r * v.abs() + a


def _need(key, out, exact):
    r, a = EXPF[key]
    err = (out.double().cpu() - exact).abs()
    NEED[key] = max(NEED.get(key, 0.0), float(((err - a).clamp_min(0) / exact.abs().clamp_min(1e-300)).max()))


def _check(what, out, exact, bound):
    out = out.detach().double().cpu()
    assert out.shape == exact.shape, (what, out.shape, exact.shape)
    assert bool(torch.isfinite(out).all()), what
    err = (out - exact).abs()
    bound = bound.double().expand_as(exact)
    share = float((err / bound.clamp_min(1e-300)).max())
    SHARE[what] = share
    print(f'{what}: max err {float(err.max()):.3e}, largest share of the bound {share:.3f}')
    assert bool((err <= bound).all()), f'{what}: {_worst(err, bound)}'


def _pitched(t, pad):
    """Device copy of t [R, C] inside a poisoned [R + 2, C + pad] buffer -> (buffer, view of the R rows)."""
    Rr, Cc = t.shape
    buf = torch.full((Rr + 2, Cc + pad), POISON_IN, dtype=F32, device=DEV)
    buf[1:Rr + 1, :Cc] = t.to(DEV)
    return buf, buf[1:Rr + 1, :Cc]


def _guarded(Rr, Cc):
    """Output [R, C] with a guard row before and after -> (buffer, view)."""
    buf = torch.full((Rr + 2, Cc), POISON_OUT, dtype=F32, device=DEV)
    return buf, buf[1:Rr + 1]


def _guards_intact(*bufs):
    return all(bool((b[0] == POISON_OUT).all()) and bool((b[-1] == POISON_OUT).all()) for b in bufs)


def _p(t):
    return 0 if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------
# sdmi_lstm_cell / sdmi_lstm_cell_bwd
# ------------------------------------------------------------------------------------------
CELL_SHAPES = [(Rr, H) for Rr in (1, 5, 33) for H in (8, 96)]


@pytest.mark.parametrize('given', [False, True], ids=['null_c_prev', 'c_prev'])
@pytest.mark.parametrize('shape', CELL_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_lstm_cell_forward(shape, given):
    """cell bound of the header; z includes |z| > 20 (every seventh value times 10: up to ~100), where the gates saturate."""
    Rr, H = shape
    g = _gen(Rr * 131 + H + int(given))
    z = torch.randn(Rr, 4 * H, generator=g) * 3
    z.view(-1)[::7] *= 10
    assert float(z.abs().max()) > 20 or z.numel() < 64
    cp = torch.randn(Rr, H, generator=g) * 1.5 if given else None
    zb, zv = _pitched(z, 8)
    cb, cv = _pitched(cp, 4) if given else (None, None)
    before = [b.clone() for b in (zb, cb) if b is not None]
    (hb, h), (cbuf, c), (gb, gates) = _guarded(Rr, H), _guarded(Rr, H), _guarded(Rr, 4 * H)
    runs = []
    for _ in range(2):
        _call('sdmi_lstm_cell', z=_p(zv), c_prev=_p(cv), h=_p(h), c=_p(c), gates=_p(gates), R=Rr, H=H, ldz=4 * H + 8,
              ldcp=(H + 4 if given else 0))
        runs.append([t.clone() for t in (hb, cbuf, gb)])
    assert all(_same_bits(a, b) for a, b in zip(*runs)), 'a second launch gives the same bits'
    assert _guards_intact(hb, cbuf, gb)
    assert all(_same_bits(a, b) for a, b in zip(before, [b for b in (zb, cb) if b is not None])), 'inputs unchanged'
    # without the gates pointer: the same h and c
    (hb2, h2), (cb2, c2) = _guarded(Rr, H), _guarded(Rr, H)
    _call('sdmi_lstm_cell', z=_p(zv), c_prev=_p(cv), h=_p(h2), c=_p(c2), R=Rr, H=H, ldz=4 * H + 8,
          ldcp=(H + 4 if given else 0))
    assert _same_bits(hb2, hb) and _same_bits(cb2, cbuf)
    z64 = z.double()
    cp64 = cp.double() if given else torch.zeros(Rr, H, dtype=torch.float64)
    h64, c64, g64 = R.lstm_cell(z64, cp64)
    i, f, gg, o = g64.chunk(4, -1)
    d_g = torch.cat([_e('sigmoid', i), _e('sigmoid', f), _e('tanh', gg), _e('sigmoid', o)], -1)
    di, df, dg, do = d_g.chunk(4, -1)
    d_c = cp64.abs() * df + gg.abs() * di + i.abs() * dg + di * dg + 4 * U * ((f * cp64).abs() + (i * gg).abs())
    tc = torch.tanh(c64)
    d_t = d_c + _e('tanh', tc)
    d_h = tc.abs() * do + o.abs() * d_t + do * d_t + 4 * U * h64.abs()
    gi, gf, ggg, go = gates.chunk(4, -1)
    for key, got, want in (('sigmoid', torch.cat([gi, gf, go], -1), torch.cat([i, f, o], -1)), ('tanh', ggg, gg)):
        _need(key, got, want)
    tag = f'lstm_cell {Rr}x{H} {"c_prev" if given else "null"}'
    _check(tag + ' gates', gates, g64, d_g)
    _check(tag + ' c', c, c64, d_c)
    _check(tag + ' h', h, h64, d_h)
    print('needs r', NEED)


@pytest.mark.parametrize('given', [False, True], ids=['null_c_prev_dc_next', 'c_prev_dc_next'])
@pytest.mark.parametrize('shape', CELL_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_lstm_cell_backward(shape, given):
    """backward bound of the header; the stored gates include saturated values (exactly 0, exactly 1, 1 - 2^-24)."""
    Rr, H = shape
    g = _gen(Rr * 137 + H + int(given))
    sg = torch.sigmoid(torch.randn(Rr, 3 * H, generator=g) * 4)
    sg.view(-1)[::11] = 1.0
    sg.view(-1)[5::11] = 0.0
    sg.view(-1)[7::11] = 1.0 - 2.0 ** -24
    i, f, o = sg.chunk(3, -1)
    gg = torch.tanh(torch.randn(Rr, H, generator=g) * 2)
    gates = torch.cat([i, f, gg, o], -1).contiguous()
    c = torch.randn(Rr, H, generator=g) * 2
    c.view(-1)[::5] *= 8
    cp = torch.randn(Rr, H, generator=g) * 1.5 if given else None
    dh = torch.randn(Rr, H, generator=g)
    dcn = torch.randn(Rr, H, generator=g) if given else None
    dev = lambda t: None if t is None else t.to(DEV).contiguous()
    gd, cd, dhd, dcnd = dev(gates), dev(c), dev(dh), dev(dcn)
    cb, cv = _pitched(cp, 4) if given else (None, None)
    (dzb, dz), (dcb, dcp) = _guarded(Rr, 4 * H), _guarded(Rr, H)
    runs = []
    for _ in range(2):
        _call('sdmi_lstm_cell_bwd', dh=_p(dhd), dc_next=_p(dcnd), gates=_p(gd), c_prev=_p(cv), c=_p(cd), dz=_p(dz),
              dc_prev=_p(dcp), R=Rr, H=H, ldcp=(H + 4 if given else 0))
        runs.append([dzb.clone(), dcb.clone()])
    assert all(_same_bits(a, b) for a, b in zip(*runs)) and _guards_intact(dzb, dcb)
    i, f, gg, o, c, dh = (t.double() for t in (i, f, gg, o, c, dh))
    cp64 = cp.double() if given else torch.zeros_like(c)
    dcn64 = dcn.double() if given else torch.zeros_like(c)
    t = torch.tanh(c)
    d_t = _e('tanh', t)
    dc = dh * o * (1 - t * t) + dcn64
    d_dc = (dh * o).abs() * (2 * t.abs() * d_t + d_t * d_t + 3 * U) + 3 * U * ((dh * o * (1 - t * t)).abs() + dcn64.abs())
    want = torch.cat([dc * gg * i * (1 - i), dc * cp64 * f * (1 - f), dc * i * (1 - gg * gg), dh * t * o * (1 - o)], -1)
    wi, wf, wg, wo = want.chunk(4, -1)
    bound = torch.cat([(gg * i * (1 - i)).abs() * d_dc + 6 * U * wi.abs(),
                       (cp64 * f * (1 - f)).abs() * d_dc + 6 * U * wf.abs(),
                       i.abs() * ((1 - gg * gg).abs() * d_dc + 2 * U * dc.abs()) + 6 * U * wg.abs(),
                       (dh * o * (1 - o)).abs() * d_t + 6 * U * wo.abs()], -1)
    tag = f'lstm_cell_bwd {Rr}x{H} {"given" if given else "null"}'
    _check(tag + ' dz', dz, want, bound + 1e-45)
    _check(tag + ' dc_prev', dcp, dc * f, f.abs() * d_dc + 2 * U * (dc * f).abs() + 1e-45)


def test_lstm_cell_function_chain_matches_fp64_autograd():
    """kern.LstmCellFn over two chained steps (the second step's dc reaches the first's backward as dc_next) against
    float64 autograd of predictor_ref.lstm_cell.  The kernels are pinned per element above; this checks the wiring (saved
    tensors, None gradients, argument order): a wrong wire is an error of the gradient's own size, so 64 U of its
    largest magnitude (two steps of fp32 arithmetic on unit-scale values stay far below that) separates the two."""
    g = _gen(5)
    Rr, H = 5, 8
    z0, z1 = (torch.randn(Rr, 4 * H, generator=g) for _ in range(2))
    wh, wc = torch.randn(Rr, H, generator=g), torch.randn(Rr, H, generator=g)
    a0, a1 = (t.to(DEV).requires_grad_(True) for t in (z0, z1))
    h0, c0 = kern.LstmCellFn.apply(a0, None)
    h1, c1 = kern.LstmCellFn.apply(a1 + h0.repeat(1, 4), c0)
    ((h1 * wh.to(DEV)).sum() + (c1 * wc.to(DEV)).sum()).backward()
    b0, b1 = (t.double().requires_grad_(True) for t in (z0, z1))
    r0 = R.lstm_cell(b0, torch.zeros(Rr, H, dtype=torch.float64))
    r1 = R.lstm_cell(b1 + r0[0].repeat(1, 4), r0[1])
    ((r1[0] * wh.double()).sum() + (r1[1] * wc.double()).sum()).backward()
    for got, want in ((a0.grad, b0.grad), (a1.grad, b1.grad)):
        assert float((got.double().cpu() - want).abs().max()) <= 64 * U * float(want.abs().max())


# ------------------------------------------------------------------------------------------
# sdmi_pred_step
# ------------------------------------------------------------------------------------------
MODES = {'mlp': (True, False, True), 'mlp_post': (True, False, False), 'rnn': (False, True, True),
         'mlp_rnn': (True, True, True)}            # (mlp, rnn, norm_first)


@functools.lru_cache(None)
def _weights(D, H):
    """fp32 CPU weights of one geometry, matrices on the bf16 grid (so bf16 and fp32 operands hold the same values)."""
    g = _gen(D * 7 + H)
    rn = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(torch.bfloat16).float()
    p, w = 'predictor.base_predictor', 'predictor'
    return {f'{p}.ln.weight': 1 + 0.1 * rn(D), f'{p}.ln.bias': 0.05 * rn(D),
            f'{p}.mlp.0.weight': q(rn(2 * D, D) / D ** 0.5), f'{p}.mlp.0.bias': 0.05 * rn(2 * D),
            f'{p}.mlp.2.weight': q(rn(D, 2 * D) / (2 * D) ** 0.5), f'{p}.mlp.2.bias': 0.05 * rn(D),
            f'{w}.rnn.weight_ih_l0': q(rn(4 * H, D) / D ** 0.5), f'{w}.rnn.weight_hh_l0': q(rn(4 * H, H) / H ** 0.5),
            f'{w}.rnn.bias_ih_l0': 0.05 * rn(4 * H), f'{w}.rnn.bias_hh_l0': 0.05 * rn(4 * H),
            f'{w}.out_projector.weight': q(rn(D, H) / H ** 0.5), f'{w}.out_projector.bias': 0.05 * rn(D)}


@functools.lru_cache(None)
def _packed(D, H):
    return kern.pred_pack(_weights(D, H), 'predictor.base_predictor', 'predictor', device=DEV)


def _ref_and_bound(W, x, state, mlp, rnn, norm_first, rnd, feed, feed_shared, kacc):
    """float64 transition on x [R, D] with `rnd` where a value feeds a product, and the header's bound for a kernel
    whose feeds differ from the reference's by `feed` |v| (`feed_shared` |v| for x in rnn mode and the state).
    -> (y, h, c), (d_y, d_h, d_c)."""
    W = {k: v.double() for k, v in W.items()}
    p, w = 'predictor.base_predictor', 'predictor'
    D = x.shape[1]
    A = lambda a, m, *add: a.abs() @ m.abs().t() + sum(t.abs() for t in add)
    if mlp:
        gam, bet = W[f'{p}.ln.weight'], W[f'{p}.ln.bias']
        m = x.mean(1, keepdim=True)
        xc = x - m
        rstd = ((xc * xc).mean(1, keepdim=True) + 1e-5).rsqrt()
        xn = xc * rstd * gam + bet
        d_xn = gam.abs() * rstd * (D * U * x.abs().amax(1, keepdim=True)) + (D + 8) * U * (gam * xc * rstd).abs() + \
            2 * U * xn.abs()
        w1, b1, w2, b2 = (W[f'{p}.mlp.{k}'] for k in ('0.weight', '0.bias', '2.weight', '2.bias'))
        f0, d_f0 = rnd(xn), d_xn + feed * xn.abs()
        hid = torch.relu(f0 @ w1.t() + b1)
        d_hid = d_f0 @ w1.abs().t() + (D + kacc) * U * A(f0, w1, b1)
        f1, d_f1 = rnd(hid), d_hid + feed * hid.abs()
        res, d_res = (xn, d_xn) if norm_first else (x, torch.zeros_like(x))
        u = f1 @ w2.t() + b2 + res
        d_u = d_f1 @ w2.abs().t() + (2 * D + kacc + 1) * U * A(f1, w2, b2, res) + d_res
        d_fu = d_u + feed * u.abs()
    else:
        u, d_u = x, torch.zeros_like(x)
        d_fu = feed_shared * x.abs()
    if not rnn:
        return (u, None, None), (d_u, None, None)
    wg = torch.cat([W[f'{w}.rnn.weight_ih_l0'], W[f'{w}.rnn.weight_hh_l0']], 1)
    bg = W[f'{w}.rnn.bias_ih_l0'] + W[f'{w}.rnn.bias_hh_l0']
    wo, bo = W[f'{w}.out_projector.weight'], W[f'{w}.out_projector.bias']
    H = wo.shape[1]
    hp, cp = state if state is not None else (x.new_zeros(x.shape[0], H), x.new_zeros(x.shape[0], H))
    a = torch.cat([rnd(u), rnd(hp)], 1)
    d_a = torch.cat([d_fu, feed_shared * hp.abs()], 1)
    z = a @ wg.t() + bg
    d_z = d_a @ wg.abs().t() + (D + H + kacc) * U * A(a, wg, bg)
    h, c, gates = R.lstm_cell(z, cp)
    i, f, g, o = gates.chunk(4, -1)
    dzi, dzf, dzg, dzo = d_z.chunk(4, -1)
    di, df, dg, do = dzi / 4 + _e('sigmoid', i), dzf / 4 + _e('sigmoid', f), dzg + _e('tanh', g), dzo / 4 + _e('sigmoid', o)
    d_c = cp.abs() * df + g.abs() * di + i.abs() * dg + di * dg + 4 * U * ((f * cp).abs() + (i * g).abs())
    tc = torch.tanh(c)
    d_t = d_c + _e('tanh', tc)
    d_h = tc.abs() * do + o.abs() * d_t + do * d_t + 4 * U * h.abs()
    fh, d_fh = rnd(h), d_h + feed * h.abs()
    y = fh @ wo.t() + bo
    d_y = d_fh @ wo.abs().t() + (H + kacc) * U * A(fh, wo, bo)
    return (y, h, c), (d_y, d_h, d_c)


def _launch_fused(P, xv, ldx, hv, cv, ldh, Rr, D, H, mode, norm_first):
    (yb, y), (hb, h), (cb, c) = _guarded(Rr, D), _guarded(Rr, max(H, 1)), _guarded(Rr, max(H, 1))
    rnn = bool(mode & ops.PRED_RNN)
    runs = []
    for _ in range(2):
        _call('sdmi_pred_step', x=_p(xv), h_prev=_p(hv), c_prev=_p(cv), y=_p(y), h=_p(h if rnn else None),
              c=_p(c if rnn else None), ln_g=_p(P['ln_g']), ln_b=_p(P['ln_b']), w1p=_p(P['w1p']), b1=_p(P['b1']),
              w2p=_p(P['w2p']), b2=_p(P['b2']), wgp=_p(P['wgp']), bg=_p(P['bg']), wop=_p(P['wop']), bo=_p(P['bo']),
              R=Rr, D=D, H=(H if rnn else 0), ldx=ldx, ldh=ldh, mode=mode, norm_first=int(norm_first), eps=1e-5)
        runs.append([yb.clone(), hb.clone(), cb.clone()])
    assert all(_same_bits(a, b) for a, b in zip(*runs)), 'a second launch gives the same bits'
    assert _guards_intact(yb, hb, cb), 'rows the launch does not own are unchanged'
    if not rnn:
        assert bool((hb == POISON_OUT).all()) and bool((cb == POISON_OUT).all())
    return y, (h if rnn else None), (c if rnn else None)


@pytest.mark.parametrize('geom', [(32, 64), (192, 384)], ids=lambda g: f'D{g[0]}H{g[1]}')
@pytest.mark.parametrize('Rr', [1, 17, 77])
@pytest.mark.parametrize('mode', list(MODES))
def test_pred_step_against_fp64(mode, Rr, geom):
    """transition bound of the header against the reference that rounds where the kernel rounds (feed 2 BF, shared feeds
    0): step 0 with a null state, then step 1 on another x with the state the kernel itself produced (handed back in
    pitched, poisoned rows).  R = 77: five workgroups, the last with 13 of its 16 rows."""
    D, H = geom
    mlp, rnn, norm_first = MODES[mode]
    W, P = _weights(D, H), _packed(D, H)
    flag = (ops.PRED_MLP if mlp else 0) | (ops.PRED_RNN if rnn else 0)
    g = _gen(Rr * 17 + D)
    state_dev = state64 = None
    for step in range(2 if rnn else 1):
        x = torch.randn(Rr, D, generator=g) * (1.5 if step else 1.0)
        xb, xv = _pitched(x, 4)
        hv = cv = hbuf = cbuf = None
        if state_dev is not None:
            (hbuf, hv), (cbuf, cv) = _pitched(state_dev[0].cpu(), 4), _pitched(state_dev[1].cpu(), 4)
        before = [b.clone() for b in (xb, hbuf, cbuf) if b is not None]
        y, h, c = _launch_fused(P, xv, D + 4, hv, cv, H + 4 if hv is not None else 0, Rr, D, H, flag, norm_first)
        assert all(_same_bits(a, b) for a, b in zip(before, [b for b in (xb, hbuf, cbuf) if b is not None]))
        (y64, h64, c64), (dy, dh, dc) = _ref_and_bound(W, x.double(), state64, mlp, rnn, norm_first, R.bf16, 2 * BF, 0.0, 3)
        tag = f'pred_step {mode} R{Rr} D{D}H{H} step{step}'
        _check(tag + ' y', y, y64, dy)
        if rnn:
            _check(tag + ' h', h, h64, dh)
            _check(tag + ' c', c, c64, dc)
            state_dev = (h.clone(), c.clone())
            state64 = (h.double().cpu(), c.double().cpu())


def test_pred_step_rejects_uncovered_geometry():
    P = _packed(32, 64)
    x = torch.zeros(4, 40, device=DEV)
    with pytest.raises(Exception, match='multiple of 32'):
        _call('sdmi_pred_step', x=_p(x), y=_p(torch.empty_like(x)), ln_g=_p(P['ln_g']), ln_b=_p(P['ln_b']),
              w1p=_p(P['w1p']), b1=_p(P['b1']), w2p=_p(P['w2p']), b2=_p(P['b2']), R=4, D=40, H=0, ldx=40, mode=1,
              norm_first=1, eps=1e-5)


# ------------------------------------------------------------------------------------------
# composed chain and dispatch, on a model's weight bank
# ------------------------------------------------------------------------------------------
def _spy(fn):
    seen, orig = {}, kern.call

    def spy(fname, *a, **k):
        seen[fname] = seen.get(fname, 0) + 1
        return orig(fname, *a, **k)
    kern.call = ops.call = spy
    try:
        out = fn()
    finally:
        kern.call = ops.call = orig
    return out, seen


def _savi(D, H, case, dtype, sg_every=None, T=4):
    """Tiny SAVi with a [D, H] transition whose predictor tensors are _weights(D, H) (on the bf16 grid)."""
    from slotdiffusion_amd import models
    cfg = R.tiny_cfg('SAVi', case, sg_every)
    cfg['slot_dict'].update(slot_size=D, slot_mlp_size=H)
    cfg['enc_dict']['enc_out_channels'] = D
    cfg['dec_dict']['dec_channels'] = (D, 16, 16, 16, 16)
    cfg.pop('model'), cfg.pop('input_frames')
    m = models.SAVi(clip_len=T, **cfg, compute_dtype=dtype)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    W = _weights(D, H)
    sd = m.state_dict()
    with torch.no_grad():
        for k, v in W.items():
            key = k if k in sd else k.replace('.base_predictor', '')
            if key in sd:
                sd[key].copy_(v)
    m.pred_dropout = 0.0
    return m.cuda().eval()


def _bank_weights(m, rnn):
    """The model's predictor tensors under the names _ref_and_bound reads."""
    sd = {k: v.detach().float().cpu() for k, v in m.state_dict().items() if k.startswith('predictor.')}
    return sd if rnn else {k.replace('predictor.', 'predictor.base_predictor.'): v for k, v in sd.items()}


def test_uncovered_geometry_runs_composed_and_matches_fp64():
    """D = 40, H = 24 is outside pred_step_covers: a bf16 model runs the composed chain (fp32 arithmetic on the master
    weights, like the transformer predictor) -- transition bound with feed 0 and c = 24, two calls (the state carries)."""
    D, H, Rr = 40, 24, 6
    m = _savi(D, H, 'mlp_rnn', torch.bfloat16)
    W = _bank_weights(m, True)
    K = m.K()                                         # (the bank's own first-use launches stay out of the count)
    st = engine.PredictorState()
    g = _gen(3)
    state64 = None
    for step in range(2):
        x = torch.randn(2, 3, D, generator=g)
        with torch.no_grad():
            y, seen = _spy(lambda: engine.slot_transition(K, x.cuda(), m.pred_dict, st))
        assert 'sdmi_pred_step' not in seen and seen.get('sdmi_lstm_cell') == 1 and seen.get('sdmi_igemm', 0) >= 5
        (y64, h64, c64), (dy, dh, dc) = _ref_and_bound(W, x.reshape(Rr, D).double(), state64, True, True, True, R.ident,
                                                      0.0, 0.0, 24)
        _check(f'composed D40H24 step{step} y', y.reshape(Rr, D), y64, dy)
        _check(f'composed D40H24 step{step} h', st.hidden[0], h64, dh)
        _check(f'composed D40H24 step{step} c', st.hidden[1], c64, dc)
        state64 = (st.hidden[0].double().cpu(), st.hidden[1].double().cpu())


@pytest.mark.parametrize('case', ['mlp', 'mlp_rnn'])
def test_fused_and_composed_each_within_own_bound_of_one_reference(case):
    """One float64 reference (no rounding anywhere; the weights are on the bf16 grid, so the bf16 operands of the fused
    launch and the fp32 master weights of the composed chain hold the same values).  Fused: feed BF' on every feed.
    Composed (kern._PRED_FUSED off): feed 0, c = 24.  They are not compared with each other."""
    D, H, Rr = 32, 64, 6
    rnn = case == 'mlp_rnn'
    m = _savi(D, H, case, torch.bfloat16)
    W = _bank_weights(m, rnn)
    K = m.K()
    x = torch.randn(2, 3, D, generator=_gen(8))
    (y64, _, _), (dy_f, _, _) = _ref_and_bound(W, x.reshape(Rr, D).double(), None, True, rnn, True, R.ident, 1.01 * BF,
                                               1.01 * BF, 3)
    _, (dy_c, _, _) = _ref_and_bound(W, x.reshape(Rr, D).double(), None, True, rnn, True, R.ident, 0.0, 0.0, 24)
    with torch.no_grad():
        yf, seen = _spy(lambda: engine.slot_transition(K, x.cuda(), m.pred_dict, engine.PredictorState()))
        assert seen == {'sdmi_pred_step': 1}
        kern._PRED_FUSED = False
        try:
            yc, seen = _spy(lambda: engine.slot_transition(K, x.cuda(), m.pred_dict, engine.PredictorState()))
        finally:
            kern._PRED_FUSED = True
        assert 'sdmi_pred_step' not in seen and seen.get('sdmi_igemm', 0) >= 2
    _check(f'{case} fused vs unrounded fp64', yf.reshape(Rr, D), y64, dy_f)
    _check(f'{case} composed vs unrounded fp64', yc.reshape(Rr, D), y64, dy_c)


# ------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------
NEW = ('mlp', 'mlp_rnn', 'transformer_rnn')


def _clip(T, seed=4):
    return (torch.randn(2, T, 3, 32, 32, generator=_gen(seed)) * 0.5).clamp(-1, 1)


@functools.lru_cache(None)
def _model(name, case, dtype=F32, sg_every=None):
    return R.build_tiny(name, case, sg_every, compute_dtype=dtype).cuda().eval()


def _encode(m, img, prev=None):
    out = m.encode(img, prev)
    return out[0] if isinstance(out, tuple) else out


def _ref_weights(m, dtype=torch.float64):
    return {k: v.detach().cpu().to(dtype) for k, v in m.state_dict().items() if not k.startswith(('dm_decoder.', 'decoder'))}


@pytest.mark.parametrize('name,bar', [('SAVi', 5e-5), ('SAViDiffusion', 1e-4)])
@pytest.mark.parametrize('case', NEW)
def test_model_slots_fp32_match_restatement(case, name, bar):
    """Tiny model (32 x 32 frames, T = 4, B = 2, 3 slots, D = 32, H = 64) in fp32 against predictor_ref composed with
    the oracle's encoder and Slot Attention, in float64.  Bars: the ones test_gpu_model.py holds the video models'
    slots to (SAVi 5e-5, SAViDiffusion 1e-4, largest absolute error)."""
    m = _model(name, case)
    img = _clip(4)
    with torch.no_grad():
        slots = _encode(m, img.cuda())
    plan = spec.encoder_plan(m.resolution, m.enc_dict)[0]
    want = R.clip_slots(_ref_weights(m), img.double(), plan, m.num_iterations, m.pred_dict, m.eps)
    err = float((slots.double().cpu() - want).abs().max())
    print(f'{name} {case}: slots max err {err:.2e} of {float(want.abs().max()):.2f}')
    assert slots.shape == want.shape and err <= bar


@pytest.mark.parametrize('case', ['mlp_rnn', 'transformer_rnn'])
def test_state_carries_across_encode_calls_and_resets(case):
    """encode(img[:, :2]) then encode(img[:, 2:], prev_slots) equals encode(img) bit for bit; a forward without
    prev_slots after that equals the first one bit for bit (the state was reset)."""
    m = _model('SAVi', case)
    img = _clip(4).cuda()
    with torch.no_grad():
        full = _encode(m, img).clone()
        a = _encode(m, img[:, :2].contiguous()).clone()
        b = _encode(m, img[:, 2:].contiguous(), a[:, -1].contiguous()).clone()
        assert m.pred_state.step == 3
        again = _encode(m, img).clone()
    assert _same_bits(again, full), 'a forward without prev_slots starts from a zero state'
    assert _same_bits(torch.cat([a, b], 1), full), 'a continuation carries the state'


def _grad_case(name, case, T, sg_every, frame_weights):
    """Gradients of sum(slots * w) on our model (train mode, fp32) and by autograd on the restatement in float64 and in
    fp32.  -> {tensor name: (ours, fp64, fp32)} for the predictor's tensors, init_latents and the encoder's first and
    last tensors (the image is data here: encoder.conv1.weight is the input end of the time chain)."""
    m = _model(name, case, F32, sg_every).train()
    m.pred_dropout = 0.0
    img = _clip(T, seed=6)
    w = torch.randn(2, T, 3, R.D, generator=_gen(12)) * frame_weights.view(1, T, 1, 1)
    names = [k for k, _ in m.named_parameters() if k.startswith('predictor.')] + \
        ['init_latents', 'encoder.conv1.weight', 'encoder_out_layer.3.weight']
    try:
        m.grad_arena().zero_()
        slots = _encode(m, img.cuda())
        (slots * w.cuda()).sum().backward()
        torch.cuda.synchronize()
        named = dict(m.named_parameters())
        ours = {k: named[k].grad.detach().double().cpu().clone() for k in names}
    finally:
        m.eval()
    plan = spec.encoder_plan(m.resolution, m.enc_dict)[0]
    refs = []
    for dt in (torch.float64, torch.float32):
        W = {k: v.requires_grad_(k in names) for k, v in _ref_weights(m, dt).items()}
        s = R.clip_slots(W, img.to(dt), plan, m.num_iterations, m.pred_dict, m.eps)
        (s * w.to(dt)).sum().backward()
        refs.append({k: (W[k].grad.double() if W[k].grad is not None else torch.zeros_like(W[k]).double()) for k in names})
    return {k: (ours[k], refs[0][k], refs[1][k]) for k in names}


def _assert_grads(tag, G):
    """Per tensor, per element: |ours - fp64| <= 8 x the largest error of the restatement's own fp32 evaluation against
    its float64 one on that tensor, never below 64 U of the tensor's largest gradient -- the reference's own fp32 error
    is the measure of what fp32 arithmetic through this depth of chain costs; 8 covers another summation order."""
    for k, (ours, g64, g32) in G.items():
        bound = max(8 * float((g32 - g64).abs().max()), 64 * U * float(g64.abs().max()))
        err = float((ours - g64).abs().max())
        print(f'{tag} {k}: err {err:.2e} bound {bound:.2e} |g| {float(g64.abs().max()):.2e}')
        assert err <= bound, (tag, k, err, bound)


@pytest.mark.parametrize('name', ['SAVi', 'SAViDiffusion'])
@pytest.mark.parametrize('case', NEW)
def test_training_gradients_through_time_match_fp64_autograd(case, name):
    """T = 3: every predictor tensor, init_latents and both ends of the encoder, through the chain of frames."""
    G = _grad_case(name, case, 3, None, torch.ones(3))
    assert all(float(g64.abs().max()) > 0 for _, g64, _ in G.values())
    _assert_grads(f'{name} {case}', G)


@pytest.mark.parametrize('case', ['mlp_rnn', 'transformer_rnn'])
def test_sg_every_cuts_the_chain_at_step_two(case):
    """pred_sg_every = 2, T = 4: the third transition (step 2, into frame 3) detaches its input and the state.  With a
    loss on frame 3 alone nothing reaches what lies before the cut: init_latents takes exactly zero gradient, and every
    tensor matches the restatement that detaches there; with a loss on all frames the gradients match it too."""
    G = _grad_case('SAVi', case, 4, 2, torch.tensor([0., 0., 0., 1.]))
    ours, g64, _ = G['init_latents']
    assert float(g64.abs().max()) == 0.0 and float(ours.abs().max()) == 0.0
    _assert_grads(f'sg2 frame3 {case}', G)
    _assert_grads(f'sg2 all {case}', _grad_case('SAVi', case, 4, 2, torch.ones(4)))
    # and the cut is real: without it init_latents does take gradient from frame 3
    G0 = _grad_case('SAVi', case, 4, None, torch.tensor([0., 0., 0., 1.]))
    assert float(G0['init_latents'][0].abs().max()) > 0.0


@pytest.mark.parametrize('case', NEW)
def test_bf16_eval_engages_the_fused_step_once_per_transition(case):
    """bf16 eval: exactly one sdmi_pred_step per frame transition (T - 1 = 3) and no sdmi_lstm_cell; the fp32 model and a
    gradient-recording bf16 model log the composed calls instead."""
    rnn = R.VARIANTS[case]['pred_rnn']
    img = _clip(4).cuda()
    assert kern._PRED_FUSED is True
    m16 = _model('SAVi', case, torch.bfloat16)
    with torch.no_grad():
        _, seen = _spy(lambda: _encode(m16, img))
    assert seen.get('sdmi_pred_step') == 3 and 'sdmi_lstm_cell' not in seen, seen
    with torch.no_grad():
        _, seen = _spy(lambda: _encode(_model('SAVi', case), img))
    assert 'sdmi_pred_step' not in seen and seen.get('sdmi_lstm_cell', 0) == (3 if rnn else 0), seen
    m16.train()
    try:
        m16.grad_arena().zero_()
        slots, seen = _spy(lambda: _encode(m16, img))
        assert slots.requires_grad
        assert 'sdmi_pred_step' not in seen and seen.get('sdmi_lstm_cell', 0) == (3 if rnn else 0), seen
        _, seen = _spy(lambda: slots.float().sum().backward())
        assert seen.get('sdmi_lstm_cell_bwd', 0) == (3 if rnn else 0), seen
    finally:
        m16.eval()
