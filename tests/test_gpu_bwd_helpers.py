"""The small streaming kernels of a training step, each called through the C ABI and pinned to a
float64 CPU reference computed from the inputs the kernel saw (rounded to bf16 first for bf16 storage).

Every tolerance in this file is one of three kinds, and each test's docstring says which:

  bit-exact   the output bits are predictable (copies, one fp32 add, a fixed fp32 expression, one rounding to bf16).
  derived     a per-element bound the test computes in float64 from the operation itself:
                fp32 sums of n terms       n * 2^-24 * sum|terms|  +  4 * 2^-24 * |exact|
                bf16 storage               2^-8 * |exact|  +  the fp32 bound of the same case
              (2^-8 |x| is half a bf16 ulp: the fp32 value is rounded once).  No norms, no "share of elements".
  expf        kernels that go through the hardware exponential (__expf): |out - exact| <= r * |exact| + a * |dy|
              per element (|dy| = 1 where the operation has no incoming gradient).  (r, a) start at the forward
              activation test's (4e-7, 2e-7); EXPF below lists them per kernel with the largest error measured on
              an MI355X beside each.  r never exceeds 4e-6 (about three times the argument-rounding error of a
              hardware exp at |x| <= 12, 12 * log2(e) * 2^-24) and a never exceeds 1e-6.  gelu and gelu' below
              x = -4 get the absolute term only: 0.5 (1 + erf) cancels there in any fp32 evaluation.
              The expf bound pins the fp32 instantiations.  The fast forms that only bf16 storage compiles (v_rcp SiLU,
              the branch-free erf: act_apply<true> / act_grad<true>) are pinned to half a bf16 ulp on top of it, no
              tighter: an error of 1e-4 relative inside them would pass here.

The shapes are the smallest that reach the path named beside them: ragged tails, more rows than one grid covers
(the second trip of the grid-stride loops: 4096 x 256 threads for the element-wise kernels, 2048 x 256 for the GRU
gates and the quantizer backward, 256 x 256 vectors for the segment tables), row pitches wider than the row."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = 'cuda'
U = 2.0 ** -24              # fp32 unit roundoff
BF = 2.0 ** -8              # half a bf16 ulp, relative
CAP = 4096 * 256            # threads of the largest element-wise grid
CAP_ROWS = 2048 * 256       # ... of gru_gates* and vq_bwd
DTYPES = [torch.float32, torch.bfloat16]
_ID = {torch.float32: 'fp32', torch.bfloat16: 'bf16'}

# (r, a) of the expf bound, per kernel and, where the outputs differ, per activation or output.  "needs r" = max over
# elements of (err - a |dy|) / |exact| measured on an MI355X, fp32 storage, over every case of this file.  Where it
# exceeds the starting 4e-7, r = twice the measurement, rounded up to one digit.
EXPF = {
    'act': (4e-7, 2e-7),               # needs r 7.3e-8 (silu bf16 -> fp32)
    # silu' = s (1 + x (1 - s)): for x above ~8 the 1 - s cancels and x multiplies the half ulp of s
    'act_bwd/silu': (2e-6, 2e-7),      # needs r 5.4e-7 (both the sweep and the wrap case)
    'act_bwd/gelu': (4e-7, 2e-7),      # needs r 0
    'act_bwd/relu': (4e-7, 2e-7),      # needs r 0 (exact)
    'geglu': (4e-7, 2e-7),             # needs r 9.6e-8
    'geglu_bwd': (4e-7, 2e-7),         # needs r 1.0e-7
    'gru_gates': (4e-7, 2e-7),         # needs r 9.9e-8
    'gru_gates_bwd/r': (4e-7, 2e-7),   # gate columns of dgi and dgh; needs r 0
    # dz-gate = dh (h - n) z (1 - z): a saturated z leaves 1 - z with the absolute error of z, times |h - n| up to ~5
    'gru_gates_bwd/z': (2e-6, 2e-7),   # needs r 5.5e-7 (2731 x 192; the smaller shapes 9.5e-9)
    'gru_gates_bwd/n': (4e-7, 2e-7),   # needs r 0
    'gru_gates_bwd/dh': (4e-7, 2e-7),  # needs r 0
    'sa_combine': (4e-7, 2e-7),        # needs r 1.4e-7
    'sa_combine_bwd': (4e-7, 2e-7),    # needs r 6.9e-8
}
assert all(r <= 4e-6 and a <= 1e-6 for r, a in EXPF.values())
NEED = {}       # largest r each EXPF key needed so far in this session (for a measuring script to read after a run)


# ---- plumbing ------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _end_the_session_on_a_gpu_fault():
    """A kernel fault surfaces at the next synchronisation: stop there instead of running the rest on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'GPU fault: {e}', returncode=3)


def _L():
    from slotdiffusion_amd import _lib
    return _lib


def _call(fname, **kw):
    _L().call(fname, torch.cuda.current_stream().cuda_stream, **kw)


def _dt(dtype):
    return _L().BF16 if dtype == torch.bfloat16 else _L().F32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _q(t, dtype):
    """Round a CPU fp32 tensor to the storage dtype's grid (both sides then see equal inputs)."""
    return t.to(dtype).float()


def _dev(t, dtype=None):
    return (t if dtype is None else t.to(dtype)).contiguous().to(DEV)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _poison(shape, dtype, value=-3.0):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def _worst(err, bound):
    over = (err - bound).reshape(-1)
    i = int(over.argmax())
    return f'element {i}: err {float(err.reshape(-1)[i]):.3e} > bound {float(bound.reshape(-1)[i]):.3e}'


def _check_derived(what, out, exact, bound, bf16=False):
    """|out - exact| <= bound (+ half a bf16 ulp of the exact value for bf16 storage), every element."""
    out, exact = out.detach().double().cpu(), exact.detach().double()
    assert out.shape == exact.shape, (what, out.shape, exact.shape)
    assert bool(torch.isfinite(out).all()), what
    err = (out - exact).abs()
    bound = bound.double().expand_as(exact) + (BF * exact.abs() if bf16 else 0.0)
    assert bool((err <= bound).all()), f'{what}: {_worst(err, bound)}'


def _check_expf(key, what, out, exact, dy=None, abs_only=None, bf16=False):
    """The expf bound of the module docstring; records the r this case needs in NEED before asserting."""
    r, a = EXPF[key]
    out, exact = out.detach().double().cpu(), exact.detach().double()
    assert out.shape == exact.shape, (what, out.shape, exact.shape)
    assert bool(torch.isfinite(out).all()), what
    mag = exact.abs()
    absb = a * (dy.detach().double().abs().expand_as(exact) if dy is not None else torch.ones_like(mag))
    if bf16:
        absb = absb + BF * mag
    err = (out - exact).abs()
    rel = torch.full_like(mag, r)
    if abs_only is not None:
        rel = torch.where(abs_only.expand_as(exact), torch.zeros_like(rel), rel)
    over = (err - absb).clamp_min(0.0)
    need = over / mag.clamp_min(1e-300)
    if abs_only is not None:
        need = need[~abs_only.expand_as(exact)]
    if not bf16:
        NEED[key] = max(NEED.get(key, 0.0), float(need.max()) if need.numel() else 0.0)
    bound = rel * mag + absb
    assert bool((err <= bound).all()), f'{key} {what}: {_worst(err, bound)}'


# ---- activations ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _sweep():
    return torch.cat([torch.linspace(-12, 12, 200001),
                      torch.tensor([0.0, -0.0, 100.0, -100.0, 1.3120, -1.3120])])


def _act64(x, kind):
    x = x.double()
    return {'silu': F.silu, 'gelu': F.gelu, 'relu': F.relu}[kind](x)


def _act_grad64(x, kind):
    """Analytic derivative in float64 (erfc keeps the negative GELU tail accurate)."""
    x = x.double()
    if kind == 'relu':
        return (x > 0).double()
    if kind == 'silu':
        s = torch.sigmoid(x)
        return s * (1 + x * (1 - s))
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _run_act_bwd(x, dy, kind, dtype):
    xd, dyd = _dev(x, dtype), _dev(dy, dtype)
    dx = _poison(xd.shape, dtype)
    _call('sdmi_act_bwd', x=xd.data_ptr(), dy=dyd.data_ptr(), dx=dx.data_ptr(), dtype=_dt(dtype),
          act=_L().ACT[kind], n=xd.numel())
    return dx


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('kind', ['silu', 'gelu', 'relu'])
def test_act_bwd_sweep(kind, dtype):
    """act_grad point-wise over [-12, 12] plus {0, -0, +-100, +-1.312}, dy = 1.  expf bound (bf16: + half an ulp)."""
    x = _q(_sweep(), dtype)
    dx = _run_act_bwd(x, torch.ones_like(x), kind, dtype)
    _check_expf('act_bwd/' + kind, f'{_ID[dtype]} sweep', dx, _act_grad64(x, kind),
                abs_only=(x < -4.0) if kind == 'gelu' else None, bf16=dtype == torch.bfloat16)


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('kind', ['silu', 'gelu', 'relu'])
def test_act_bwd_grid_stride_wrap(kind, dtype):
    """n = 4096 * 256 + 257: the last 257 elements are served by the second trip of the grid-stride loop.
    Random dy; expf bound scaled by |dy| (bf16: + half an ulp)."""
    n = CAP + 257
    g = _gen(11)
    x, dy = _q(torch.randn(n, generator=g) * 3, dtype), _q(torch.randn(n, generator=g), dtype)
    dx = _run_act_bwd(x, dy, kind, dtype)
    _check_expf('act_bwd/' + kind, f'{_ID[dtype]} wrap', dx, dy.double() * _act_grad64(x, kind), dy=dy,
                abs_only=(x < -4.0) if kind == 'gelu' else None, bf16=dtype == torch.bfloat16)


@pytest.mark.parametrize('src,dst', [(torch.float32, torch.bfloat16), (torch.bfloat16, torch.float32)],
                         ids=['fp32_to_bf16', 'bf16_to_fp32'])
@pytest.mark.parametrize('kind', ['silu', 'gelu'])
def test_act_mixed_dtypes(kind, src, dst):
    """sdmi_act converting while it applies the activation, same sweep.  expf bound at the forward test's (r, a);
    bf16 destination: + half an ulp."""
    x = _q(_sweep(), src)
    xd = _dev(x, src)
    y = _poison(xd.shape, dst)
    _call('sdmi_act', x=xd.data_ptr(), y=y.data_ptr(), src_dtype=_dt(src), dst_dtype=_dt(dst),
          act=_L().ACT[kind], n=xd.numel())
    _check_expf('act', f'{kind} {_ID[src]}->{_ID[dst]}', y, _act64(x, kind),
                abs_only=(x < -4.0) if kind == 'gelu' else None, bf16=dst == torch.bfloat16)


# ---- GEGLU ---------------------------------------------------------------------------------------------
GEGLU_SHAPES = [(5, 8), (37, 520), (2049, 2056)]      # the last: 2049 * 514 fp32 vectors > 4096 * 256


@functools.lru_cache(None)
def _geglu_case(rows, C, dtype):
    g = _gen(rows * 31 + C)
    h = _q(torch.randn(rows, 2 * C, generator=g) * 1.5, dtype)
    dy = _q(torch.randn(rows, C, generator=g), dtype)
    h64 = h.double().requires_grad_(True)
    y = h64[:, :C] * F.gelu(h64[:, C:])
    y.backward(dy.double())
    return h, dy, y.detach(), h64.grad


def _check_geglu(h, dy, y64, dh64, y, dh, dtype, tag):
    C = dy.shape[1]
    bf = dtype == torch.bfloat16
    x, gate = h[:, :C], h[:, C:]
    tail = gate < -4.0
    if y is not None:
        _check_expf('geglu', tag, y, y64, dy=x, abs_only=tail, bf16=bf)
    _check_expf('geglu_bwd', tag + ' dx', dh[:, :C], dh64[:, :C], dy=dy, abs_only=tail, bf16=bf)
    _check_expf('geglu_bwd', tag + ' dgate', dh[:, C:], dh64[:, C:], dy=dy * x, abs_only=tail, bf16=bf)


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('shape', GEGLU_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_geglu_and_bwd(shape, dtype):
    """y = x * gelu(gate) and its backward against fp64 autograd.  expf bound scaled by the factor that multiplies
    the activation (|x| forward, |dy| and |dy x| backward); bf16: + half an ulp."""
    rows, C = shape
    h, dy, y64, dh64 = _geglu_case(rows, C, dtype)
    hd, dyd = _dev(h, dtype), _dev(dy, dtype)
    y, dh = _poison((rows, C), dtype), _poison((rows, 2 * C), dtype)
    _call('sdmi_geglu', h=hd.data_ptr(), y=y.data_ptr(), dtype=_dt(dtype), rows=rows, C=C)
    _call('sdmi_geglu_bwd', h=hd.data_ptr(), dy=dyd.data_ptr(), dh=dh.data_ptr(), dtype=_dt(dtype), rows=rows, C=C)
    _check_geglu(h, dy, y64, dh64, y, dh, dtype, f'{rows}x{C} {_ID[dtype]}')


def test_geglu_function_wiring():
    """kern.GegluFn (forward + backward through torch.autograd) at the ragged shape: same expf bounds."""
    from slotdiffusion_amd.kern import GegluFn
    rows, C = 37, 520
    h, dy, y64, dh64 = _geglu_case(rows, C, torch.float32)
    hd = _dev(h).requires_grad_(True)
    y = GegluFn.apply(hd)
    y.backward(_dev(dy))
    _check_geglu(h, dy, y64, dh64, y, hd.grad, torch.float32, 'GegluFn')


# ---- GRU gates -----------------------------------------------------------------------------------------
GRU_SHAPES = [(1, 1), (14, 192), (3, 65), (2731, 192)]     # the last: 2731 * 192 > 2048 * 256


@functools.lru_cache(None)
def _gru_case(R, D):
    g = _gen(R * 7 + D)
    gi, gh = torch.randn(R, 3 * D, generator=g), torch.randn(R, 3 * D, generator=g)
    h, dout = torch.randn(R, D, generator=g), torch.randn(R, D, generator=g)
    a, b, c = (t.double().requires_grad_(True) for t in (gi, gh, h))
    r = torch.sigmoid(a[:, :D] + b[:, :D])                       # torch.nn.GRUCell's gate algebra
    z = torch.sigmoid(a[:, D:2 * D] + b[:, D:2 * D])
    n = torch.tanh(a[:, 2 * D:] + r * b[:, 2 * D:])
    out = (1 - z) * n + z * c
    out.backward(dout.double())
    return gi, gh, h, dout, out.detach(), a.grad, b.grad, c.grad


def _check_gru(case, out, dgi, dgh, dh, tag):
    gi, gh, h, dout, out64, dgi64, dgh64, dh64 = case
    _check_expf('gru_gates', tag, out, out64)
    d3 = dout.repeat(1, 3)
    D = dout.shape[1]
    for name, got, want in (('dgi', dgi, dgi64), ('dgh', dgh, dgh64)):
        for k, gate in enumerate('rzn'):
            c = slice(k * D, (k + 1) * D)
            _check_expf('gru_gates_bwd/' + gate, f'{tag} {name}', got[:, c], want[:, c], dy=d3[:, c])
    _check_expf('gru_gates_bwd/dh', tag + ' dh', dh, dh64, dy=dout)


@pytest.mark.parametrize('shape', GRU_SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_gru_gates_and_bwd(shape):
    """GRUCell gate arithmetic on given gi, gh, h against fp64 autograd.  expf bound, backward scaled by |dhout|."""
    R, D = shape
    case = _gru_case(R, D)
    gi, gh, h, dout = (_dev(t) for t in case[:4])
    out, dgi, dgh, dh = _poison((R, D), torch.float32), _poison((R, 3 * D), torch.float32), \
        _poison((R, 3 * D), torch.float32), _poison((R, D), torch.float32)
    _call('sdmi_gru_gates', gi=gi.data_ptr(), gh=gh.data_ptr(), h=h.data_ptr(), hout=out.data_ptr(), R=R, D=D)
    _call('sdmi_gru_gates_bwd', gi=gi.data_ptr(), gh=gh.data_ptr(), h=h.data_ptr(), dhout=dout.data_ptr(),
          dgi=dgi.data_ptr(), dgh=dgh.data_ptr(), dh=dh.data_ptr(), R=R, D=D)
    _check_gru(case, out, dgi, dgh, dh, f'{R}x{D}')


def test_gru_gates_function_wiring():
    """kern.GruGatesFn through torch.autograd: same expf bounds."""
    from slotdiffusion_amd.kern import GruGatesFn
    case = _gru_case(14, 192)
    gi, gh, h = (_dev(t).requires_grad_(True) for t in case[:3])
    out = GruGatesFn.apply(gi, gh, h)
    out.backward(_dev(case[3]))
    _check_gru(case, out, gi.grad, gh.grad, h.grad, 'GruGatesFn')


# ---- plain-SA decoder combine --------------------------------------------------------------------------
# (B, N, HW, ldo, hard): hard = alpha logits x8 + 100, where the max subtraction decides the result
SA_CASES = [(2, 7, 100, 4, False), (1, 1, 37, 8, False), (3, 11, 63, 8, True)]


@functools.lru_cache(None)
def _sa_case(B, N, HW, ldo, hard, dtype):
    g = _gen(B * 1000 + N * 100 + HW)
    o = torch.randn(B * N, HW, ldo, generator=g)
    if hard:
        o[..., 3] = o[..., 3] * 8 + 100
    o = _q(o, dtype)
    dr = torch.randn(B, HW, 4, generator=g)                  # (channel 3 of drecon is not read)
    o64 = o.double().requires_grad_(True)
    v = o64.view(B, N, HW, ldo)
    m = torch.softmax(v[..., 3], dim=1)                      # over slots
    recon = (m.unsqueeze(-1) * v[..., :3]).sum(1)            # [B, HW, 3]
    recon.backward(dr[..., :3].double())
    return o, dr, recon.detach(), m.detach(), o64.grad


def _check_sa(case, dims, dtype, recon, masks, dout, tag):
    B, N, HW, ldo = dims
    o, dr, recon64, m64, do64 = case
    bf = dtype == torch.bfloat16
    # recon and masks are fp32 whatever the storage of o: no bf16 term
    _check_expf('sa_combine', tag + ' masks', masks, m64)
    _check_expf('sa_combine', tag + ' recon', recon[..., :3], recon64)
    assert bool((recon[..., 3] == 0).all())
    d = dout.view(B, N, HW, ldo)
    g64 = do64.view(B, N, HW, ldo)
    drb = dr.view(B, 1, HW, 4)[..., :3].expand(B, N, HW, 3)
    _check_expf('sa_combine_bwd', tag + ' drgb', d[..., :3], g64[..., :3], dy=drb, bf16=bf)
    # alpha: m_s * sum_c (rgb_sc - recon_c) * drecon_c; its |dy| is the size of the products that meet in the sum
    sc = (o.view(B, N, HW, ldo)[..., :3].abs().amax(1) * dr[..., :3].abs()).sum(-1)          # [B, HW]
    _check_expf('sa_combine_bwd', tag + ' dalpha', d[..., 3], g64[..., 3], dy=sc.view(B, 1, HW), bf16=bf)
    assert bool((d[..., 4:] == 0).all()), 'pad channels of dout must be zeroed'
    if N == 1:
        assert bool((masks == 1).all()) and bool((d[..., 3] == 0).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('case', SA_CASES, ids=lambda c: 'x'.join(str(int(v)) for v in c))
def test_sa_combine_and_bwd(case, dtype):
    """masks = softmax over slots of the alpha logit, recon = sum of rgb * mask, and the backward (which reads the
    forward's masks) against fp64 autograd.  expf bound (dout in bf16: + half an ulp); dout[..., 4:] == 0 exactly;
    with one slot the masks are exactly 1 and the alpha gradient exactly 0."""
    B, N, HW, ldo, hard = case
    ref = _sa_case(B, N, HW, ldo, hard, dtype)
    od, drd = _dev(ref[0], dtype), _dev(ref[1])
    recon, masks = _poison((B, HW, 4), torch.float32), _poison((B, N, HW), torch.float32)
    dout = _poison((B * N, HW, ldo), dtype)
    _call('sdmi_sa_combine', o=od.data_ptr(), recon=recon.data_ptr(), masks=masks.data_ptr(), dtype=_dt(dtype),
          B=B, N=N, HW=HW, ldo=ldo)
    _call('sdmi_sa_combine_bwd', o=od.data_ptr(), masks=masks.data_ptr(), drecon=drd.data_ptr(),
          dout=dout.data_ptr(), dtype=_dt(dtype), B=B, N=N, HW=HW, ldo=ldo)
    _check_sa(ref, (B, N, HW, ldo), dtype, recon, masks, dout, f'{B}x{N}x{HW}x{ldo} {_ID[dtype]}')


def test_sa_combine_function_wiring():
    """kern.SaCombineFn through torch.autograd (o as [B*N, H, W, ld]): same bounds."""
    from slotdiffusion_amd.kern import SaCombineFn
    B, N, HW, ldo = 3, 11, 63, 8
    ref = _sa_case(B, N, HW, ldo, True, torch.float32)
    od = _dev(ref[0]).view(B * N, 7, 9, ldo).requires_grad_(True)
    recon, masks = SaCombineFn.apply(od, B, N)
    recon.backward(_dev(ref[1]).view(B, 7, 9, 4))
    _check_sa(ref, (B, N, HW, ldo), torch.float32, recon.detach().view(B, HW, 4), masks, od.grad.view(B * N, HW, ldo),
              'SaCombineFn')


# ---- softmax backward ----------------------------------------------------------------------------------
SM_SHAPES = [(3, 1, 1), (5, 7, 8), (4, 255, 256), (4, 257, 264), (2, 1000, 1000)]


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('scale', [1.0, 0.125])
@pytest.mark.parametrize('shape', SM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_softmax_rows_bwd(shape, scale, dtype):
    """ds = scale * p * (dp - sum p dp) in place, one workgroup of 256 per row: one column, ragged rows, exactly one
    trip short of two (255), two trips with ld > cols (257 / 264), four trips.  Derived bound: the dot is a fp32 sum
    of `cols` terms, three roundings around it; bf16: + half an ulp.  The row padding and p are left untouched."""
    rows, cols, ld = shape
    g = _gen(rows * 10007 + cols)
    p = _q(torch.softmax(torch.randn(rows, cols, generator=g).double() * 4, -1).float(), dtype)
    dp = _q(torch.randn(rows, cols, generator=g), dtype)
    P, D = _poison((rows, ld), dtype), _poison((rows, ld), dtype)
    P[:, :cols], D[:, :cols] = _dev(p, dtype), _dev(dp, dtype)
    P0 = P.clone()
    _call('sdmi_softmax_rows_bwd', p=P.data_ptr(), dp=D.data_ptr(), dtype=_dt(dtype), rows=rows, cols=cols, ld=ld,
          scale=scale)
    p64, dp64 = p.double(), dp.double()
    terms = p64 * dp64
    exact = scale * p64 * (dp64 - terms.sum(-1, keepdim=True))
    bound = (scale * p64).abs() * (cols * U * terms.abs().sum(-1, keepdim=True)) + 4 * U * exact.abs()
    _check_derived(f'softmax_rows_bwd {shape} x{scale} {_ID[dtype]}', D[:, :cols], exact, bound,
                   bf16=dtype == torch.bfloat16)
    assert _same_bits(D[:, cols:], _poison((rows, ld - cols), dtype)), 'row padding of dp was written'
    assert _same_bits(P, P0)


# ---- straight-through quantizer backward ---------------------------------------------------------------
VQ_SHAPES = [(300, 64, 3, 4), (1000, 2, 3, 8), (CAP_ROWS + 77, 64, 3, 4)]    # ragged / two codes / grid-stride wrap
BETA = 0.25


@functools.lru_cache(None)
def _vq_inputs(R, codes, dim, ldz):
    g = _gen(R + codes)
    code = torch.randn(codes, dim, generator=g)
    used = torch.tensor([c for c in range(codes) if codes <= 2 or c % 8 != 5])
    idx = used[torch.randint(0, len(used), (R,), generator=g)]
    z = torch.randn(R, ldz, generator=g)                                 # (pad columns: garbage the kernel must not read)
    zq = torch.full((R, ldz), 7.0)
    zq[:, :dim] = code[idx]
    a = torch.randn(R, ldz, generator=g)
    init = torch.randn(codes + 2, dim, generator=g) * (8.0 * BETA / (R * dim))   # the size of a few terms
    return code, used, idx, z, zq, a, init


def _vq_reference(R, codes, dim, ldz, with_dzq, gval):
    code, used, idx, z, zq, a, init = _vq_inputs(R, codes, dim, ldz)
    z64 = z.double().requires_grad_(True)
    c64 = code.double().requires_grad_(True)
    z3, q3 = z64[:, :dim], c64[idx]
    ql = ((q3.detach() - z3) ** 2).mean() + BETA * ((q3 - z3.detach()) ** 2).mean()
    st = z3 + (q3 - z3).detach()                                         # straight-through estimator
    loss = gval * ql + ((st * a[:, :dim].double()).sum() if with_dzq else 0.0)
    loss.backward()
    n = R * dim
    diff = (z[:, :dim].double() - zq[:, :dim].double())
    t = gval * 2.0 / n * diff
    dzq = a[:, :dim].double() if with_dzq else torch.zeros_like(t)
    dz64 = z64.grad[:, :dim]
    # dz = dzq + t: a two-term sum whose second term carries three roundings of its own
    b_dz = 2 * U * (dzq.abs() + t.abs()) + 4 * U * dz64.abs()
    dc64 = init[1:-1].double() + c64.grad
    tc = (BETA * t).abs()
    sumabs = init[1:-1].double().abs().index_add(0, idx, tc)
    n_terms = (torch.bincount(idx, minlength=codes) + 1).double().unsqueeze(1)
    b_dc = n_terms * U * sumabs + 4 * U * dc64.abs()
    return dz64, b_dz, dc64, b_dc


@pytest.mark.parametrize('with_g', [False, True], ids=['g_null', 'g_1.3'])
@pytest.mark.parametrize('with_dzq', [True, False], ids=['dzq', 'dzq_null'])
@pytest.mark.parametrize('shape', VQ_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_vq_bwd(shape, with_dzq, with_g):
    """dz = dzq + g 2/n (z - zq), dcode[idx] += g 2 beta/n (zq - z) by fp32 atomics, against fp64 autograd of the
    straight-through loss.  Derived bounds: dz a two-term sum; dcode a sum of (rows on the code + 1) terms in
    arbitrary order onto the value it held.  Unused codes and the rows around the table keep their bits; the pad
    columns of dz are exactly 0."""
    R, codes, dim, ldz = shape
    code, used, idx, z, zq, a, init = _vq_inputs(*shape)
    gt = torch.tensor([1.3], dtype=torch.float32)
    dz64, b_dz, dc64, b_dc = _vq_reference(R, codes, dim, ldz, with_dzq, float(gt) if with_g else 1.0)
    zd, zqd, ad, idxd = _dev(z), _dev(zq), _dev(a), _dev(idx)
    gd = _dev(gt)
    dz = _poison((R, ldz), torch.float32)
    dcode = _dev(init)                                     # row 0 and row codes + 1 guard the table
    _call('sdmi_vq_bwd', z=zd.data_ptr(), zq=zqd.data_ptr(), dzq=ad.data_ptr() if with_dzq else 0, dz=dz.data_ptr(),
          dcode=dcode[1:].data_ptr(), idx=idxd.data_ptr(), g=gd.data_ptr() if with_g else 0, R=R, dim=dim, ldz=ldz,
          beta=BETA)
    tag = f'vq_bwd {shape} dzq={with_dzq} g={with_g}'
    _check_derived(tag + ' dz', dz[:, :dim], dz64, b_dz)
    assert bool((dz[:, dim:] == 0).all()), 'pad columns of dz'
    _check_derived(tag + ' dcode', dcode[1:-1], dc64, b_dc)
    unused = torch.ones(codes + 2, dtype=torch.bool)
    unused[1 + used] = False
    assert _same_bits(dcode.cpu()[unused], init[unused]), 'a code no row maps to (or a guard row) was written'


def test_vq_function_wiring():
    """kern.VqFn (nearest code + straight-through backward) through torch.autograd against the fp64 gradients of
    w1 * sum(zq * a) + w2 * quant_loss, as in test_vae_train_kernels; derived bounds of test_vq_bwd."""
    from slotdiffusion_amd.kern import VqFn
    g = _gen(5)
    R, codes, w1, w2 = 300, 64, 0.7, 1.3
    code = torch.randn(codes, 3, generator=g)
    z = F.pad(torch.randn(R, 3, generator=g), (0, 1))
    a = torch.randn(R, 4, generator=g)
    z64, c64 = z.double().requires_grad_(True), code.double().requires_grad_(True)
    z3 = z64[:, :3]
    idx = ((z3 ** 2).sum(1, keepdim=True) + (c64 ** 2).sum(1) - 2 * z3 @ c64.t()).argmin(1)
    q3 = c64[idx]
    ql = ((q3.detach() - z3) ** 2).mean() + BETA * ((q3 - z3.detach()) ** 2).mean()
    st = z3 + (q3 - z3).detach()
    ((st * a[:, :3].double()).sum() * w1 + w2 * ql).backward()
    zd = _dev(z).requires_grad_(True)
    dcode = torch.zeros(codes, 3, device=DEV)
    anchor = torch.zeros(1, device=DEV, requires_grad=True)
    zq_d, ql_d, idx_d = VqFn.apply(zd, anchor, _dev(code), dcode, BETA)
    assert torch.equal(idx_d.cpu(), idx)
    # zq leaves the kernel in its straight-through form z + (code - z): two fp32 roundings away from the code
    _check_derived('VqFn zq', zq_d[:, :3], code[idx].double(), 2 * U * (z[:, :3].abs() + code[idx].abs()).double())
    assert bool((zq_d[:, 3] == 0).all())
    # quant_loss = (1 + beta) * mean((zq - z)^2) over the 3 used channels: a sum of R * 3 squares
    sq = (1 + BETA) * (code[idx].double() - z[:, :3].double()) ** 2 / (R * 3)
    _check_derived('VqFn quant_loss', ql_d.reshape(1), ql.detach().reshape(1),
                   R * 3 * U * sq.sum().reshape(1) + 4 * U * ql.detach().abs().reshape(1))
    ((zq_d * _dev(a)).sum() * w1 + w2 * ql_d).backward()
    gval = float(torch.tensor(w2, dtype=torch.float32))
    t = gval * 2.0 / (R * 3) * (z[:, :3].double() - code[idx].double())
    dzq = w1 * a[:, :3].double()
    # (w1 and w2 are fp32 on the device: one more rounding on each term than the bare kernel's)
    _check_derived('VqFn dz', zd.grad[:, :3], z64.grad[:, :3], 3 * U * (dzq.abs() + t.abs()) + 4 * U * z64.grad[:, :3].abs())
    assert bool((zd.grad[:, 3] == 0).all())
    n_terms = (torch.bincount(idx, minlength=codes) + 1).double().unsqueeze(1)
    sumabs = torch.zeros(codes, 3, dtype=torch.float64).index_add(0, idx, (BETA * t).abs())
    _check_derived('VqFn dcode', dcode, c64.grad, n_terms * U * sumabs + 4 * U * c64.grad.abs())


# ---- bit-exact streaming kernels -----------------------------------------------------------------------
def _pool_shapes(dtype):
    vec = 8 if dtype == torch.bfloat16 else 4
    side = 128 if vec == 4 else 179          # side * side * (264 / vec) vectors > 4096 * 256: second grid-stride trip
    return [(1, 1, 1, 8), (2, 3, 5, 24), (1, 64, 64, 264), (1, side, side, 264)]


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('which', range(4), ids=['1px', 'ragged', '64x64x264', 'wrap'])
def test_pool2x2_sum(which, dtype):
    """Bit-exact: fp32 (a0 + a1) + (a2 + a3) in that order, rounded once to bf16 for bf16 storage."""
    B, H, W, C = _pool_shapes(dtype)[which]
    assert which != 3 or B * H * W * (C // (8 if dtype == torch.bfloat16 else 4)) > CAP
    x = _q(torch.randn(B, 2 * H, 2 * W, C, generator=_gen(H * W + C)), dtype)
    xd = _dev(x, dtype)
    y = _poison((B, H, W, C), dtype)
    _call('sdmi_pool2x2_sum', x=xd.data_ptr(), y=y.data_ptr(), dtype=_dt(dtype), B=B, H=H, W=W, C=C)
    ref = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2]) + (x[:, 1::2, 0::2] + x[:, 1::2, 1::2])
    assert _same_bits(y, ref.to(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('n', [1, 3, 8, 4099, CAP * 4 + 5, CAP * 8 + 13])
def test_add(n, dtype):
    """Bit-exact: one fp32 add, then the rounding to bf16.  n below one vector, a vector plus a tail, and more
    vectors than the grid has threads (4 per vector in fp32, 8 in bf16) with a scalar tail."""
    g = _gen(n)
    a, b = _q(torch.randn(n, generator=g), dtype), _q(torch.randn(n, generator=g), dtype)
    ad, bd = _dev(a, dtype), _dev(b, dtype)
    y = _poison((n + 8,), dtype)
    _call('sdmi_add', x=ad.data_ptr(), z=bd.data_ptr(), y=y.data_ptr(), dtype=_dt(dtype), n=n)
    assert _same_bits(y[:n], (a + b).to(dtype))
    assert _same_bits(y[n:], _poison((8,), dtype)), 'wrote past n'


def test_add_function_wiring():
    """kern.AddFn: y bit-exact, both gradients are dy itself."""
    from slotdiffusion_amd.kern import AddFn
    g = _gen(4099)
    a, b, dy = (torch.randn(4099, generator=g) for _ in range(3))
    ad, bd = _dev(a).requires_grad_(True), _dev(b).requires_grad_(True)
    y = AddFn.apply(ad, bd)
    y.backward(_dev(dy))
    assert _same_bits(y, a + b) and _same_bits(ad.grad, dy) and _same_bits(bd.grad, dy)


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('B,per', [(1, 8), (3, 10 * 24)])
def test_add_pos(B, per, dtype):
    """Bit-exact: x[b] + pos (pos fp32) in fp32, then the rounding to bf16."""
    g = _gen(B + per)
    x, pos = _q(torch.randn(B, per, generator=g), dtype), torch.randn(per, generator=g)
    xd, pd = _dev(x, dtype), _dev(pos)
    y = _poison((B, per), dtype)
    _call('sdmi_add_pos', x=xd.data_ptr(), pos=pd.data_ptr(), y=y.data_ptr(), dtype=_dt(dtype), B=B, per=per)
    assert _same_bits(y, (x + pos).to(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=_ID.get)
@pytest.mark.parametrize('which', range(3), ids=['3x8+16', '1031x24+40', 'wrap'])
def test_split_and_concat_channels(which, dtype):
    """Bit-exact copies: split_channels of y, and concat_channels of the halves back to y.  The last shape has more
    vectors than the grid has threads."""
    vec = 8 if dtype == torch.bfloat16 else 4
    rows, Ca, Cb = [(3, 8, 16), (1031, 24, 40), (CAP // (64 // vec) + 1, 32, 32)][which]
    assert which != 2 or rows * ((Ca + Cb) // vec) > CAP
    y = _q(torch.randn(rows, Ca + Cb, generator=_gen(rows + Ca)), dtype)
    yd = _dev(y, dtype)
    a, b = _poison((rows, Ca), dtype), _poison((rows, Cb), dtype)
    _call('sdmi_split_channels', y=yd.data_ptr(), a=a.data_ptr(), b=b.data_ptr(), dtype=_dt(dtype), rows=rows,
          Ca=Ca, Cb=Cb)
    assert _same_bits(a, y[:, :Ca].to(dtype)) and _same_bits(b, y[:, Ca:].to(dtype))
    back = _poison((rows, Ca + Cb), dtype)
    _call('sdmi_concat_channels', a=a.data_ptr(), b=b.data_ptr(), y=back.data_ptr(), dtype=_dt(dtype), rows=rows,
          Ca=Ca, Cb=Cb)
    assert _same_bits(back, y.to(dtype))


def _layout(sizes_offs, guard, align):
    """Place segments in one buffer: each starts at a multiple of `align` plus its offset, with at least `guard`
    untouched units before it and after the last.  -> (starts, total)."""
    starts, cur = [], 0
    for size, off in sizes_offs:
        s = (cur + guard + align - 1) // align * align + off
        starts.append(s)
        cur = s + size
    return starts, cur + guard + align


def _items(struct, rows):
    arr = (_L().CSTRUCT[struct] * max(1, len(rows)))()
    for it, row in zip(arr, rows):
        for (name, _), v in zip(_L().STRUCTS[struct], row):
            setattr(it, name, v)
    return arr


def test_scatter_add_one_launch_of_32_segments():
    """dst_i += src_i, bit-exact fp32, the whole destination buffer compared (so the guard words on both sides of
    every segment are unchanged).  Counts 0, 1, 3 (< one vector), 4, 5, 1023 and 256 * 256 * 4 + 7 (second trip of
    the vector loop, scalar tail), each with both pointers 16-byte aligned, src / dst / both offset by one float
    (the scalar branch)."""
    counts = [0, 1, 3, 4, 5, 1023, 256 * 256 * 4 + 7]
    assert max(counts) // 4 > 256 * 256 and max(counts) % 4
    segs = [(c, so, do) for c in counts for so, do in ((0, 0), (1, 0), (0, 1), (1, 1))]
    segs += [(7, 0, 0), (8, 0, 0), (1024, 0, 0), (4099, 0, 0)]
    assert len(segs) == 32
    s_start, s_total = _layout([(c, so) for c, so, _ in segs], 4, 4)
    d_start, d_total = _layout([(c, do) for c, _, do in segs], 4, 4)
    g = _gen(32)
    src, dst = torch.randn(s_total, generator=g), torch.randn(d_total, generator=g)
    srcd, dstd = _dev(src), _dev(dst)
    assert srcd.data_ptr() % 16 == 0 and dstd.data_ptr() % 16 == 0
    want = dst.clone()
    rows = []
    for (c, _, _), s0, d0 in zip(segs, s_start, d_start):
        want[d0:d0 + c] = dst[d0:d0 + c] + src[s0:s0 + c]
        rows.append((srcd.data_ptr() + 4 * s0, dstd.data_ptr() + 4 * d0, c))
    arr = _items('SdmiScatterItem', rows)
    _call('sdmi_scatter_add', items=ctypes.addressof(arr), n=len(rows))
    assert _same_bits(dstd, want)
    assert _same_bits(srcd, src)


def test_copy_group_one_launch():
    """Byte-exact copies, the whole destination buffer compared (guard bytes around each destination unchanged):
    0, 1, 15, 16, 17, 4099 and 256 * 256 * 16 + 25 bytes (second trip of the vector loop, byte tail), each aligned
    and with src / dst offset by 2 bytes (the byte branch)."""
    sizes = [0, 1, 15, 16, 17, 4099, 256 * 256 * 16 + 25]
    assert max(sizes) // 16 > 256 * 256 and max(sizes) % 16            # more vectors than the grid has threads, and a tail
    items = [(n, so, do) for n in sizes for so, do in ((0, 0), (2, 0), (0, 2))]
    s_start, s_total = _layout([(n, so) for n, so, _ in items], 16, 16)
    d_start, d_total = _layout([(n, do) for n, _, do in items], 16, 16)
    g = _gen(21)
    src = torch.randint(0, 256, (s_total,), generator=g, dtype=torch.uint8)
    dst = torch.randint(0, 256, (d_total,), generator=g, dtype=torch.uint8)
    srcd, dstd = _dev(src), _dev(dst)
    assert srcd.data_ptr() % 16 == 0 and dstd.data_ptr() % 16 == 0
    want = dst.clone()
    rows = []
    for (n, _, _), s0, d0 in zip(items, s_start, d_start):
        want[d0:d0 + n] = src[s0:s0 + n]
        rows.append((srcd.data_ptr() + s0, dstd.data_ptr() + d0, n))
    arr = _items('SdmiCopyItem', rows)
    _call('sdmi_copy_group', items=ctypes.addressof(arr), n=len(rows))
    assert _same_bits(dstd, want)
    assert _same_bits(srcd, src)


# ---- dropout -------------------------------------------------------------------------------------------
def _share_ok(share, q, n):
    return abs(share - q) <= 5.0 * math.sqrt(q * (1.0 - q) / n)


@pytest.mark.parametrize('p', [0.0, 0.1, 0.5])
def test_dropout_standalone(p):
    """The stand-alone inverted dropout (the backward re-runs it to regenerate the mask), n = 4096 * 256 + 257.
    Bit-exact: every output is 0 or x * inv with inv = fp32 1 / (1 - p), rounded once for bf16; p = 0 is the
    identity; the mask is the same for both storages, for a repeated call and for seed_dev NULL or pointing at 0.
    Derived (binomial, 5 sigma at each sample's own n): the kept share overall, of even and odd indices and of
    the first and second grid-stride trips is 1 - p; masks of another seed, or of *seed_dev + 1, agree with the
    first on a share (1 - p)^2 + p^2."""
    n = CAP + 257
    g = _gen(17)
    x = (torch.rand(n, generator=g) + 0.5) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    x = _q(x, torch.bfloat16)                                  # one input for both storages
    pf = torch.tensor(p, dtype=torch.float32)
    inv = torch.tensor(1.0) / (torch.tensor(1.0) - pf)
    seed = 1234

    def run(dtype, seed, dev_word):
        xd = _dev(x, dtype)
        y = _poison((n,), dtype)
        sd = torch.tensor([dev_word], dtype=torch.int64, device=DEV) if dev_word is not None else None
        _call('sdmi_dropout', x=xd.data_ptr(), y=y.data_ptr(), dtype=_dt(dtype), n=n, p=float(pf), seed=seed,
              seed_dev=sd.data_ptr() if sd is not None else 0)
        return y.cpu()

    y32 = run(torch.float32, seed, 7)
    keep = y32 != 0
    want = torch.where(keep, x * inv, torch.zeros_like(x))
    assert _same_bits(y32, want)
    y16 = run(torch.bfloat16, seed, 7)
    assert _same_bits(y16, want.to(torch.bfloat16))             # same mask, x * inv rounded once
    assert _same_bits(run(torch.float32, seed, 7), y32)
    assert _same_bits(run(torch.float32, seed, None), run(torch.float32, seed, 0))
    if p == 0.0:
        assert _same_bits(y32, x)
    k = keep.double()
    for what, part in (('all', k), ('even', k[0::2]), ('odd', k[1::2]), ('trip 1', k[:CAP]), ('trip 2', k[CAP:])):
        assert _share_ok(float(part.mean()), 1.0 - p, part.numel()), (what, float(part.mean()))
    q = (1.0 - p) ** 2 + p ** 2
    for what, other in (('seed + 1', run(torch.float32, seed + 1, 7)), ('*seed_dev + 1', run(torch.float32, seed, 8))):
        agree = float(((other != 0) == keep).double().mean())
        assert _share_ok(agree, q, n), (what, agree)
        assert p == 0.0 or not torch.equal(other != 0, keep), what


# ---- refusals ------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    """Each call must report an error through the ABI and launch nothing: the output buffer keeps its poison."""
    Err = _L().SdmiError
    bf, f32 = torch.bfloat16, torch.float32
    x16, o16 = torch.ones(4 * 24, dtype=bf, device=DEV), _poison((4 * 24,), bf)
    x32, o32 = torch.ones(4 * 24, device=DEV), _poison((4 * 24,), f32)
    idx = torch.zeros(4, dtype=torch.int64, device=DEV)
    rows33 = [(x32.data_ptr(), o32.data_ptr(), 4)] * 33
    sc, cp = _items('SdmiScatterItem', rows33), _items('SdmiCopyItem', rows33)
    bad = [
        ('sdmi_geglu', dict(h=x16.data_ptr(), y=o16.data_ptr(), dtype=_dt(bf), rows=4, C=12)),
        ('sdmi_geglu_bwd', dict(h=x16.data_ptr(), dy=x16.data_ptr(), dh=o16.data_ptr(), dtype=_dt(bf), rows=4, C=12)),
        ('sdmi_split_channels', dict(y=x16.data_ptr(), a=o16.data_ptr(), b=o16[48:].data_ptr(), dtype=_dt(bf),
                                     rows=4, Ca=12, Cb=12)),
        ('sdmi_pool2x2_sum', dict(x=x16.data_ptr(), y=o16.data_ptr(), dtype=_dt(bf), B=1, H=1, W=1, C=12)),
        ('sdmi_scatter_add', dict(items=ctypes.addressof(sc), n=0)),
        ('sdmi_scatter_add', dict(items=ctypes.addressof(sc), n=33)),
        ('sdmi_copy_group', dict(items=ctypes.addressof(cp), n=0)),
        ('sdmi_copy_group', dict(items=ctypes.addressof(cp), n=33)),
        ('sdmi_dropout', dict(x=x32.data_ptr(), y=o32.data_ptr(), dtype=_dt(f32), n=96, p=1.0, seed=1)),
        ('sdmi_vq_bwd', dict(z=x32.data_ptr(), zq=x32.data_ptr(), dz=o32.data_ptr(), dcode=o32.data_ptr(),
                             idx=idx.data_ptr(), R=4, dim=3, ldz=2, beta=BETA)),
    ]
    for fname, kw in bad:
        with pytest.raises(Err):
            _call(fname, **kw)
        assert len(_L().lib().sdmi_last_error()) > 0, fname
    torch.cuda.synchronize()
    assert _same_bits(o16, _poison((4 * 24,), bf)) and _same_bits(o32, _poison((4 * 24,), f32))
