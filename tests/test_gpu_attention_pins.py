"""sdmi_attention and sdmi_attention_bwd, called through the C ABI in the packed layouts production uses and pinned,
element by element, to a float64 CPU reference computed from the tensors the kernel read (rounded to the storage
dtype first).  Forward: S = scale q k^T, P = softmax(S), O = P v, lse = logsumexp(S).  Backward: the header formulas
of attention_bwd.hip on q, k, v, dout and the `out` and `lse` the forward kernel stored (downloaded), so the backward
kernels are judged on their own:  P = exp(S - lse), D = dout . out, dV = P^T dout, dS = P o (dout v^T - D),
dQ = scale dS k, dK = scale dS^T q.

Every tolerance is one of three kinds (the discipline of test_gpu_bwd_helpers.py), and each test says which:

  bit-exact   the output bits are predictable: planted keys (out = one row of v), poison that must survive, zeros.
  derived     a per-element bound computed in float64 from the operation itself, no norms:
                fp32 sum of n terms             n U sum|terms| + 4 U |exact|            (U = 2^-24)
                bf16 storage of a result        BF (|exact| + the bound before it)       (BF = 2^-8, half an ulp)
                one bf16 rounding inside the matrix-core kernels, coefficient 1 each, listed below
  expf        the hardware exponential.  A kernel evaluates P_ij with __expf (v_exp_f32) on an fp32 argument s_ij - m_i
              (m_i the running row maximum; lse_i in the backward) that c = HD + 3 fp32 operations formed: the
              HD-term dot product (products included) and the scale (q * scale before the dot, s * scale after it,
              or scale * log2(e) in the matrix-core forward) err relative to A_ij = scale sum_d |q_id k_jd|, the
              subtraction and the multiplication by log2(e) in front of v_exp_f32 relative to the argument, whose
              magnitude is at most |S_ij| + |m_i|:
                  |P^_ij - P_ij| <= P_ij e_ij + 2^-126,    e_ij = r + (HD + 1) U A_ij + 2 U (|S_ij| + |m_i|).
              (A_ij and not |S_ij| under the dot product: where the products cancel, |S_ij| says nothing about
              their rounding.  With one key lse is that dot product itself, and fp32 arithmetic done honestly on
              the CPU missed (HD + 3) U (|S_ij| + |m_i|) there.)  Everything but r is derived; r is the measured
              relative error of the instruction itself; 2^-126 is fp32 underflow (a flushed P_ij, and likewise one
              per product of a sum and one for the stored result).  In the forward a common factor of a row of P
              cancels in P v / sum P (the running maximum, with its own rounding, and every rescaling factor alpha
              are such factors), so
                  |O^ - O|_id <= sum_j P_ij e_ij |v_jd| + |O_id| sum_j P_ij e_ij + the accumulation bound;
              the accumulations have n = Skv + ceil(Skv / 4) terms (one rescaling multiply per four-key step at
              most; once per 32 keys in the matrix-core kernels).
              lse_i = m_i + log(l_i):  sum_j P_ij (e_ij - r)  +  n U (the sum l_i)  +  4 U (|m_i| + |lse_i| +
              |lse_i - m_i|) (the roundings of the logarithm's result, of the exp2-domain conversion and of the
              final add)  +  r (a relative error of l_i is an absolute one of lse_i)  +  a, the measured absolute
              error of the logarithm (v_log_f32).  The backward kernels take no logarithm: their a is 0.

EXPL below holds (r, a) per kernel, starting at the precedent's (4e-7, 2e-7), with the largest value any case of this
file needed on an MI355X beside each; r <= 4e-6 and a <= 1e-6 are asserted at import.  These, U, BF, 2^-126 and the
counted c and n are the only literals.

Roundings of the matrix-core kernels (each adds one term, coefficient 1, on top of the fp32 terms above):
  attn_fwd_mfma_kernel   `pack_bf16x2(s[8 * mm + 0], ...)`: the un-normalised P of a key block becomes the bf16 B
                         operand of V^T P^T               ->  BF sum_j P_ij |v_jd|      (the row sum uses the
                         un-rounded P; alpha scales rounded values without changing their relative error)
                         `pack_bf16x2(o[jd][4 * j] * inv, ...)`: the output           ->  BF |O_id| (storage)
  attn_bwd_dkv_mfma_body `bpack8(pr + 8 * mm)`: P as the B operand of dO^T P            ->  BF sum_i P_ij |dout_id|
                         `bpack8(ds + 8 * mm)`: dS as the B operand of Q^T dS           ->  scale BF sum_i |dS_ij| |q_id|
                         `store_col(... dk / dv ...)`                                   ->  BF |dK|, BF |dV| (storage)
  attn_bwd_dq_mfma_body  `bpack8(ds + 8 * mm)`: dS as the B operand of K^T dS^T         ->  scale BF sum_j |dS_ij| |k_jd|
                         `store_col(... dq ...)`                                        ->  BF |dQ| (storage)
  D_i = dout_i . out_i is an fp32 dot of bf16 values on both sides (the reference uses the same stored `out`): it
  and dout_i . v_j add HD U (sum_d |dout_id out_id| + sum_d |dout_id v_jd|) to dout v^T - D, carried through P_ij and
  |k_jd| or |q_id| like every other term of dS.

Geometry of every case: B = 2 and 3 heads (batch stride, head offset, the [B][heads][Sq] layout of lse), C = 3 HD.
Self-attention (Sq == Skv) reads q | k | v as column slices of one [B S, 3C] tensor and writes dq | dk | dv into one
poisoned [B S, 3C] tensor; otherwise q is [B Sq, C], k | v slices of [B Skv, 2C], dk | dv slices of a poisoned
[B Skv, 2C].  out and dout have a pitch of C + 8 (bf16) or C + 4 (fp32) elements with poison in the gap, and every
buffer ends in one poisoned guard row.  After each call every element of the result is checked against its bound and
every poison element (gaps, guard rows) must be bit-identical; the inputs must be unchanged.  (ldk == ldv in both
layouts; test_four_different_pitches adds one case per kernel where all four pitches differ.)

Not reachable through the ABI, hence NOT covered here: attn_fwd_kernel<bf16_t, 32> and launch_attn_bwd<bf16_t, 32>
(its three kernels at bf16 / head size 32) -- bf16 at head size 32 always takes the matrix-core kernels."""
import math

import pytest
import torch

from tests.test_gpu_bwd_helpers import (BF, DEV, U, _call, _dt, _end_the_session_on_a_gpu_fault,  # noqa: F401
                                        _gen, _L, _poison, _q, _same_bits, _worst)

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
_ID = {F32: 'fp32', BF16: 'bf16'}
BATCH, HEADS = 2, 3
TINY = 2.0 ** -126          # smallest normal fp32 / bf16: what a flushed value loses at most

# (r, a) of the expf bound per kernel.  "needs" = the largest r (from out / dq / dk / dv) and a (from lse) any case of
# this file needed on an MI355X with every derived term in place, and "uses" = the largest share of its bound any
# element reached there.  r and a 0: the derived terms alone covered every element, so no constant was raised; the
# shares near 1 are bf16 storage roundings that land on half an ulp.
EXPL = {
    'fwd/valu': (4e-7, 2e-7),            # attn_fwd_kernel<float, 32|48>, <bf16_t, 48>: needs r 0, a 0; uses 0.98
    'fwd/mfma32': (4e-7, 2e-7),          # attn_fwd_mfma_kernel<32, 512>: needs r 0, a 0; uses 0.84
    'fwd/mfma64': (4e-7, 2e-7),          # attn_fwd_mfma_kernel<64, 256>: needs r 0, a 0; uses 0.78
    'bwd/valu_dq': (4e-7, 0.0),          # attn_bwd_dq_kernel: needs r 0; uses 0.98
    'bwd/valu_dkv': (4e-7, 0.0),         # attn_bwd_dkv_kernel: needs r 0; uses 0.99
    'bwd/valu_dkv_small': (4e-7, 0.0),   # attn_bwd_dkv_small_kernel (fp32, head size 32, Skv <= 16): needs r 0; uses 0.025
    'bwd/mfma_dq': (4e-7, 0.0),          # attn_bwd_mfma_kernel, dQ body: needs r 0; uses 0.88
    'bwd/mfma_dkv': (4e-7, 0.0),         # attn_bwd_mfma_kernel, dKV body: needs r 0; uses 0.94
}
assert all(r <= 4e-6 and a <= 1e-6 for r, a in EXPL.values())
# largest r ('<key> r') and a ('<key> a') needed so far in this session, and the largest share of its bound any element
# used ('<key> err/bound'), for a measuring run to print
NEED = {}


# ---- plumbing ------------------------------------------------------------------------------------------
def _scale(hd):
    """head_dim^-0.5 as the fp32 value the ABI carries."""
    return float(torch.tensor(hd ** -0.5, dtype=torch.float32))


def _is_mfma(dtype, hd):
    return dtype == BF16 and hd in (32, 64)


def _keys(dtype, hd, Skv):
    """EXPL rows of the forward, dQ and dK/dV kernels that serve this case."""
    if _is_mfma(dtype, hd):
        return f'fwd/mfma{hd}', 'bwd/mfma_dq', 'bwd/mfma_dkv'
    return 'fwd/valu', 'bwd/valu_dq', 'bwd/valu_dkv_small' if hd == 32 and Skv <= 16 else 'bwd/valu_dkv'


def _split(t, hd):
    """[B, S, heads * hd] -> float64 [B, heads, S, hd]."""
    B, S, C = t.shape
    return t.double().view(B, S, C // hd, hd).permute(0, 2, 1, 3)


def _merge(t):
    """[B, heads, S, hd] -> [B, S, heads * hd]."""
    B, H, S, hd = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, S, H * hd)


def _buf(rows, cols, dtype, fill=None):
    """Poisoned [rows + 1, cols] device buffer (the last row is the guard), `fill` [rows, <= cols] in its first columns."""
    b = _poison((rows + 1, cols), dtype)
    if fill is not None:
        b[:rows, :fill.shape[1]] = fill.to(dtype).to(DEV)
    return b


def _only_poison_outside(buf, rows, cols):
    """Every element of `buf` outside [:rows, :cols] still holds the poison, bit for bit."""
    t = buf.clone()
    t[:rows, :cols] = _poison((rows, cols), buf.dtype)
    return _same_bits(t, _poison(tuple(buf.shape), buf.dtype))


def _pack(dtype, Sq, Skv, C, layout, q=None, k=None, v=None):
    """Buffers for q | k | v (or, without data, poisoned ones for dq | dk | dv) in `layout`.
    -> (views of q, k, v with the guard row, their pitches, [(buffer, rows, used columns)])."""
    B = BATCH
    flat = lambda t, S: None if t is None else t.reshape(B * S, C)
    cat = lambda *ts: None if ts[0] is None else torch.cat(ts, -1)
    vec = 8 if dtype == BF16 else 4
    if layout == 'self':                       # one [B S, 3C] tensor
        t = _buf(B * Sq, 3 * C, dtype, cat(flat(q, Sq), flat(k, Skv), flat(v, Skv)))
        return (t[:, :C], t[:, C:2 * C], t[:, 2 * C:]), (3 * C,) * 3, [(t, B * Sq, 3 * C)]
    if layout == 'cross':                      # q [B Sq, C], k | v in [B Skv, 2C]
        tq, tkv = _buf(B * Sq, C, dtype, flat(q, Sq)), _buf(B * Skv, 2 * C, dtype, cat(flat(k, Skv), flat(v, Skv)))
        return (tq, tkv[:, :C], tkv[:, C:]), (C, 2 * C, 2 * C), [(tq, B * Sq, C), (tkv, B * Skv, 2 * C)]
    assert layout == 'apart'                   # three tensors, three different pitches, a poisoned gap in each
    lds = (C + 2 * vec, C + 4 * vec, C + 3 * vec)
    ts = [_buf(B * S, ld, dtype, flat(t, S)) for t, S, ld in zip((q, k, v), (Sq, Skv, Skv), lds)]
    return tuple(ts), lds, [(t, B * S, C) for t, S in zip(ts, (Sq, Skv, Skv))]


def _launch(dtype, hd, q, k, v, dout=None, layout=None):
    """q [B, Sq, C], k, v [B, Skv, C], dout [B, Sq, C] (CPU, on the grid of `dtype`): pack them as the module docstring
    says ('self' when Sq == Skv, else 'cross', unless `layout` says otherwise), run sdmi_attention and, with dout,
    sdmi_attention_bwd on what it stored.  bit-exact: poison in gaps and guard rows survives, inputs are unchanged.
    -> CPU (out [B, Sq, C], lse [B, heads, Sq], dq, dk, dv | None)."""
    B, Sq, C = q.shape
    Skv = k.shape[1]
    heads = C // hd
    layout = layout or ('self' if Sq == Skv else 'cross')
    ldo = C + (8 if dtype == BF16 else 4)
    (qd, kd, vd), (ldq, ldk, ldv), packed = _pack(dtype, Sq, Skv, C, layout, q, k, v)
    inputs = [t for t, _, _ in packed]
    before = [t.clone() for t in inputs]
    out = _buf(B * Sq, ldo, dtype)
    lse = _poison((B * heads + 1, Sq), F32)
    geom = dict(dtype=_dt(dtype), B=B, heads=heads, Sq=Sq, Skv=Skv, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo,
                scale=_scale(hd), head_dim=hd)
    _call('sdmi_attention', q=qd.data_ptr(), k=kd.data_ptr(), v=vd.data_ptr(), out=out.data_ptr(),
          lse=lse.data_ptr(), **geom)
    assert _only_poison_outside(out, B * Sq, C), 'forward wrote the pitch gap or the guard row of out'
    assert _only_poison_outside(lse, B * heads, Sq), 'forward wrote past the end of lse'
    assert all(_same_bits(a, b) for a, b in zip(inputs, before)), 'forward changed its inputs'
    res = [out[:B * Sq, :C].cpu().view(B, Sq, C), lse[:B * heads].cpu().view(B, heads, Sq), None, None, None]
    if dout is None:
        return res
    dob = _buf(B * Sq, ldo, dtype, dout.reshape(B * Sq, C))
    (dq, dk, dv), _, grads = _pack(dtype, Sq, Skv, C, layout)
    before += [out.clone(), lse.clone(), dob.clone()]
    _call('sdmi_attention_bwd', q=qd.data_ptr(), k=kd.data_ptr(), v=vd.data_ptr(), out=out.data_ptr(),
          dout=dob.data_ptr(), lse=lse.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), **geom)
    assert all(_only_poison_outside(*g) for g in grads), 'backward wrote a pitch gap or a guard row of dq / dk / dv'
    assert all(_same_bits(a, b) for a, b in zip(inputs + [out, lse, dob], before)), 'backward changed its inputs'
    res[2:] = [dq[:B * Sq, :C].cpu().view(B, Sq, C), dk[:B * Skv, :C].cpu().view(B, Skv, C),
               dv[:B * Skv, :C].cpu().view(B, Skv, C)]
    return res


def _assert_bound(key, what, got, exact, rest, coef, bf16_out, const='r', base=0.0):
    """|got - exact| <= rest + const * coef (+ base), every element, const = r or a of EXPL[key]; for bf16 storage the
    rounding of the result, BF (|exact| + that bound), comes on top.  Records in NEED what `const` had to be."""
    value = EXPL[key][0 if const == 'r' else 1]
    got, exact = got.detach().double().cpu(), exact.double()
    assert got.shape == exact.shape, (what, got.shape, exact.shape)
    assert bool(torch.isfinite(got).all()), what
    err = (got - exact).abs()
    rest = rest.double().expand_as(exact) + base
    coef = coef.double().expand_as(exact)
    before_rounding = (err - TINY - BF * exact.abs()) / (1 + BF) if bf16_out else err - TINY
    need = ((before_rounding - rest).clamp_min(0.0) / coef.clamp_min(1e-300)).max()
    NEED[f'{key} {const}'] = max(NEED.get(f'{key} {const}', 0.0), float(need))
    bound = rest + value * coef
    if bf16_out:
        bound = bound + BF * (exact.abs() + bound)
    bound = bound + TINY
    NEED[f'{key} err/bound'] = max(NEED.get(f'{key} err/bound', 0.0), float((err / bound).max()))
    assert bool((err <= bound).all()), f'{key} {what}: {_worst(err, bound)}'


# ---- float64 references and the bounds derived from them ------------------------------------------------
def _forward_reference(q, k, v, hd):
    qh, kh, vh = _split(q, hd), _split(k, hd), _split(v, hd)
    S = _scale(hd) * qh @ kh.transpose(-1, -2)
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse.unsqueeze(-1))
    A = _scale(hd) * qh.abs() @ kh.abs().transpose(-1, -2)
    return dict(S=S, A=A, m=S.amax(-1), lse=lse, P=P, O=P @ vh, vabs=vh.abs())


def _check_forward(dtype, hd, ref, out, lse, tag):
    """expf + derived bounds of the module docstring on out and lse."""
    key = _keys(dtype, hd, ref['S'].shape[-1])[0]
    Skv = ref['S'].shape[-1]
    n = Skv + (Skv + 3) // 4
    P, O, m = ref['P'], ref['O'], ref['m']
    arg = P * ((hd + 1) * U * ref['A'] + 2 * U * (ref['S'].abs() + m.abs().unsqueeze(-1)))    # P_ij (e_ij - r)
    Pv = P @ ref['vabs']
    rest = arg @ ref['vabs'] + O.abs() * arg.sum(-1, keepdim=True) + n * U * (Pv + O.abs()) + 4 * U * O.abs() \
        + TINY * (ref['vabs'].sum(-2, keepdim=True) + n)
    if _is_mfma(dtype, hd):
        rest = rest + BF * Pv                                                      # P rounded to bf16 before P V
    _assert_bound(key, tag + ' out', _split(out, hd), O, rest, Pv + O.abs(), dtype == BF16)
    rest = arg.sum(-1) + n * U + 4 * U * (m.abs() + ref['lse'].abs() + (ref['lse'] - m).abs())
    _assert_bound(key, tag + ' lse', lse, ref['lse'], rest, torch.ones_like(m), False, const='a', base=EXPL[key][0])


def _check_backward(dtype, hd, q, k, v, dout, out, lse, dq, dk, dv, tag):
    """expf + derived bounds of the module docstring on dq, dk, dv; `out` and `lse` are what the forward stored."""
    Sq, Skv = q.shape[1], k.shape[1]
    _, key_q, key_kv = _keys(dtype, hd, Skv)
    mfma, bf, scale = _is_mfma(dtype, hd), dtype == BF16, _scale(hd)
    qh, kh, vh, do, oh = (_split(t, hd) for t in (q, k, v, dout, out))
    lse = lse.double().unsqueeze(-1)
    S = scale * qh @ kh.transpose(-1, -2)
    P = torch.exp(S - lse)
    D = (do * oh).sum(-1, keepdim=True)
    X = do @ vh.transpose(-1, -2) - D
    dS = P * X
    T = lambda t: t.transpose(-1, -2)
    arg = (hd + 1) * U * scale * qh.abs() @ T(kh.abs()) + 2 * U * (S.abs() + lse.abs())          # e_ij - r
    # dout v^T - D: two HD-term fp32 dots and the subtraction
    G = hd * U * (do.abs() @ T(vh.abs()) + (do * oh).abs().sum(-1, keepdim=True)) + U * X.abs()
    H = P * (arg * X.abs() + G) + U * dS.abs() + TINY * (X.abs() + 1)              # |dS^ - dS| without the r term
    PX = P * X.abs()                                                               # ... and what r multiplies
    # dV_jd = sum_i P_ij dout_id
    Pdo = T(P) @ do.abs()
    rest = T(P * arg) @ do.abs() + Sq * U * Pdo + 4 * U * (T(P) @ do).abs() \
        + TINY * (do.abs().sum(-2, keepdim=True) + Sq)
    if mfma:
        rest = rest + BF * Pdo
    _assert_bound(key_kv, tag + ' dv', _split(dv, hd), T(P) @ do, rest, Pdo, bf)
    # dQ_id = scale sum_j dS_ij k_jd
    exact, terms = scale * dS @ kh, scale * dS.abs() @ kh.abs()
    rest = scale * H @ kh.abs() + Skv * U * terms + 4 * U * exact.abs() + TINY * Skv
    if mfma:
        rest = rest + BF * terms
    _assert_bound(key_q, tag + ' dq', _split(dq, hd), exact, rest, scale * PX @ kh.abs(), bf)
    # dK_jd = scale sum_i dS_ij q_id
    exact, terms = scale * T(dS) @ qh, scale * T(dS.abs()) @ qh.abs()
    rest = scale * T(H) @ qh.abs() + Sq * U * terms + 4 * U * exact.abs() + TINY * Sq
    if mfma:
        rest = rest + BF * terms
    _assert_bound(key_kv, tag + ' dk', _split(dk, hd), exact, rest, scale * T(PX) @ qh.abs(), bf)


# ---- 1. random inputs, flat (amp 1) and peaked (amp 3) --------------------------------------------------
# (Sq, Skv) and the path the pair reaches
MFMA32 = [
    (33, 1, 'one key, 31 pad keys'), (1, 7, 'one query; slot keys; backward query chunks of 128'),
    (31, 31, 'self, ragged block on both sides'), (33, 32, 'one full key block; second wave with one query'),
    (33, 33, 'self, ragged second 32-key block'), (130, 100, 'second workgroup with one active wave'),
    (129, 511, 'one key short of the LDS chunk; second workgroup'), (31, 512, 'exactly one LDS chunk'),
    (1, 513, 'second LDS chunk: one ragged block'), (130, 545, 'second LDS chunk: one full plus one ragged block'),
    (129, 33, 'backward: Skv > 32 switches to query chunks of 512'),
    (127, 7, 'backward: one query short of the 128-chunk'), (128, 32, 'backward: exactly one 128-chunk, Skv = 32'),
    (129, 7, 'backward: second 128-chunk, one query'), (257, 32, 'backward: third 128-chunk; third dQ workgroup'),
    (130, 33, 'backward: ragged second key block of the dKV body'),
    (513, 129, 'backward: second key workgroup; second 512-chunk of queries'),
    (513, 513, 'self: second chunk on both sides of the backward'),
    (130, 513, 'backward: second 512-chunk of keys in the dQ body'),
]
MFMA64 = [(33, 17, 'one ragged block'), (130, 255, 'one key short of the 256-chunk'), (33, 256, 'exactly one chunk'),
          (33, 257, 'second chunk: one ragged block'), (130, 513, 'third chunk; second workgroup')]
VALU = [
    (65, 1, 'one key'), (1, 3, 'one query; less than one four-key step'), (63, 4, 'exactly one four-key step'),
    (64, 5, 'second four-key step, ragged'), (65, 15, 'dkv_small at head size 32'),
    (257, 16, 'last size of dkv_small; second query block'),
    (63, 17, 'first size of the lane-per-key dKV kernel'), (65, 100, 'second 64-query staging chunk, one query'),
    (64, 257, 'second key block of the dKV kernel'), (1, 400, 'largest key count'),
    (257, 257, 'self: second block on both sides'),
    (65, 65, 'self: staging chunk boundary'),
]
RANDOM = ([(BF16, 32, sq, skv, True, why) for sq, skv, why in MFMA32]
          + [(BF16, 64, sq, skv, False, why) for sq, skv, why in MFMA64]
          + [(dt, hd, sq, skv, True, why) for dt, hd in ((F32, 32), (F32, 48), (BF16, 48)) for sq, skv, why in VALU])


def _random_case(dtype, hd, Sq, Skv, amp):
    g = _gen(hd * 1000003 + Sq * 1009 + Skv * 7 + amp)
    C = HEADS * hd
    q = _q(torch.randn(BATCH, Sq, C, generator=g) * amp, dtype)
    k = _q(torch.randn(BATCH, Skv, C, generator=g) * amp, dtype)
    v = _q(torch.randn(BATCH, Skv, C, generator=g), dtype)
    dout = _q(torch.randn(BATCH, Sq, C, generator=g), dtype)
    return q, k, v, dout, _forward_reference(q, k, v, hd)


@pytest.mark.parametrize('amp', [1, 3])
@pytest.mark.parametrize('case', RANDOM, ids=lambda c: f'{_ID[c[0]]}-hd{c[1]}-{c[2]}x{c[3]}')
def test_random_inputs(case, amp):
    """q, k ~ N(0, amp^2), v, dout ~ N(0, 1): forward out and lse, then (head sizes 32 and 48) dq, dk, dv of the
    backward run on the stored out and lse.  expf + derived bounds per element; bit-exact poison."""
    dtype, hd, Sq, Skv, bwd, why = case
    q, k, v, dout, ref = _random_case(dtype, hd, Sq, Skv, amp)
    tag = f'{_ID[dtype]} hd{hd} {Sq}x{Skv} amp {amp} ({why})'
    out, lse, dq, dk, dv = _launch(dtype, hd, q, k, v, dout if bwd else None)
    _check_forward(dtype, hd, ref, out, lse, tag)
    if bwd:
        _check_backward(dtype, hd, q, k, v, dout, out, lse, dq, dk, dv, tag)


APART = [(BF16, 32, 130, 100, True), (BF16, 32, 33, 7, True), (BF16, 64, 33, 257, False), (F32, 32, 65, 17, True),
         (F32, 32, 65, 15, True), (F32, 48, 65, 100, True), (BF16, 48, 65, 100, True)]


@pytest.mark.parametrize('case', APART, ids=lambda c: f'{_ID[c[0]]}-hd{c[1]}-{c[2]}x{c[3]}')
def test_four_different_pitches(case):
    """In both production layouts ldk == ldv, so a kernel that took one for the other would pass every case above.
    One case per kernel with q, k, v (and dq, dk, dv) in three tensors of pitches C + 2 vec, C + 4 vec, C + 3 vec and
    out / dout at C + vec, a poisoned gap in each.  Same expf + derived bounds, amp 1; bit-exact poison."""
    dtype, hd, Sq, Skv, bwd = case
    q, k, v, dout, ref = _random_case(dtype, hd, Sq, Skv, 1)
    tag = f'{_ID[dtype]} hd{hd} {Sq}x{Skv} apart'
    out, lse, dq, dk, dv = _launch(dtype, hd, q, k, v, dout if bwd else None, layout='apart')
    _check_forward(dtype, hd, ref, out, lse, tag)
    if bwd:
        _check_backward(dtype, hd, q, k, v, dout, out, lse, dq, dk, dv, tag)


# ---- 2. planted keys ------------------------------------------------------------------------------------
def _planted(dtype, hd, Sq, Skv, a):
    """k_j = +-a by the first hd bits of j (xor a constant per image and head, so every head has its own keys),
    q_i = k_pi(i), pi(i) = (7 i + Skv - 1) mod Skv; v = +-(1 + n / 8).  Everything is exact in bf16."""
    g = _gen(hd * 7919 + Sq * 31 + Skv)
    C = HEADS * hd
    j = torch.arange(Skv).view(1, 1, Skv, 1)
    flip = (5 * torch.arange(BATCH).view(BATCH, 1, 1, 1) + torch.arange(HEADS).view(1, HEADS, 1, 1) + 1) & 7
    bits = ((j ^ flip) >> torch.arange(hd).clamp(max=62).view(1, 1, 1, hd)) & 1
    kh = a * (1.0 - 2.0 * bits.float())                                            # [B, heads, Skv, hd]
    pi = (7 * torch.arange(Sq) + Skv - 1) % Skv
    k, q = _merge(kh), _merge(kh[:, :, pi])
    v = (1 + torch.randint(0, 8, (BATCH, Skv, C), generator=g).float() / 8) \
        * (1 - 2 * torch.randint(0, 2, (BATCH, Skv, C), generator=g).float())
    dout = _q(torch.randn(BATCH, Sq, C, generator=g), dtype)
    assert all(torch.equal(_q(t, BF16), t) for t in (q, k, v))
    return q, k, v, dout, pi


def _check_planted_forward(dtype, hd, q, k, v, pi, out, lse, tag):
    ref = _forward_reference(q, k, v, hd)
    Sq = q.shape[1]
    # precondition, on the reference alone: all the mass of every row sits on key pi(i)
    off = ref['P'].sum(-1) - ref['P'][:, :, torch.arange(Sq), pi]
    assert float(off.max()) <= 2.0 ** -26, (tag, float(off.max()))
    assert _same_bits(out.to(dtype), v[:, pi].to(dtype)), f'{tag}: out is not v[pi] bit for bit'
    # lse_i = scale q_i . k_pi(i): hd products of one sign, so sum|terms| = |S|
    St = ref['S'][:, :, torch.arange(Sq), pi]
    err = (lse.double() - St).abs()
    bound = hd * U * St.abs() + 4 * U * St.abs() + (ref['lse'] - St)
    assert bool((err <= bound).all()), f'{tag} lse: {_worst(err, bound)}'


PLANTED = ([(BF16, 32, 130, skv, 8.0) for skv in (1, 33, 512, 513, 545)]
           + [(BF16, 64, 70, skv, 16.0) for skv in (17, 256, 257, 513)]
           + [(dt, hd, 65, skv, 8.0 if hd == 32 else 16.0) for dt, hd in ((F32, 32), (F32, 48), (BF16, 48))
              for skv in (1, 5, 16, 17, 257, 400)])


@pytest.mark.parametrize('case', PLANTED, ids=lambda c: f'{_ID[c[0]]}-hd{c[1]}-{c[2]}x{c[3]}')
def test_planted_keys(case):
    """Every query attends to exactly one key (query 0 to the last one, the rest walking across the block and chunk
    boundaries).  bit-exact: out[i] == v[pi(i)].  derived: lse_i within the fp32 bound of the dot product
    scale q_i . k_pi(i) (not bit-exact: the VALU kernels round the partial sums n * fl(a scale) * a, the
    matrix-core kernels hold the exact integer dot product but pass it through the exp2 domain, two roundings each
    way); dq, dk, dv (dV a gather-sum of dout rows, dQ and dK about 0) within the expf + derived bounds of
    test_random_inputs, which are absolute here and dominated by the argument rounding at |S| of several hundred."""
    dtype, hd, Sq, Skv, a = case
    q, k, v, dout, pi = _planted(dtype, hd, Sq, Skv, a)
    tag = f'planted {_ID[dtype]} hd{hd} {Sq}x{Skv}'
    bwd = hd != 64
    out, lse, dq, dk, dv = _launch(dtype, hd, q, k, v, dout if bwd else None)
    _check_planted_forward(dtype, hd, q, k, v, pi, out, lse, tag)
    if bwd:
        _check_backward(dtype, hd, q, k, v, dout, out, lse, dq, dk, dv, tag)


INJECTIVE = [(BF16, 32, 33, 100), (F32, 32, 33, 100), (F32, 32, 5, 15), (F32, 48, 33, 100), (BF16, 48, 33, 100)]


@pytest.mark.parametrize('case', INJECTIVE, ids=lambda c: f'{_ID[c[0]]}-hd{c[1]}-{c[2]}x{c[3]}')
def test_planted_keys_injective_dv(case):
    """Sq < Skv with gcd(7, Skv) = 1, so pi is injective: each dV row is one dout row or nothing.  a = 32 puts every
    off-target score 2 a^2 scale (290 and more) below lse, past 150 ln 2 where exp is 0 in fp32, denormals included.
    bit-exact: dV of a key no query attends to is 0 (a pad query leaking into dO^T P would show here), out == v[pi];
    expf + derived for the attended rows and for dq, dk."""
    dtype, hd, Sq, Skv = case
    assert math.gcd(7, Skv) == 1 and Sq < Skv and 2 * 32.0 ** 2 * _scale(hd) > 2 * 150 * math.log(2)
    q, k, v, dout, pi = _planted(dtype, hd, Sq, Skv, 32.0)
    tag = f'injective {_ID[dtype]} hd{hd} {Sq}x{Skv}'
    out, lse, dq, dk, dv = _launch(dtype, hd, q, k, v, dout)
    _check_planted_forward(dtype, hd, q, k, v, pi, out, lse, tag)
    _check_backward(dtype, hd, q, k, v, dout, out, lse, dq, dk, dv, tag)
    unattended = torch.ones(Skv, dtype=torch.bool)
    unattended[pi] = False
    assert int(unattended.sum()) == Skv - Sq
    assert bool((dv[:, unattended] == 0).all()), f'{tag}: dV of a key nobody attends to is not 0'


# ---- 3. refusals ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_launch():
    """Each call must report an error through the ABI and launch nothing: bit-exact, the outputs keep their poison."""
    Err = _L().SdmiError
    n = (BATCH * 401 + 1) * (3 * 64 + 16)                           # room for every geometry below, had it launched
    src = {dt: torch.ones(n, dtype=dt, device=DEV) for dt in (F32, BF16)}
    lse_in = torch.zeros(n, device=DEV)
    outs = {(dt, name): _poison((n,), dt) for dt in (F32, BF16) for name in ('out', 'dq', 'dk', 'dv')}
    outs[F32, 'lse'] = _poison((n,), F32)

    def args(dtype, hd, Skv, bwd, **pitch):
        C, s = HEADS * hd, src[dtype].data_ptr()
        kw = dict(q=s, k=s, v=s, dtype=_dt(dtype), B=BATCH, heads=HEADS, Sq=4, Skv=Skv, ldq=C, ldk=C, ldv=C, ldo=C,
                  scale=_scale(hd), head_dim=hd)
        kw.update(pitch)
        if bwd:
            kw.update(out=s, dout=s, lse=lse_in.data_ptr(), **{g: outs[dtype, g].data_ptr() for g in ('dq', 'dk', 'dv')})
        else:
            kw.update(out=outs[dtype, 'out'].data_ptr(), lse=outs[F32, 'lse'].data_ptr())
        return ('sdmi_attention_bwd' if bwd else 'sdmi_attention'), kw

    bad = [args(F32, 32, 401, False), args(F32, 32, 401, True),                                  # fp32 beyond 400 keys
           args(F32, 48, 401, False), args(F32, 48, 401, True),                                  # head size 48 beyond 400
           args(BF16, 48, 401, False), args(BF16, 48, 401, True),
           args(F32, 64, 17, False),                                                             # head size 64 in fp32
           args(BF16, 64, 17, True), args(F32, 64, 17, True),                                    # ... and in the backward
           args(BF16, 40, 17, False), args(F32, 40, 17, False), args(BF16, 40, 17, True),        # head size 40
           args(BF16, 32, 0, False), args(BF16, 64, 0, False), args(BF16, 32, 0, True),          # no keys, bf16 path
           args(BF16, 32, 17, False, ldo=97), args(F32, 32, 17, False, ldq=97),                  # pitch of C + 1
           args(BF16, 32, 17, True, ldk=97), args(F32, 48, 17, True, ldv=145)]
    for fname, kw in bad:
        with pytest.raises(Err):
            _call(fname, **kw)
        assert len(_L().lib().sdmi_last_error()) > 0, (fname, kw)
    torch.cuda.synchronize()
    for (dtype, name), o in outs.items():
        assert _same_bits(o, _poison((n,), dtype)), f'{name} ({_ID[dtype]}) was written by a refused call'
