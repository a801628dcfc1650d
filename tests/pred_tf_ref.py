"""float64 restatement of the transformer slot transition (video_based/models/predictor.py:20-44: nn.TransformerEncoder,
norm_first, ReLU feed-forward, no dropout) with a per-element error bound for a kernel that computes it in fp32 with
bf16 MFMA operands (sdmi_pred_tf), for tests/test_gpu_pred_tf.py.  Torch on the CPU only.

`rnd` is applied at exactly the feed points the header of sdmi_pred_tf lists: LN1(x); q, k, v; the softmax
probabilities; the attention output; LN2(x); the hidden layer.  With rnd = ident the function is
oracle.transformer_predictor (the GPU test asserts that the two agree to 1e-12).

The bound is carried stage by stage next to the values, per element (U = 2^-24, BF = 2^-8; d_v = bound on |kernel's v -
reference's v|):

  product   out = a W^T (+ bias) (+ residual), K terms:  d_out = d_a |W|^T + (K + kacc) U A (+ d_residual),
            A = |a| |W|^T + |bias| + |residual|;  kacc = 3 (bias add, residual add, the scale of the scores)
  feed      a value v rounded to bf16 where it feeds a product: d_f = d_v + feed |v|
              feed = 2 BF    against this reference with rnd = bf16 (both round; they differ by at most one bf16 ulp
                             on top of d_v)
              feed = 1.01 BF against the reference that does not round (half an ulp of the kernel's own value)
  LayerNorm fp32, two-pass, on an input that carries d_x already:
              own      |g| rstd D U max_row |x| + (D + 8) U |g (x - m) rstd| + 2 U |xn|   (test_gpu_predictor.py's row)
              carried  |g| rstd (d_x + mean(d_x) + |xh| mean(|xh| d_x)) (1 + 4 rho),  xh = (x - m) rstd,
                       rho = rstd max_row d_x
            the carried row is the exact first-order term (d xn_i / d x_j = g_i rstd (delta_ij - 1 / D - xh_i xh_j / D),
            taken with absolute values); rstd and xh move by at most a relative rho inside the d_x ball, each entering
            the derivative at most twice: (1 + 4 rho) covers the second order
  scores    s = scale q k^T over head_dim terms: the product row with both operands carrying an error,
              d_s = scale (d_q |k|^T + |q| d_k^T + d_q d_k^T) + (head_dim + kacc) U scale |q| |k|^T
  softmax   p_i' = sigmoid(logit(p_i) + t), |t| <= 2 Delta, Delta = max_row d_s, and sigmoid' = p (1 - p) grows by at most
            e^|t| on the way:  carried = p (1 - p) 2 Delta e^(2 Delta)   (the scores' error through p (1 - p))
            evaluated in fp32 as e_i / sum e, e_i = __expf(s_i - max s), |__expf(v) - exp(v)| <= r exp(v) + a
            (the row EXPF['exp'] of the test):
              own = p (2 r + 2 U max_row |s - max s| + 20 U) + a (1 + N p)
            (r twice: numerator and denominator; the subtraction's rounding moves the exponent by U |s - max s|; 16 + 4 U
            for the sum, the division and the scale; the sum is >= 1, so an absolute a in a term is at most a in p and
            N a p through the sum).  d_p = min(carried + own, 1); past 2 Delta = 50 the carried row is above 1 wherever
            p (1 - p) is not exactly 0, so the exponent is held there to keep the arithmetic finite.
  P V       16 terms (the kernel's k extent; pad keys are exact zeros), both operands carry an error, as the scores.

Second-order cross terms between stages other than the ones written above are not carried (the own-error rows are
evaluated at the reference's values): they are d U, below 1e-9 of every bound here."""
import torch

U = 2.0 ** -24
BF = 2.0 ** -8
NAME = 'predictor'
MATS = ('self_attn.in_proj_weight', 'self_attn.out_proj.weight', 'linear1.weight', 'linear2.weight')


def ident(t):
    return t


def bf16(t):
    """Round to bf16 (nearest even), keep the dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def weights(D, F, layers, seed, qk_gain=1.0, amp=None, name=NAME):
    """fp32 CPU weights of one geometry under the checkpoint's key names, matrices on the bf16 grid (so the packed bf16
    operands and a float64 copy hold the same values).  qk_gain scales the q and k rows of in_proj (large scores).
    amp = None: matrix entries N(0, 1 / K), the scale of a trained layer.  amp = a: entries N(0, (a / (0.8 K))^2), so
    that a row's sum of magnitudes -- the factor by which `d_a |W|^T` grows an error -- is about a."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g) * (1.0 if amp is None else amp / (0.8 * s[-1] ** 0.5))
    rv = lambda *s: torch.randn(*s, generator=g)
    q = lambda t: t.to(torch.bfloat16).float()
    W = {}
    for i in range(layers):
        l = f'{name}.transformer_encoder.layers.{i}'
        wqkv = rn(3 * D, D) / D ** 0.5
        wqkv[:2 * D] *= qk_gain
        W.update({f'{l}.norm1.weight': 1 + 0.1 * rv(D), f'{l}.norm1.bias': 0.05 * rv(D),
                  f'{l}.self_attn.in_proj_weight': q(wqkv), f'{l}.self_attn.in_proj_bias': 0.05 * rv(3 * D),
                  f'{l}.self_attn.out_proj.weight': q(rn(D, D) / D ** 0.5), f'{l}.self_attn.out_proj.bias': 0.05 * rv(D),
                  f'{l}.norm2.weight': 1 + 0.1 * rv(D), f'{l}.norm2.bias': 0.05 * rv(D),
                  f'{l}.linear1.weight': q(rn(F, D) / D ** 0.5), f'{l}.linear1.bias': 0.05 * rv(F),
                  f'{l}.linear2.weight': q(rn(D, F) / F ** 0.5), f'{l}.linear2.bias': 0.05 * rv(D)})
    return W


def _A(a, m, *add):
    return a.abs() @ m.abs().t() + sum(t.abs() for t in add)


def _ln(x, g, b, d_x, eps=1e-5):
    D = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    xc = x - m
    rstd = ((xc * xc).mean(-1, keepdim=True) + eps).rsqrt()
    xh = xc * rstd
    xn = xh * g + b
    own = g.abs() * rstd * (D * U * x.abs().amax(-1, keepdim=True)) + (D + 8) * U * (g * xh).abs() + 2 * U * xn.abs()
    rho = rstd * d_x.amax(-1, keepdim=True)
    carried = g.abs() * rstd * (d_x + d_x.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * d_x).mean(-1, keepdim=True))
    return xn, own + carried * (1 + 4 * rho)


def ref_and_bound(W, x, heads, layers, rnd=ident, feed=0.0, kacc=3, expf=(0.0, 0.0), name=NAME):
    """x [B, N, D] float64 -> (y, d_y, extremes): the transition with `rnd` at the feed points and the header's bound for a
    kernel whose feeds differ from the reference's by `feed` |v|.  extremes: dict(pmax = largest softmax probability,
    smax = largest |score|) for the tests that ask for a particular regime."""
    W = {k: v.double() for k, v in W.items()}
    B, N, D = x.shape
    hd = D // heads
    scale = hd ** -0.5
    r_e, a_e = expf
    d_x = torch.zeros_like(x)
    sp = lambda t: t.view(B, N, heads, hd).permute(0, 2, 1, 3)          # [B, h, N, hd]
    ext = dict(pmax=0.0, smax=0.0)
    for i in range(layers):
        l = f'{name}.transformer_encoder.layers.{i}'
        w = lambda k: W[f'{l}.{k}']
        xn, d_xn = _ln(x, w('norm1.weight'), w('norm1.bias'), d_x)
        f0, d_f0 = rnd(xn), d_xn + feed * xn.abs()
        wqkv, bqkv = w('self_attn.in_proj_weight'), w('self_attn.in_proj_bias')
        qkv = f0 @ wqkv.t() + bqkv
        d_qkv = d_f0 @ wqkv.abs().t() + (D + kacc) * U * _A(f0, wqkv, bqkv)
        fq, d_fq = rnd(qkv), d_qkv + feed * qkv.abs()
        (q, k, v), (dq, dk, dv) = (sp(t) for t in fq.chunk(3, -1)), (sp(t) for t in d_fq.chunk(3, -1))
        kT, dkT = k.transpose(-1, -2), dk.transpose(-1, -2)
        s = scale * (q @ kT)
        d_s = scale * (dq @ kT.abs() + q.abs() @ dkT + dq @ dkT) + (hd + kacc) * U * scale * (q.abs() @ kT.abs())
        p = s.softmax(-1)
        delta = d_s.amax(-1, keepdim=True)
        spread = (s - s.amax(-1, keepdim=True)).abs().amax(-1, keepdim=True)
        d_p = p * (1 - p) * 2 * delta * torch.exp((2 * delta).clamp_max(50.0)) + p * (2 * r_e + 2 * U * spread + 20 * U) + a_e * (1 + N * p)
        d_p = d_p.clamp_max(1.0)
        ext = dict(pmax=max(ext['pmax'], float(p.max())), smax=max(ext['smax'], float(s.abs().max())))
        fp, d_fp = rnd(p), d_p + feed * p
        o = fp @ v
        d_o = d_fp @ v.abs() + fp.abs() @ dv + d_fp @ dv + (16 + kacc) * U * (fp.abs() @ v.abs())
        o, d_o = (t.permute(0, 2, 1, 3).reshape(B, N, D) for t in (o, d_o))
        fo, d_fo = rnd(o), d_o + feed * o.abs()
        wo, bo = w('self_attn.out_proj.weight'), w('self_attn.out_proj.bias')
        x1 = fo @ wo.t() + bo + x
        d_x1 = d_fo @ wo.abs().t() + (D + kacc + 1) * U * _A(fo, wo, bo, x) + d_x
        xn2, d_xn2 = _ln(x1, w('norm2.weight'), w('norm2.bias'), d_x1)
        f2, d_f2 = rnd(xn2), d_xn2 + feed * xn2.abs()
        w1, b1, w2, b2 = w('linear1.weight'), w('linear1.bias'), w('linear2.weight'), w('linear2.bias')
        hid = torch.relu(f2 @ w1.t() + b1)
        d_hid = d_f2 @ w1.abs().t() + (D + kacc) * U * _A(f2, w1, b1)
        fh, d_fh = rnd(hid), d_hid + feed * hid.abs()
        x = fh @ w2.t() + b2 + x1
        d_x = d_fh @ w2.abs().t() + (w1.shape[0] + kacc + 1) * U * _A(fh, w2, b2, x1) + d_x1
    return x, d_x, ext
