"""Float64 reference of the conv / linear backward (include/sdmi.h: sdmi_wgrad, sdmi_bwd_pair), plain tensor code with
explicit loops over the filter taps, from the definitions of the C ABI:

    forward     y[b, oy, ox, n] = sum_{kh, kw, ci} A[(b, oy, ox)][(kh, kw, ci)] W[n][(kh, kw, ci)]
    A           the NHWC input x at virtual pixel (oy stride - pad_t + kh, ox stride - pad_l + kw): zero outside the image;
                with `ups` the image is the nearest x2 view of x (virtual pixel (iy, ix) of 2H x 2W reads x[iy / 2, ix / 2])
    wgrad       S[n][k] = sum_m dY[m][n] A[m][k]          A0[n][k] = sum_m |dY[m][n] A[m][k]|
    bias        sb[n]   = sum_m dY[m][n]                   ab[n]    = sum_m |dY[m][n]|
    dgrad       Z[p][ci] = sum over the (m, kh, kw) whose tap reads pixel p, and n, of dY[m][n] W[n][(kh, kw, ci)]
                Az the same sum over |dY W|

A0 / ab / Az are what an accumulation error is relative to (not |S|: where the products cancel, |S| says nothing about
their rounding).  `g` is any object with the geometry fields of SdmiWgradArgs (B, H, W, Cin, Ho, Wo, KH, KW, stride,
pad_t, pad_l, ups) and N.  tests/test_wgrad_ref_cpu.py holds all of this against torch.autograd in float64."""
import torch


def src_index(n_out, stride, pad, k, size, ups):
    """Source index of filter tap k for every output coordinate, and whether it exists."""
    i = torch.arange(n_out) * stride - pad + k
    if ups:
        ok, s = (i >= 0) & (i < 2 * size), i // 2
    else:
        ok, s = (i >= 0) & (i < size), i
    return ok, s.clamp(0, size - 1)


def tap(x, g, kh, kw):
    """Columns [(kh, kw, 0), (kh, kw, Cin)) of A for all rows: [B * Ho * Wo, Cin] float64 (x: [B, H, W, Cin])."""
    oky, sy = src_index(g.Ho, g.stride, g.pad_t, kh, g.H, g.ups)
    okx, sx = src_index(g.Wo, g.stride, g.pad_l, kw, g.W, g.ups)
    a = x.double()[:, sy][:, :, sx] * (oky[:, None] & okx[None, :])[None, :, :, None]
    return a.reshape(-1, g.Cin)


def wgrad_reference(x, dy, g, with_abs=True):
    """-> S [N, K], A0 [N, K] (None without with_abs), sb [N], ab [N]; x [B, H, W, Cin], dy [M, N]."""
    dy = dy.double()
    K = g.KH * g.KW * g.Cin
    S = torch.zeros(dy.shape[1], K, dtype=torch.float64)
    A0 = torch.zeros_like(S) if with_abs else None
    dyt, dyat = dy.t().contiguous(), dy.abs().t().contiguous()
    for kh in range(g.KH):
        for kw in range(g.KW):
            a = tap(x, g, kh, kw)
            k0 = (kh * g.KW + kw) * g.Cin
            S[:, k0:k0 + g.Cin] = dyt @ a
            if with_abs:
                A0[:, k0:k0 + g.Cin] = dyat @ a.abs()
    return S, A0, dy.sum(0), dy.abs().sum(0)


def dgrad_reference(dy, w, g, with_abs=True):
    """-> Z [B * H * W, Cin], Az (None without with_abs); dy [M, N], w [N, K] (K = (kh, kw, ci)).  Stride-1 problems
    without `ups` (the pair launch's): output row (b, oy, ox) and tap (kh, kw) touch pixel (oy - pad_t + kh, ox - pad_l + kw)."""
    assert g.stride == 1 and not g.ups
    dy4 = dy.double().view(g.B, g.Ho, g.Wo, -1)
    w = w.double()
    Z = torch.zeros(g.B, g.H, g.W, g.Cin, dtype=torch.float64)
    Az = torch.zeros_like(Z) if with_abs else None
    for kh in range(g.KH):
        # output rows oy whose tap kh lies inside the image: iy = oy - pad_t + kh
        oy0, oy1 = max(0, g.pad_t - kh), min(g.Ho, g.H + g.pad_t - kh)
        for kw in range(g.KW):
            ox0, ox1 = max(0, g.pad_l - kw), min(g.Wo, g.W + g.pad_l - kw)
            if oy0 >= oy1 or ox0 >= ox1:
                continue
            k0 = (kh * g.KW + kw) * g.Cin
            wt = w[:, k0:k0 + g.Cin]
            d = dy4[:, oy0:oy1, ox0:ox1]
            iy0, ix0 = oy0 - g.pad_t + kh, ox0 - g.pad_l + kw
            Z[:, iy0:iy0 + (oy1 - oy0), ix0:ix0 + (ox1 - ox0)] += d @ wt
            if with_abs:
                Az[:, iy0:iy0 + (oy1 - oy0), ix0:ix0 + (ox1 - ox0)] += d.abs() @ wt.abs()
    Z = Z.view(-1, g.Cin)
    return Z, (Az.view(-1, g.Cin) if with_abs else None)
