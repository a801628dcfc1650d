"""The upsample convolutions' training path ("nearest 2x, then 3x3, pad 1" as ConvTranspose2d(4, stride 2, padding 1)
with the composite filter W4: kern.GemmFn / WeightBank.ups_train_ok), launched as kern.py launches it -- ops.conv2d for
the forward and the data gradient, bwd.LayerProblem.upsampled for the weight gradient -- and pinned, element by element,
to float64 CPU references computed from the tensors the kernels read.  The discipline is tests/test_gpu_igemm_pins.py's.

Tolerances (U = 2^-24, BF = 2^-8; A = sum |a| |w| over the contraction, z the exact value):
  bit-exact   (a) both composite operands, single and batched form: torch's float32 sum of the 1 / 2 / 4 source taps,
              ky ascending, kx ascending inside one ky, rounded to bf16 once (kern.ups_composite); guard elements around
              every destination; the fold of dW4 (each term the sum of its M-split partials in split order, then the
              four-term fp32 sum u ascending, v ascending inside one u: kern.ups_fold) and its accumulation into a
              pre-filled destination, given the partials the weight gradient wrote; the bias partials the fold launch
              writes against sdmi_rowgroup_sum's.
  derived     (b) forward and (c) dx, bf16 storage: (K + s + 3) U A + 4 U |z|, one BF rounding on top (s = K slices of
              the split-K second stage); (d) dW4, fp32: (M + s + 3) U A + 4 U |z| (M low-resolution rows, s = M-splits);
              dw after the fold: the four terms' bounds + 4 U (|prefill| + sum of |term| + bound) for the three adds of
              the fold and the one into the destination; dbias: (rows + nblk + 1) U sum |dy| + 4 U |z|.
              (e) the same outputs against the ORIGINAL layer -- float64 3x3 convolution of the upsampled input with the
              bf16 shadow weights, and its autograd gradients: forward and dx widened by BF A', A' = sum |x| |W4| with
              the exact W4 (the operand's one rounding); dw needs no widening (no weight operand enters it).
Routes are asserted with sdmi_igemm_last_route / sdmi_wgrad_route.  Shapes: the issue's three -- borders dominate in the
first, two K chunks and N != Cin in the second, non-square with a ragged N tile in the third."""
import ctypes
import functools
import types

import pytest
import torch
import torch.nn.functional as F

from slotdiffusion_amd import bwd, kern, ops
from tests.test_gpu_bwd_helpers import (BF, DEV, U, _call, _end_the_session_on_a_gpu_fault, _L,  # noqa: F401
                                        _same_bits, _worst)
from tests.test_gpu_igemm_pins import _route_name
from tests.test_gpu_wgrad_pins import route_name as _wgrad_route_name

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SHAPES = {'b2-4to8-c64-n64': (2, 4, 4, 64, 64), 'b2-8to16-c128-n64': (2, 8, 8, 128, 64),
          'b1-4x8to8x16-c64-n192': (1, 4, 8, 64, 192)}          # B, H, W, Cin, Cout
IDS = list(SHAPES)
GUARD, POISON = 64, -3.0
PRE_W, PRE_B = 0.5, 0.25                                         # what the gradient destinations hold before


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _guarded(n, dtype, value=POISON):
    """-> (whole buffer, the n elements in its middle)."""
    buf = torch.full((n + 2 * GUARD,), value, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_kept(buf, value=POISON):
    return bool((buf[:GUARD] == value).all()) and bool((buf[-GUARD:] == value).all())


def _igemm_split(M, N, K):
    """dispatch's own K split of a 64 x 64 bf16 launch with a workspace (igemm.hip: 384 workgroups aimed for, at least
    four 128-byte K tiles per slice, at most 16 slices)."""
    t64, nk, s = -(-M // 64) * -(-N // 64), -(-K * 2 // 128), 1
    while t64 * s < 384 and s * 2 <= nk // 4 and s < 16:
        s *= 2
    return s


@functools.lru_cache(None)
def _run(cid):
    """Every launch of one shape, once; results on the CPU next to their float64 references."""
    B, H, W, ci, co = SHAPES[cid]
    L = _L()
    g = torch.Generator().manual_seed(sum(map(ord, cid)))
    w = (torch.randn(co, 3, 3, ci, generator=g) / (9 * ci) ** 0.5).to(BF16)
    x = torch.randn(B, H, W, ci, generator=g).to(BF16)
    dy = torch.randn(B, 2 * H, 2 * W, co, generator=g).to(BF16)
    dal = torch.randn(B, H, W, ci, generator=g).to(BF16)
    bias = torch.randn(co, generator=g)
    wd_, xd, dyd, dald, biasd = (t.to(DEV) for t in (w, x, dy, dal, bias))
    r = types.SimpleNamespace(B=B, H=H, W=W, ci=ci, co=co, w=w, x=x, dy=dy, dal=dal, bias=bias)
    st = torch.cuda.current_stream().cuda_stream

    # ---- (a) operands: single form and ONE batched launch over a two-entry table
    n = 16 * ci * co
    fwd_buf, fwd = _guarded(n, BF16)
    wdg_buf, wdg = _guarded(n, BF16)
    for dst, comp in ((fwd, 'SDMI_PACK_UPS_FWD'), (wdg, 'SDMI_PACK_UPS_DGRAD')):
        _call('sdmi_pack_dgrad', src=wd_.data_ptr(), dst=dst.data_ptr(), dtype=L.BF16, Cout=co, KH=3, KW=3, Cin=ci,
              CoutPad=co, comp=L.ENUMS[comp])
    fwd2_buf, fwd2 = _guarded(n, BF16)
    wdg2_buf, wdg2 = _guarded(n, BF16)
    blocks = 16 * -(-co // 64) * -(-ci // 64)
    descs = (L.CSTRUCT['SdmiPackDesc'] * 2)()
    for i, (dst, comp) in enumerate(((fwd2, 'SDMI_PACK_UPS_FWD'), (wdg2, 'SDMI_PACK_UPS_DGRAD'))):
        d = descs[i]
        d.src, d.dst, d.Cout, d.KH, d.KW, d.Cin, d.CoutPad, d.block_begin = wd_.data_ptr(), dst.data_ptr(), co, 3, 3, ci, co, i * blocks
        d.kstep, d.nkh, d.nkw = L.ENUMS[comp], 4, 4
    tab = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    _call('sdmi_pack_dgrad_batch', descs=tab.data_ptr(), n_desc=2, dtype=L.BF16, total_blocks=2 * blocks)
    torch.cuda.synchronize()
    r.guards = all(_guards_kept(b) for b in (fwd_buf, wdg_buf, fwd2_buf, wdg2_buf))
    r.fwd, r.wdg, r.fwd2, r.wdg2 = (t.cpu() for t in (fwd, wdg, fwd2, wdg2))

    # ---- (b) forward
    out_buf, out = _guarded(B * 4 * H * W * co, BF16)
    out = out.view(B, 2 * H, 2 * W, co)
    ops.conv2d(xd, fwd.view(4, co, 4 * ci), biasd, kh=2, kw=2, out=out, parity4=True)
    r.route_fwd = _route_name(L.lib().sdmi_igemm_last_route())
    # ---- (c) dx, without and with the gradient of x's other consumer in the epilogue
    dx = ops.conv2d(dyd, wdg.view(ci, 16 * co), None, kh=4, kw=4, stride=2, pad=(1, 1, 1, 1))
    r.route_dx = _route_name(L.lib().sdmi_igemm_last_route())
    dxr = ops.conv2d(dyd, wdg.view(ci, 16 * co), None, kh=4, kw=4, stride=2, pad=(1, 1, 1, 1), residual=dald)
    r.route_dxr = _route_name(L.lib().sdmi_igemm_last_route())
    # ---- (d) dW4 by sdmi_wgrad with the roles swapped, folded into a pre-filled destination; dbias
    # (the M-split the planner gives these sizes, and -- where M has two 64-row steps -- a forced split of two, so that the
    # fold of the partials is covered)
    P = bwd.LayerProblem.upsampled(xd, co)
    r.P = P
    rows = B * 4 * H * W
    chunk = next((c for c in (256, 128, 64) if rows % c == 0), rows)
    r.rows, r.nblk = rows, rows // chunk
    r.wg, kept = [], True
    for splits in [bwd.standalone_splits(P)] + ([2] if P.M >= 128 else []):
        fields = dict(P.wgrad_fields(), splits=splits, accumulate=0, defer_fold=1)
        route = _wgrad_route_name(L.query('sdmi_wgrad_route', **fields))
        ws_buf, ws = _guarded(splits * (P.N * P.K + P.N), F32)
        _call('sdmi_wgrad', a=dyd.data_ptr(), dy=xd.data_ptr(), dw=ws.data_ptr(), dbias=0, workspace=ws.data_ptr(), **fields)
        dw_buf, dwv = _guarded(co * 9 * ci, F32, PRE_W)
        dw0_buf, dwv0 = _guarded(co * 9 * ci, F32)
        part_buf, part = _guarded(r.nblk * co, F32)
        _call('sdmi_ups_fold_dw', dw4=ws.data_ptr(), dw=dwv.data_ptr(), Cin=ci, Cout=co, accumulate=1, splits=splits,
              dy=dyd.data_ptr(), bias_part=part.data_ptr(), dtype=L.BF16, rows=rows, rows_per=chunk)
        _call('sdmi_ups_fold_dw', dw4=ws.data_ptr(), dw=dwv0.data_ptr(), Cin=ci, Cout=co, accumulate=0, splits=splits)
        torch.cuda.synchronize()
        kept = kept and _guards_kept(ws_buf) and _guards_kept(dw_buf, PRE_W) and _guards_kept(dw0_buf) and _guards_kept(part_buf)
        r.wg.append(types.SimpleNamespace(splits=splits, route=route, ws=ws[:splits * P.N * P.K].view(splits, -1).cpu(),
                                          dwv=dwv.cpu(), dwv0=dwv0.cpu(), part=part.cpu()))
    part_ref = torch.empty((r.nblk, co), dtype=F32, device=DEV)          # (these sizes take its long-group kernel)
    _call('sdmi_rowgroup_sum', x=dyd.data_ptr(), out=part_ref.data_ptr(), dtype=L.BF16, groups=r.nblk, rows_per=chunk,
          N=co, ldx=co)
    db_buf, db = _guarded(co, F32, PRE_B)
    items = L.struct_array('SdmiColsumItem', [dict(partial=part.data_ptr(), out0=db.data_ptr(), out1=0, nblk=r.nblk, C=co)])
    L.call('sdmi_colsum_group', st, items=ctypes.addressof(items), n=1)
    torch.cuda.synchronize()
    r.guards_out = kept and _guards_kept(out_buf) and _guards_kept(db_buf, PRE_B)
    r.out, r.dx, r.dxr, r.db, r.part_ref = (t.cpu() for t in (out, dx, dxr, db, part_ref))
    r.inputs_kept = all(_same_bits(a, b.cpu()) for a, b in ((w, wd_), (x, xd), (dy, dyd), (dal, dald)))

    # ---- float64 references
    w64 = w.double().permute(0, 3, 1, 2)                                  # [co][ci][3][3]
    r.w4q = kern.ups_composite(w.float().permute(0, 3, 1, 2)).to(BF16)    # the operand: fp32 sums, rounded once
    w4q, w4x = r.w4q.double(), kern.ups_composite(w64)                    # ... and the exact composite filter
    x64, dy64 = _nchw(x.double()).requires_grad_(True), _nchw(dy.double())
    tconv = lambda a, f: F.conv_transpose2d(a, f.permute(1, 0, 2, 3), stride=2, padding=1)
    sconv = lambda a, f: F.conv2d(a, f.permute(1, 0, 2, 3), stride=2, padding=1)
    b64 = bias.double().view(1, -1, 1, 1)
    r.y, r.y_A = tconv(x64.detach(), w4q) + b64, tconv(x64.detach().abs(), w4q.abs())
    r.y_Ax = tconv(x64.detach().abs(), w4x.abs())
    r.gx, r.gx_A = sconv(dy64, w4q), sconv(dy64.abs(), w4q.abs())
    r.gx_Ax = sconv(dy64.abs(), w4x.abs())
    w4v = w4q.permute(1, 0, 2, 3).contiguous().requires_grad_(True)       # [ci][co][4][4]
    (g4,) = torch.autograd.grad(F.conv2d(dy64, w4v, stride=2, padding=1), [w4v], x64.detach())
    (g4a,) = torch.autograd.grad(F.conv2d(dy64.abs(), w4v, stride=2, padding=1), [w4v], x64.detach().abs())
    r.g4, r.g4_A = g4.permute(1, 0, 2, 3), g4a.permute(1, 0, 2, 3)        # [co][ci][4][4]
    w64v = w64.clone().requires_grad_(True)
    y0 = F.conv2d(F.interpolate(x64, scale_factor=2, mode='nearest'), w64v, padding=1) + b64
    r.y0 = y0.detach()
    r.gx0, r.gw0 = torch.autograd.grad(y0, [x64, w64v], dy64)
    r.gb, r.gb_A = dy64.sum((0, 2, 3)), dy64.abs().sum((0, 2, 3))
    return r


def _within(what, got, exact, bound):
    err = (got.double() - exact).abs()
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= bound).all()), f'{what}: {_worst(err, bound)} (largest share of the bound used: ' \
                                       f'{float((err / bound.clamp_min(1e-300)).max()):.3f})'


def _bf16_bound(K, s, A, z):
    b = (K + s + 3) * U * A + 4 * U * z.abs()
    return b + BF * (z.abs() + b)


@pytest.mark.parametrize('cid', IDS)
def test_composite_operands_bit_exact(cid):
    """(a): both layouts, from the single launch and from the batched one; nothing written outside them."""
    r = _run(cid)
    ci, co = r.ci, r.co
    want_wd = r.w4q.permute(1, 2, 3, 0).contiguous().view(-1)                      # [ci][4][4][co]
    want_fwd = torch.empty(4, co, 2, 2, ci, dtype=BF16)
    for py in (0, 1):
        for px in (0, 1):
            for rr in (0, 1):
                for c in (0, 1):
                    want_fwd[2 * py + px, :, rr, c, :] = r.w4q[:, :, 3 - 2 * rr - py, 3 - 2 * c - px]
    for name, got, want in (('forward operand', r.fwd, want_fwd.view(-1)), ('forward operand (batched)', r.fwd2, want_fwd.view(-1)),
                            ('dgrad operand', r.wdg, want_wd), ('dgrad operand (batched)', r.wdg2, want_wd)):
        assert _same_bits(got, want), f'{cid}: {name} differs from the fp32 sum rounded to bf16'
    assert r.guards and r.inputs_kept


@pytest.mark.parametrize('cid', IDS)
def test_forward(cid):
    """(b) against the composite definition, (e) against the original layer."""
    r = _run(cid)
    assert r.route_fwd[0] == 'dma 64x64 st4 lw4 mode2', r.route_fwd
    got = _nchw(r.out.float())
    bound = _bf16_bound(4 * r.ci, 0, r.y_A, r.y)
    _within(f'{cid} forward', got, r.y, bound)
    _within(f'{cid} forward vs the 3x3 layer', got, r.y0, _bf16_bound(4 * r.ci, 0, r.y_A, r.y0) + BF * r.y_Ax)
    assert r.guards_out


@pytest.mark.parametrize('res', [False, True], ids=['plain', 'dalias'])
@pytest.mark.parametrize('cid', IDS)
def test_data_gradient(cid, res):
    """(c) against the strided convolution with the composite operand, (e) against autograd of the original layer."""
    r = _run(cid)
    name, s = r.route_dxr if res else r.route_dx
    want_s = _igemm_split(r.B * r.H * r.W, r.ci, 16 * r.co)
    assert name == 'dma 64x64 st4 lw4 mode2' + (f' split{want_s}' if want_s > 1 else ''), (name, want_s)
    extra = _nchw(r.dal.double()) if res else 0.0
    got = _nchw((r.dxr if res else r.dx).float())
    s = s if s > 1 else 0
    _within(f'{cid} dx', got, r.gx + extra, _bf16_bound(16 * r.co, s, r.gx_A, r.gx + extra))
    _within(f'{cid} dx vs the 3x3 layer', got, r.gx0 + extra,
            _bf16_bound(16 * r.co, s, r.gx_A, r.gx0 + extra) + BF * r.gx_Ax)


@pytest.mark.parametrize('cid', IDS)
def test_weight_and_bias_gradient(cid):
    """(d): dW4 per element; the fold bit for bit from that dW4, overwriting and accumulating; dw and dbias in their
    pre-filled destinations against the composite definition and (e) autograd of the original layer."""
    r = _run(cid)
    ci, co, P = r.ci, r.co, r.P
    lay = lambda t: t.view(co, 3, 3, ci).permute(0, 3, 1, 2)
    assert [g.splits for g in r.wg] == [1] + ([2] if P.M >= 128 else [])
    for g in r.wg:
        what = f'{cid} splits {g.splits}'
        assert g.route == f'tr {64 if ci <= 64 else 128}x128 mode0', g.route
        s = g.splits if g.splits > 1 else 0
        dw4 = g.ws[0].clone()
        for k in range(1, g.splits):
            dw4 += g.ws[k]                                                    # fp32, split order
        dw4 = dw4.view(ci, 4, 4, co).permute(3, 0, 1, 2)                      # [co][ci][4][4]
        b4 = (P.M + s + 3) * U * r.g4_A + 4 * U * r.g4.abs()
        _within(f'{what} dW4', dw4, r.g4, b4)
        fold = kern.ups_fold(dw4.contiguous())                                # fp32, the kernel's order
        assert _same_bits(lay(g.dwv0).contiguous(), fold), f'{what}: fold (overwrite) is not the four-term fp32 sum'
        assert _same_bits(lay(g.dwv).contiguous(), PRE_W + fold), f'{what}: fold (accumulate) is not prefill + that sum'
        terms = kern.ups_fold(r.g4.abs() + b4)
        bw = kern.ups_fold(b4) + 4 * U * (PRE_W + terms)
        _within(f'{what} dw', lay(g.dwv), PRE_W + kern.ups_fold(r.g4), bw)
        _within(f'{what} dw vs the 3x3 layer', lay(g.dwv), PRE_W + r.gw0, bw)
        assert _same_bits(g.part.view(r.nblk, co), r.part_ref), f'{what}: bias partials differ from sdmi_rowgroup_sum'
    bb = (r.rows + r.nblk + 1) * U * r.gb_A + 4 * U * (PRE_B + r.gb).abs()
    _within(f'{cid} dbias', r.db, PRE_B + r.gb, bb)
    assert r.guards_out and r.inputs_kept
