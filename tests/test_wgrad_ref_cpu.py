"""No GPU: (1) the float64 reference of tests/wgrad_ref.py against torch.autograd of F.conv2d / F.linear in float64;
(2) the case table of tests/test_gpu_wgrad_pins.py against the library's host-side queries sdmi_wgrad_route /
sdmi_bwd_pair_route (no launch): every case passes the ABI's geometry checks and takes exactly the kernel instantiation
its entry names; (3) every instantiation the dispatchers of csrc/wgrad.hip and csrc/bwd_pair.hip can launch (read from
their source) is named by some case or listed as unreachable."""
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

from slotdiffusion_amd import _lib
from tests import test_gpu_wgrad_pins as G
from tests import wgrad_ref as R

CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), 'csrc')
P1 = (1, 1, 1, 1)
# (id, B, H, W, Cin, N, KH, KW, stride, (top, bottom, left, right), ups)
GEOMS = [
    ('1x1', 3, 4, 5, 4, 3, 1, 1, 1, (0, 0, 0, 0), 0),
    ('linear', 7, 1, 1, 5, 3, 1, 1, 1, (0, 0, 0, 0), 0),
    ('3x3same', 2, 4, 4, 3, 2, 3, 3, 1, P1, 0),
    ('5x5same', 2, 6, 6, 2, 3, 5, 5, 1, (2, 2, 2, 2), 0),
    ('1x3', 2, 3, 5, 2, 3, 1, 3, 1, (0, 0, 1, 1), 0),
    ('1x2p0001', 2, 3, 5, 2, 3, 1, 2, 1, (0, 0, 0, 1), 0),
    ('2x2p0', 2, 4, 4, 2, 3, 2, 2, 1, (0, 0, 0, 0), 0),
    ('2x2p0101', 2, 4, 4, 2, 3, 2, 2, 1, (0, 1, 0, 1), 0),
    ('4x4p1212', 2, 4, 4, 2, 3, 4, 4, 1, (1, 2, 1, 2), 0),
    ('3x3s2p0101', 2, 6, 6, 2, 3, 3, 3, 2, (0, 1, 0, 1), 0),
    ('3x3s2p1111', 2, 6, 6, 2, 3, 3, 3, 2, P1, 0),
    ('1x1s2', 2, 6, 6, 2, 3, 1, 1, 2, (0, 0, 0, 0), 0),
    ('2x2s2', 2, 6, 6, 2, 3, 2, 2, 2, (0, 0, 0, 0), 0),
    ('7x7s2p3', 1, 9, 9, 2, 2, 7, 7, 2, (3, 3, 3, 3), 0),
    ('ups3x3', 2, 3, 3, 2, 3, 3, 3, 1, P1, 1),
    ('3x3@5x5', 3, 5, 5, 2, 3, 3, 3, 1, P1, 0),
    ('3x3@6x10', 2, 6, 10, 2, 3, 3, 3, 1, P1, 0),
]


def _geom(t):
    _, B, H, W, Cin, N, KH, KW, stride, pad, ups = t
    Hv, Wv = (2 * H, 2 * W) if ups else (H, W)
    Ho = (Hv + pad[0] + pad[1] - KH) // stride + 1
    Wo = (Wv + pad[2] + pad[3] - KW) // stride + 1
    return types.SimpleNamespace(B=B, H=H, W=W, Cin=Cin, N=N, KH=KH, KW=KW, stride=stride, pad=pad, pad_t=pad[0],
                                 pad_l=pad[2], ups=ups, Ho=Ho, Wo=Wo)


def _autograd(g, x, w, dy):
    """dW [N, K], dX [B H W, Cin], dbias [N] of the forward of sdmi.h, by torch.autograd in float64."""
    x4 = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    w4 = w.view(g.N, g.KH, g.KW, g.Cin).permute(0, 3, 1, 2).clone().requires_grad_(True)
    b = torch.zeros(g.N, dtype=torch.float64, requires_grad=True)
    v = F.interpolate(x4, scale_factor=2, mode='nearest') if g.ups else x4
    v = F.pad(v, (g.pad[2], g.pad[3], g.pad[0], g.pad[1]))
    if g.H == g.W == g.KH == g.KW == 1:
        y = F.linear(x4.flatten(1), w4.flatten(1), b).view(g.B, g.N, 1, 1)
    else:
        y = F.conv2d(v, w4, b, stride=g.stride)
    assert y.shape == (g.B, g.N, g.Ho, g.Wo), (y.shape, g)
    y.backward(dy.view(g.B, g.Ho, g.Wo, g.N).permute(0, 3, 1, 2))
    return (w4.grad.permute(0, 2, 3, 1).reshape(g.N, -1), x4.grad.permute(0, 2, 3, 1).reshape(-1, g.Cin), b.grad)


@pytest.mark.parametrize('t', GEOMS, ids=lambda t: t[0])
def test_reference_matches_autograd_in_float64(t):
    g = _geom(t)
    gen = torch.Generator().manual_seed(len(t[0]) + g.B * g.H)
    x = torch.randn(g.B, g.H, g.W, g.Cin, generator=gen, dtype=torch.float64)
    w = torch.randn(g.N, g.KH * g.KW * g.Cin, generator=gen, dtype=torch.float64)
    dy = torch.randn(g.B * g.Ho * g.Wo, g.N, generator=gen, dtype=torch.float64)
    S, A0, sb, ab = R.wgrad_reference(x, dy, g)
    dw, dx, db = _autograd(g, x, w, dy)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(S, dw, **tol)
    torch.testing.assert_close(sb, db, **tol)
    # the sums of magnitudes are the same sums over the magnitudes of the operands
    dwa, dxa, dba = _autograd(g, x.abs(), w.abs(), dy.abs())
    torch.testing.assert_close(A0, dwa, **tol)
    torch.testing.assert_close(ab, dba, **tol)
    assert bool((A0 >= S.abs() * (1 - 1e-12)).all())
    if g.stride == 1 and not g.ups:
        Z, Az = R.dgrad_reference(dy, w, g)
        torch.testing.assert_close(Z, dx, **tol)
        torch.testing.assert_close(Az, dxa, **tol)


def test_flipped_operand_is_the_data_gradient_of_the_abi():
    """The operand the pair cases hand to the data gradient (sdmi.h: sdmi_pack_dgrad's layout), run as the FORWARD
    definition over dY with pad' = K - 1 - pad, equals the reference's dX."""
    for t in GEOMS:
        g = _geom(t)
        if g.stride != 1 or g.ups or (g.Ho, g.Wo) != (g.H, g.W):
            continue
        gen = torch.Generator().manual_seed(7)
        w = torch.randn(g.N, g.KH * g.KW * g.Cin, generator=gen, dtype=torch.float64)
        dy = torch.randn(g.B * g.Ho * g.Wo, g.N, generator=gen, dtype=torch.float64)
        wd = G.flipped_operand(w, g)
        d = types.SimpleNamespace(B=g.B, H=g.Ho, W=g.Wo, Cin=g.N, Ho=g.H, Wo=g.W, KH=g.KH, KW=g.KW, stride=1,
                                  pad_t=g.KH - 1 - g.pad_t, pad_l=g.KW - 1 - g.pad_l, ups=0)
        dx = torch.zeros(g.B * g.H * g.W, g.Cin, dtype=torch.float64)
        for kh in range(g.KH):
            for kw in range(g.KW):
                k0 = (kh * g.KW + kw) * g.N
                dx += R.tap(dy.view(g.B, g.Ho, g.Wo, g.N), d, kh, kw) @ wd[:, k0:k0 + g.N].t()
        torch.testing.assert_close(dx, R.dgrad_reference(dy, w, g)[0], rtol=1e-12, atol=1e-12)


# ---- the case table of the GPU file ------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.CASES, ids=lambda c: c.id)
def test_case_takes_the_route_it_names(c):
    for p in c.probs:
        assert p.M < 2 ** 24 - 16, 'exact arithmetic needs every sum below 2^24'
        r = _lib.query('sdmi_wgrad_route', **G.wgrad_fields(p))
        assert r >= 0, (c.id, _lib.lib().sdmi_last_error())         # the ABI's geometry checks
        assert r & 15 == _lib.query('sdmi_wgrad_kernel', **G.wgrad_fields(p))     # the family field
    if c.kind == 'single':
        assert G.wgrad_route(c.probs[0]) == c.route
    elif c.kind == 'group':
        # sdmi_wgrad_group's own requirements (wgrad.hip): one dtype, 1x1 / linear; bf16: N, K > 64
        assert 1 <= len(c.probs) <= 16 and len({p.dt for p in c.probs}) == 1
        assert c.route == ('group bf16' if c.probs[0].dt == G.BF16 else 'group f32')
        for p in c.probs:
            assert p.KH == p.KW == p.H == p.W == 1 and p.stride == 1 and p.pad == (0, 0, 0, 0) and not p.ups
            assert p.dt == G.F32 or (p.N > 64 and p.K > 64)
    elif c.kind == 'fold':
        assert all(p.splits > 1 and (p.N * p.K) % 4 == 0 for p in c.probs)
    else:
        assert G.pair_route(c) == c.route
        assert all(q.splits > 1 for q in c.probs[1:])


def test_the_case_table_has_what_the_issue_lists():
    """Edges the table must keep: empty slices, the XCD remap's three block counts, the folds on both sides of 64 splits,
    a carried pixel state, a persistent-workgroup walk in the pair."""
    by = {c.id: c for c in G.CASES}

    def blocks(p, tn, tk):
        return (-(-p.N // tn) * -(-p.K // tk) + (-(-p.N // tn) if p.bias else 0)) * p.splits

    def empty(p, mt):
        mps = -(-(-(-p.M // p.splits)) // mt) * mt
        return (p.splits - 1) * mps >= p.M
    assert blocks(by['lin130x40x24+2blocks'].probs[0], 64, 64) == 2
    assert blocks(by['lin200x50x200-s3+9blocks+acc'].probs[0], 64, 128) == 9
    assert blocks(by['lin1000x136x264-s3-nobias+18blocks'].probs[0], 128, 128) == 18
    assert empty(by['lin130x136x264-s4-emptyslice'].probs[0], 64)
    assert empty(by['f32-3x3@8-b2-c64-n512-s5-emptyslice'].probs[0], 32)
    assert empty(by['3x3@16-c64-n64-b64-s63'].probs[0], 64)
    splits = {p.splits for c in G.CASES for p in c.probs}
    assert {1, 63, 64, 128} <= splits
    p = by['3x3@6x10-b9-c32-n136-s2'].probs[0]
    assert (p.H & (p.H - 1)) and (p.W & (p.W - 1)) and p.M // p.splits > 64        # several steps of the carried state
    p = by['pair-cap64-lin2100x136x72-s3'].probs[0]
    assert by['pair-cap64-lin2100x136x72-s3'].cap == 64 and -(-p.M // 64) * -(-p.Cin // 64) > 64


def _source_instantiations():
    """Every kernel instantiation the dispatchers can launch, in the route names of the GPU file, from their source."""
    w = open(os.path.join(CSRC, 'wgrad.hip')).read()
    b = open(os.path.join(CSRC, 'bwd_pair.hip')).read()
    out = set()
    body = w[w.index('int dispatch_wgrad_bf16'):w.index('const char* wgrad_geometry_error')]
    modes = set(re.findall(r'launch_wgrad_tr<TN, TK, (\d)>', body))
    tiles = set(re.findall(r'WG_TR\((\d+), (\d+)\)', body)) - {('TN', 'TK')}
    assert modes and tiles
    out |= {f'tr {tn}x{tk} mode{m}' for tn, tk in tiles for m in modes}
    out |= {f'halo logw{v}' for v in re.findall(r'launch_wgrad3x3_halo<(\d)>\(a', body)}
    assert 'launch_wgrad3x3_c64(a, st)' in body
    out.add('c64')
    f32 = w[w.index('int dispatch_wgrad_f32'):w.index('WgradRoute select_wgrad_bf16')]
    out |= {f'f32 {tn}x{tk} {"1x1" if one == "true" else "conv"}'
            for tn, tk, one in re.findall(r'launch_wgrad<float, (\d+), (\d+), (true|false)>', f32)}
    assert not re.search(r'launch_wgrad<bf16_t|wgrad_kernel<bf16_t', w), 'the bf16 register-transpose kernel is dispatched again'
    assert 'wgrad_group_kernel, dim3(items)' in w and 'wgrad_group_f32_kernel, dim3(items)' in w
    out |= {'group bf16', 'group f32', 'fold group'}
    go = b[b.index('extern "C" int sdmi_bwd_pair('):b.index('extern "C" int sdmi_bwd_pair_route')]
    pmodes = set(re.findall(r'launch_pair<BM, BN, BKB, (\d), WT>', go))
    shapes = set(re.findall(r'PAIR_GO\((\d+), (\d+), (\d+), (\d+)\);', go))
    assert pmodes and shapes
    out |= {f'pair {bm}x{bn} kb{kb} mode{m} wt{wt}' for bm, bn, kb, wt in shapes for m in pmodes}
    return out


def test_every_dispatched_instantiation_is_covered_or_listed_unreachable():
    have = _source_instantiations()
    assert len(have) == 12 + 1 + 3 + 4 + 3 + 12, sorted(have)
    named = {c.route for c in G.CASES}
    assert named <= have, named - have
    missing = have - named - set(G.UNREACHABLE)
    assert not missing, f'no case reaches {sorted(missing)}'
    both = named & set(G.UNREACHABLE)
    assert not both, f'listed as unreachable but reached: {sorted(both)}'


def test_pair_route_fails_like_the_launcher():
    """sdmi_bwd_pair_route runs sdmi_bwd_pair's argument checks: a narrow data-gradient output and a 64-wide dW tile next
    to 128 x 128 data-gradient tiles are refused."""
    by = {c.id: c for c in G.CASES}
    c = by['pair-lin12288x256x264-s4']
    args, keep = G.pair_structs(types.SimpleNamespace(**{**vars(c), 'wt': 64}))
    assert _lib.query('sdmi_bwd_pair_route', **args) < 0
    assert b'sdmi_bwd_pair_route' in _lib.lib().sdmi_last_error() and b'wgrad_tile' in _lib.lib().sdmi_last_error()
    args, keep = G.pair_structs(by['pair-lin72x72-m130-wt128'])
    keep[0].N = 32
    assert _lib.query('sdmi_bwd_pair_route', **args) < 0
    assert _lib.query('sdmi_bwd_pair_route', dgrad=0, wgrad=0) < 0
