"""The weight-gradient kernels (csrc/wgrad.hip, wgrad_body.h) and the paired backward launch (bwd_pair.hip), called
through the C ABI with every field spelled out and pinned, element by element, to the float64 reference of
tests/wgrad_ref.py computed from the tensors the kernel read.  Every case states the kernel instantiation it is there
for; the host-side queries sdmi_wgrad_route / sdmi_bwd_pair_route (the launcher's own selection) must answer exactly that
instantiation, here before every launch and in tests/test_wgrad_ref_cpu.py without a GPU: when dispatch changes, the
case fails with "expected tr 128x64 mode2, got tr 128x64 mode0" instead of passing on another kernel.

Two tests per case:

  test_exact   dY and A in {-1, 0, 1}; where the case accumulates, the initial dW / dbias are random integers in
               [-16, 16].  Every product and every partial sum is an integer below M + 16 < 2^24, so the fp32 result is
               the integer reference in EVERY BIT for any summation order, split count and fold.  No tolerance.  (The
               pair's data gradient: the rows of the flipped operand carry at most 96 entries of +-1, bias / residual are
               integers: |dX| < 256 is exact in bf16.)
  test_pinned  Gaussian operands on the storage grid, dY scaled by 1/8.  Per element, no norms, no share of elements
               (U = 2^-24, BF = 2^-8):
                 dW      |dW - z| <= (M + s + 2) U A + 4 U |z|     z = init + S, A = |init| + A0 (wgrad_ref.py), s = the
                         number of partials a fold summed (0 without a split); bf16 products are exact in fp32, the + 2
                         covers the fp32 path's product rounding and the accumulate add
                 dbias   the same form with sb, ab
                 dX      (K_d + 3) U A_d + 4 U |z|, then BF (|z| + that) for the bf16 store (the forward file's bound)

Poison, checked in both tests.  Inputs hold 8192.0 in the pitch gaps (ldy > N, also where N is no multiple of the
16-byte vector; lda > Cin: a pixel pitch wider than the channels), in one guard row behind dY and in W + 1 guard pixels
before and after `a`.  Outputs hold -3.0: with accumulate = 0 every element of dW [N][K] and dbias [N] is overwritten,
64 guard floats before and after both stay untouched.  The workspace is exactly splits (N K + N) floats plus a tail of
1024: the tail stays untouched; with splits == 1 the whole workspace; with dbias == NULL the bias partials.  With
defer_fold = 1 dW / dbias are untouched after the launch and sdmi_wgrad_fold_group then gives the bits of the immediate
fold.  A second launch gives the same bits; all inputs are unchanged.  The pair: dX's pitch gap and guard rows too.

Routes and the cases that reach them (the id of a case lists its edges):
  tr 64x64 mode1 / 64x128 / 128x64 / 128x128     lin130x40x24 (2 blocks: fewer than 8), lin200x50x200-s3 (9 blocks),
                                                  lin70x136x64, lin1000x136x264-s4, lin130x136x264-s4-emptyslice,
                                                  lin1000x136x264-s3-nobias (18 blocks: r8 = 2 of the XCD remap)
  tr 64x128 / 128x128 / 64x64 / 128x64 mode2     3x3@8, 3x3@5x5-b7 (Ho Wo < 64), 3x3@6x10 (carried pixel state), 5x5p2,
                                                  1x3-n40, 1x3-n72, 2x2p0101@8, 4x4p1212@8, 3x3@16-c64-s63 (last
                                                  one-lane fold, empty slices)
  tr 64x128 / 128x64 / 64x64 / 128x128 mode0     3x3s2p1, 3x3s2p0101, 1x1s2-c32, 2x2s2-c16, 2x2p0@8 (not same-size),
                                                  7x7s2-n3, 7x7s2-n136, ups3x3
  c64                                             c64-1x8x64-s2, c64-2x12x64-s4 (6 tiles over 4 slots), c64-1x4x128-s2
                                                  (lda = ldy = 72), c64-nobias
  halo logw4 / 5 / 6                              halo16-b32 (one tile per slot), halo16-b40 (ragged), halo64x16,
                                                  halo16-nobias, halo32-b10, halo64-b3-n192-s24, halo16-c64-n128-s64 and
                                                  halo16-c64-n64-s128 (the 8-lane fold, wgrad_fold_lanes)
  f32 64x64 1x1 / conv, 128x128 1x1 / conv        f32-lin70x50x24, f32-lin448x192x576-s2, f32-3x3@5x5, f32-3x3s2,
                                                  f32-ups3x3, f32-lin200x512x512-s6, f32-3x3@8-n512-s5-emptyslice
  group bf16 / group f32                          group-bf16-5 (splits 1, 3, 64; with / without dbias; accumulate mixed),
                                                  group-f32-5 (N or K <= 64 among them), group-bf16-16tiny
  fold group                                      foldgroup-3 (three defer_fold launches folded in one call)
  pair BMxBN kbBKB modeMODE wtWT                  11 of the 12 instantiations: pair-lin72x72 (64x64 kb64 mode1, wt 128 /
                                                  64), pair-lin72x264 (kb128 mode1, wt 128 / 64), pair-3x3-c72-n128@8 (kb128
                                                  mode2, wt 128 / 64), pair-1x2-c72-n96@8 (kb64 mode2, wt 128 / 64),
                                                  pair-lin12288x256x264, pair-3x3-c256-n128-b48 and pair-1x2-c256-n96-b48
                                                  (128x128: kb128 mode1, kb128 mode2, kb64 mode2), pair-cap64 (99 dX tiles
                                                  on 64 persistent workgroups), pair-fold (an earlier launch's partials)

Instantiations the dispatchers contain that no argument set reaches, hence NOT covered (UNREACHABLE below; the CPU test
holds the list against the source):
  wgrad_tr_kernel<*, *, 0> as the fallback of `fits == false` (1x1 and same-size problems whose split spans 2 GB and
    more): the kernels themselves are covered through their general-gather cases;
  launch_wgrad<bf16_t, ...> / wgrad_kernel<bf16_t, ...>: no longer dispatched, not instantiated;
  bwd_pair_kernel<128, 128, 64, 1, 128>: 128 x 128 data-gradient tiles of a 1x1 problem need K_d > 256, which takes the
    128-byte K tile;  bwd_pair_kernel<128, 128, *, *, 64>: not instantiated (64-wide dW tiles only next to 64 x 64).
  (bwd_pair_kernel<*, *, 64, 2, *> IS reachable: a 1x2 filter with 96 output channels has K_d = 192 < 256.)
Out of scope: the data-gradient operand pack, the strided / ups data-gradient chains, fp8.

Beyond the issue's list: test_tail_rows_are_never_read (+inf instead of 8192 around the operands of six MODE 1 / 2
cases; its docstring says why finite poison cannot see a loader that lost its tail mask).

Measured on an MI355X, the largest share of its bound any element of a route used (NEED; dW / dbias):
  tr mode1   64x64 0.008 / 0.0003   64x128 0.005 / 0.0005   128x64 0.013 / 0.004    128x128 0.007 / 0.0001
  tr mode2   64x64 0.008 / 0.0002   64x128 0.006 / 0.0004   128x64 0.008 / 0.001    128x128 0.012 / 0.002
  tr mode0   64x64 0.025 / 0        64x128 0.009 / 0        128x64 0.022 / 0        128x128 0.009 / 0.002
  c64 0.002 / 0.0002     halo logw4 4.2e-5 / 7.7e-6     logw5 2.7e-5 / 1.6e-5     logw6 1.8e-5 / 5.8e-6
  f32 64x64 1x1 0.041 / 0.008    64x64 conv 0.017 / 0.002    128x128 1x1 0.010 / 0.002    128x128 conv 0.015 / 0.005
  group bf16 0.089 / 0.014 (the 16 tiny problems: M = 8 ...)     group f32 0.041 / 0.008     fold group 0.005 / 0.0006
  pair       dW at most 0.010 next to 64 x 64 tiles, 5e-5 at M = 12288; dbias at most 0.0012;
             dX 0.956 ... 0.9955 on every route (the bf16 store landing on half an ulp, as in the forward file)
No route needs more than its derived bound.  The bound grows with M while the measured error grows like sqrt(M), so
the pinned test is loose at large M (the halo rows): there the exact test carries the weight -- it has no tolerance."""
import ctypes
import math
import os
import types
import zlib

import pytest
import torch

from tests import wgrad_ref as R
from tests.test_gpu_bwd_helpers import (BF, DEV, U, _call, _dt, _end_the_session_on_a_gpu_fault,  # noqa: F401
                                        _gen, _L, _poison, _q, _same_bits, _worst)

pytestmark = pytest.mark.gpu

if 'SDMI_WGRAD_HALO' in os.environ:
    pytest.skip('SDMI_WGRAD_HALO set (read once per process): the routes asserted here are the default ones',
                allow_module_level=True)

F32, BF16 = torch.float32, torch.bfloat16
POISON_IN, POISON_OUT = 8192.0, -3.0
G = 64              # guard floats before and after dW / dbias
WS_TAIL = 1024
NEED = {}           # '<route> dW | dbias | dX' -> the largest err / bound share so far (test_pinned records and prints it)

UNREACHABLE = {
    'tr * mode0 as the fits == false fallback of a 1x1 / same-size problem': 'operands of 2 GB and more',
    'launch_wgrad<bf16_t>': 'no longer dispatched',
    'pair 128x128 kb64 mode1 wt128': 'big tiles of a 1x1 problem need K_d > 256: the 128-byte K tile',
}


# ---- problems and cases ------------------------------------------------------------------------------------
_PD = dict(dt=BF16, B=1, H=1, W=1, Cin=0, N=0, kh=1, kw=1, stride=1, pad=(0, 0, 0, 0), ups=0, splits=1, bias=True,
           acc=False, lda_pad=None, ldy_pad=None)


def prob(M=None, K=None, **kw):
    """One weight-gradient problem.  M, K: a linear problem (H = W = 1).  pad = (top, bottom, left, right); bias: pass
    dbias; acc: accumulate; *_pad: elements between the row and its pitch (default: one 16-byte vector)."""
    bad = set(kw) - set(_PD)
    assert not bad, bad
    p = types.SimpleNamespace(**{**_PD, **kw})
    if M is not None:
        p.B, p.Cin = M, K
    p.vec = 8 if p.dt == BF16 else 4
    p.KH, p.KW = p.kh, p.kw
    Hv, Wv = (2 * p.H, 2 * p.W) if p.ups else (p.H, p.W)
    p.Ho = (Hv + p.pad[0] + p.pad[1] - p.KH) // p.stride + 1
    p.Wo = (Wv + p.pad[2] + p.pad[3] - p.KW) // p.stride + 1
    p.pad_t, p.pad_l = p.pad[0], p.pad[2]
    p.M = p.B * p.Ho * p.Wo
    p.K = p.KH * p.KW * p.Cin
    p.lda = p.Cin + (p.vec if p.lda_pad is None else p.lda_pad)
    p.ldy = -(-p.N // p.vec) * p.vec + (p.vec if p.ldy_pad is None else p.ldy_pad)
    p.gkey = (p.dt, p.B, p.H, p.W, p.Cin, p.N, p.KH, p.KW, p.stride, p.pad, p.ups)
    return p


def wgrad_fields(p):
    """Every non-pointer field of SdmiWgradArgs."""
    return dict(dtype=_dt(p.dt), M=p.M, N=p.N, K=p.K, lda=p.lda, ldy=p.ldy, B=p.B, H=p.H, W=p.W, Cin=p.Cin, Ho=p.Ho,
                Wo=p.Wo, KH=p.KH, KW=p.KW, stride=p.stride, pad_t=p.pad_t, pad_l=p.pad_l, ups=p.ups, splits=p.splits,
                accumulate=int(p.acc), defer_fold=0)


def dgrad_fields(p):
    """Every non-pointer field of the SdmiGemmArgs of p's data gradient (stride 1): a = dY, w = the flipped operand
    [Cin][KH KW N], out = dX [B H W][ldc]."""
    return dict(dtype=_dt(BF16), out_dtype=_dt(BF16), M=p.B * p.H * p.W, N=p.Cin, K=p.KH * p.KW * p.N, lda=p.ldy,
                ldw=p.KH * p.KW * p.N, ldc=p.Cin + 8, ldr=p.Cin + 16, B=p.B, H=p.Ho, W=p.Wo, Cin=p.N, Ho=p.H, Wo=p.W,
                KH=p.KH, KW=p.KW, stride=1, pad_t=p.KH - 1 - p.pad_t, pad_l=p.KW - 1 - p.pad_l, ups=0, act=0, alpha=1.0,
                split_k=1, batch=1)


CASES = []


def _add(cid, kind, route, probs, **kw):
    """kind: 'single' (sdmi_wgrad), 'group' (sdmi_wgrad_group), 'fold' (defer_fold launches + sdmi_wgrad_fold_group),
    'pair' (sdmi_bwd_pair; probs[0] is the layer, probs[1], if any, the earlier launch whose partials it folds)."""
    c = types.SimpleNamespace(id=cid, kind=kind, route=route, probs=probs, wt=0, cap=0, dbias_d=False,
                              res=False)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    CASES.append(c)


def _single(cid, route, M=None, K=None, **kw):
    _add(cid, 'single', route, [prob(M, K, **kw)])


def _build_cases():
    P1 = (1, 1, 1, 1)
    # ---- bf16 wgrad_tr<TN, TK, 1>: 1x1 / linear
    _single('lin130x40x24+2blocks', 'tr 64x64 mode1', M=130, N=40, K=24)
    _single('lin200x50x200-s3+9blocks+acc', 'tr 64x128 mode1', M=200, N=50, K=200, splits=3, acc=True)
    _single('lin70x136x64+acc', 'tr 128x64 mode1', M=70, N=136, K=64, acc=True)
    _single('lin1000x136x264-s4', 'tr 128x128 mode1', M=1000, N=136, K=264, splits=4)
    _single('lin130x136x264-s4-emptyslice', 'tr 128x128 mode1', M=130, N=136, K=264, splits=4)
    _single('lin1000x136x264-s3-nobias+18blocks', 'tr 128x128 mode1', M=1000, N=136, K=264, splits=3, bias=False)
    # ---- bf16 wgrad_tr<TN, TK, 2>: stride-1 same-size, not 1x1
    _single('3x3@8-b3-c16-n24', 'tr 64x128 mode2', B=3, H=8, W=8, Cin=16, N=24, kh=3, kw=3, pad=P1)
    _single('3x3@5x5-b7-c8-n72-s2', 'tr 128x128 mode2', B=7, H=5, W=5, Cin=8, N=72, kh=3, kw=3, pad=P1, splits=2)
    _single('3x3@6x10-b2-c32-n136+acc', 'tr 128x128 mode2', B=2, H=6, W=10, Cin=32, N=136, kh=3, kw=3, pad=P1, acc=True)
    _single('3x3@6x10-b9-c32-n136-s2', 'tr 128x128 mode2', B=9, H=6, W=10, Cin=32, N=136, kh=3, kw=3, pad=P1, splits=2)
    _single('5x5p2@9-c8-n40', 'tr 64x128 mode2', B=2, H=9, W=9, Cin=8, N=40, kh=5, kw=5, pad=(2, 2, 2, 2))
    _single('1x3-c8-n40', 'tr 64x64 mode2', B=3, H=6, W=7, Cin=8, N=40, kh=1, kw=3, pad=(0, 0, 1, 1))
    _single('1x3-c8-n72', 'tr 128x64 mode2', B=3, H=6, W=7, Cin=8, N=72, kh=1, kw=3, pad=(0, 0, 1, 1))
    _single('2x2p0101@8-c16-n24', 'tr 64x64 mode2', B=2, H=8, W=8, Cin=16, N=24, kh=2, kw=2, pad=(0, 1, 0, 1))
    _single('4x4p1212@8-c8-n24-s2', 'tr 64x128 mode2', B=3, H=8, W=8, Cin=8, N=24, kh=4, kw=4, pad=(1, 2, 1, 2), splits=2)
    _single('3x3@16-c64-n64-b64-s63', 'tr 64x128 mode2', B=64, H=16, W=16, Cin=64, N=64, kh=3, kw=3, pad=P1, splits=63)
    # ---- bf16 wgrad_tr<TN, TK, 0>: general gather
    _single('3x3s2p1@16-c16-n24', 'tr 64x128 mode0', B=2, H=16, W=16, Cin=16, N=24, kh=3, kw=3, stride=2, pad=P1)
    _single('3x3s2p0101@16-c16-n24-s2', 'tr 64x128 mode0', B=2, H=16, W=16, Cin=16, N=24, kh=3, kw=3, stride=2,
            pad=(0, 1, 0, 1), splits=2)
    _single('1x1s2@8-c32-n72', 'tr 128x64 mode0', B=3, H=8, W=8, Cin=32, N=72, stride=2)
    _single('2x2s2@8-c16-n40', 'tr 64x64 mode0', B=3, H=8, W=8, Cin=16, N=40, kh=2, kw=2, stride=2)
    _single('2x2p0@8-c16-n24', 'tr 64x64 mode0', B=2, H=8, W=8, Cin=16, N=24, kh=2, kw=2)
    _single('7x7s2p3@15-c8-n3', 'tr 64x128 mode0', B=2, H=15, W=15, Cin=8, N=3, kh=7, kw=7, stride=2, pad=(3, 3, 3, 3))
    _single('7x7s2p3@15-c8-n136-s2+acc', 'tr 128x128 mode0', B=2, H=15, W=15, Cin=8, N=136, kh=7, kw=7, stride=2,
            pad=(3, 3, 3, 3), splits=2, acc=True)
    _single('ups3x3@4-c16-n24', 'tr 64x128 mode0', B=3, H=4, W=4, Cin=16, N=24, kh=3, kw=3, pad=P1, ups=1)
    # ---- wgrad3x3_c64_kernel (lda = ldy = 72)
    c64 = dict(Cin=64, N=64, kh=3, kw=3, pad=P1)
    _single('c64-1x8x64-s2', 'c64', B=1, H=8, W=64, splits=2, **c64)
    _single('c64-2x12x64-s4+acc', 'c64', B=2, H=12, W=64, splits=4, acc=True, **c64)
    _single('c64-1x4x128-s2', 'c64', B=1, H=4, W=128, splits=2, **c64)
    _single('c64-1x8x64-s2-nobias', 'c64', B=1, H=8, W=64, splits=2, bias=False, **c64)
    # ---- wgrad3x3_halo_kernel<4 | 5 | 6>
    h = dict(kh=3, kw=3, pad=P1)
    _single('halo16-b32-c128-n128-s32', 'halo logw4', B=32, H=16, W=16, Cin=128, N=128, splits=32, **h)
    _single('halo16-b40-c128-n128-s32+acc', 'halo logw4', B=40, H=16, W=16, Cin=128, N=128, splits=32, acc=True, **h)
    _single('halo16-b32-c128-n128-s32-nobias', 'halo logw4', B=32, H=16, W=16, Cin=128, N=128, splits=32, bias=False, **h)
    _single('halo64x16-b8-c128-n128-s32', 'halo logw4', B=8, H=64, W=16, Cin=128, N=128, splits=32, **h)
    _single('halo32-b10-c128-n128-s32', 'halo logw5', B=10, H=32, W=32, Cin=128, N=128, splits=32, **h)
    _single('halo64-b3-c128-n192-s24', 'halo logw6', B=3, H=64, W=64, Cin=128, N=192, splits=24, **h)
    _single('halo16-b64-c64-n128-s64+acc', 'halo logw4', B=64, H=16, W=16, Cin=64, N=128, splits=64, acc=True, **h)
    _single('halo16-b128-c64-n64-s128', 'halo logw4', B=128, H=16, W=16, Cin=64, N=64, splits=128, **h)
    # ---- fp32 wgrad_kernel<float, 64 | 128, ., is1x1>
    _single('f32-lin70x50x24', 'f32 64x64 1x1', dt=F32, M=70, N=50, K=24)
    _single('f32-lin448x192x576-s2+acc', 'f32 64x64 1x1', dt=F32, M=448, N=192, K=576, splits=2, acc=True)
    _single('f32-3x3@5x5-b7-c8-n40', 'f32 64x64 conv', dt=F32, B=7, H=5, W=5, Cin=8, N=40, kh=3, kw=3, pad=P1)
    _single('f32-3x3s2p0101@16-c8-n24-s2', 'f32 64x64 conv', dt=F32, B=2, H=16, W=16, Cin=8, N=24, kh=3, kw=3, stride=2,
            pad=(0, 1, 0, 1), splits=2)
    _single('f32-ups3x3@4-c8-n24+acc', 'f32 64x64 conv', dt=F32, B=3, H=4, W=4, Cin=8, N=24, kh=3, kw=3, pad=P1, ups=1,
            acc=True)
    _single('f32-lin200x512x512-s6', 'f32 128x128 1x1', dt=F32, M=200, N=512, K=512, splits=6)
    _single('f32-3x3@8-b2-c64-n512-s5-emptyslice', 'f32 128x128 conv', dt=F32, B=2, H=8, W=8, Cin=64, N=512, kh=3, kw=3,
            pad=P1, splits=5)
    # ---- sdmi_wgrad_group
    _add('group-bf16-5', 'group', 'group bf16',
         [prob(130, 72, N=72), prob(200, 264, N=136, splits=3, bias=False, acc=True),
          prob(4200, 136, N=72, splits=64, acc=True), prob(70, 72, N=264, bias=False, acc=True),
          prob(1000, 72, N=136, splits=3)])
    _add('group-f32-5', 'group', 'group f32',
         [prob(70, 24, N=50, dt=F32), prob(200, 136, N=192, dt=F32, splits=3, bias=False, acc=True),
          prob(2100, 200, N=40, dt=F32, splits=64, acc=True), prob(130, 64, N=72, dt=F32, bias=False, acc=True),
          prob(448, 72, N=136, dt=F32, splits=3)])
    _add('group-bf16-16tiny', 'group', 'group bf16',
         [prob(8 + 9 * i, 72 + 8 * (i % 3), N=72 + 8 * (i % 2), bias=bool(i % 2), acc=bool(i % 3 == 0)) for i in range(16)])
    # ---- sdmi_wgrad_fold_group
    _add('foldgroup-3', 'fold', 'fold group',
         [prob(200, 200, N=50, splits=3, acc=True), prob(B=7, H=5, W=5, Cin=8, N=72, kh=3, kw=3, pad=P1, splits=2),
          prob(448, 136, N=72, dt=F32, splits=5, bias=False, acc=True)])
    # ---- sdmi_bwd_pair (the layer's weight gradient is probs[0]; its data gradient follows from it)
    for wt in (128, 64):
        _add(f'pair-lin72x72-m130-wt{wt}', 'pair', f'pair 64x64 kb64 mode1 wt{wt}',
             [prob(130, 72, N=72, splits=2, acc=True)], wt=wt, dbias_d=True, res=True)
        _add(f'pair-lin72x264-m130-wt{wt}', 'pair', f'pair 64x64 kb128 mode1 wt{wt}', [prob(130, 72, N=264)], wt=wt,
             res=(wt == 64))
        _add(f'pair-3x3-c72-n128@8-wt{wt}', 'pair', f'pair 64x64 kb128 mode2 wt{wt}',
             [prob(B=3, H=8, W=8, Cin=72, N=128, kh=3, kw=3, pad=P1, splits=2, bias=(wt == 128))], wt=wt,
             dbias_d=(wt == 64), res=True)
        _add(f'pair-1x2-c72-n96@8-wt{wt}', 'pair', f'pair 64x64 kb64 mode2 wt{wt}',
             [prob(B=3, H=8, W=8, Cin=72, N=96, kh=1, kw=2, pad=(0, 0, 0, 1), acc=True)], wt=wt, dbias_d=True)
    _add('pair-lin12288x256x264-s4', 'pair', 'pair 128x128 kb128 mode1 wt128',
         [prob(12288, 256, N=264, splits=4, acc=True)], res=True)
    _add('pair-3x3-c256-n128-b48@16-s4', 'pair', 'pair 128x128 kb128 mode2 wt128',
         [prob(B=48, H=16, W=16, Cin=256, N=128, kh=3, kw=3, pad=P1, splits=4)], dbias_d=True)
    _add('pair-1x2-c256-n96-b48@16-s3', 'pair', 'pair 128x128 kb64 mode2 wt128',
         [prob(B=48, H=16, W=16, Cin=256, N=96, kh=1, kw=2, pad=(0, 0, 0, 1), splits=3, bias=False)], res=True)
    _add('pair-cap64-lin2100x136x72-s3', 'pair', 'pair 64x64 kb64 mode1 wt128', [prob(2100, 136, N=72, splits=3)],
         cap=64, res=True)
    _add('pair-fold-lin130x72x72', 'pair', 'pair 64x64 kb64 mode1 wt128',
         [prob(130, 72, N=72, splits=2), prob(200, 200, N=50, splits=3, acc=True)], dbias_d=True)


_build_cases()
assert len({c.id for c in CASES}) == len(CASES)


# ---- routes -------------------------------------------------------------------------------------------------
def route_name(r):
    """Decode sdmi_wgrad_route (sdmi.h)."""
    E = _L().ENUMS
    fam, tn, tk, mode, logw = r & 15, (r >> 4 & 7) * 64, (r >> 7 & 7) * 64, r >> 10 & 3, r >> 12 & 7
    return {E['SDMI_WGRAD_KERNEL_IGEMM']: f'tr {tn}x{tk} mode{mode}', E['SDMI_WGRAD_KERNEL_C64']: 'c64',
            E['SDMI_WGRAD_KERNEL_HALO']: f'halo logw{logw}',
            E['SDMI_WGRAD_KERNEL_F32_T64']: f'f32 {tn}x{tk} {"1x1" if mode else "conv"}',
            E['SDMI_WGRAD_KERNEL_F32_T128']: f'f32 {tn}x{tk} {"1x1" if mode else "conv"}'}.get(fam, f'family {fam}?')


def pair_route_name(r):
    """Decode sdmi_bwd_pair_route (sdmi.h)."""
    return f'pair {(r & 7) * 64}x{(r >> 3 & 7) * 64} kb{(r >> 6 & 7) * 64} mode{r >> 9 & 3} wt{(r >> 12 & 7) * 64}'


def wgrad_route(p):
    r = _L().query('sdmi_wgrad_route', **wgrad_fields(p))
    assert r >= 0, _L().lib().sdmi_last_error()
    return route_name(r)


def pair_structs(c, ptr=None):
    """The three argument structs of a pair case; ptr: {field: address} (default: 16 everywhere the ABI wants a pointer --
    the route query dereferences nothing)."""
    S, p = _L().CSTRUCT, c.probs[0]
    ptr = ptr or {}
    d, w = S['SdmiGemmArgs'](), S['SdmiWgradArgs']()
    dk = dict(dgrad_fields(p), a=ptr.get('dy', 16), w=ptr.get('wd', 16), out=ptr.get('dx', 16),
              bias=ptr.get('bias_d', 16) if c.dbias_d else 0, residual=ptr.get('res', 16) if c.res else 0)
    wk = dict(wgrad_fields(p), a=ptr.get('a', 16), dy=ptr.get('dy', 16), dw=ptr.get('dw', 16),
              dbias=ptr.get('db', 16) if p.bias else 0, workspace=ptr.get('ws', 16), defer_fold=1)
    for s, kw in ((d, dk), (w, wk)):
        for k, v in kw.items():
            setattr(s, k, v)
    f = None
    if len(c.probs) > 1:
        q = c.probs[1]
        f = S['SdmiWgradArgs']()
        for k, v in dict(dw=ptr.get('fdw', 32), dbias=(ptr.get('fdb', 32) if q.bias else 0), workspace=ptr.get('fws', 32),
                         N=q.N, K=q.K, splits=q.splits, accumulate=int(q.acc)).items():
            setattr(f, k, v)
    args = dict(dgrad=ctypes.addressof(d), wgrad=ctypes.addressof(w), fold=ctypes.addressof(f) if f is not None else 0,
                dgrad_cap=c.cap, wgrad_tile=c.wt)
    return args, (d, w, f)


def pair_route(c):
    args, keep = pair_structs(c)
    r = _L().query('sdmi_bwd_pair_route', **args)
    assert r >= 0, _L().lib().sdmi_last_error()
    return pair_route_name(r)


# ---- operands and references -----------------------------------------------------------------------------------
def _seed(p, salt):
    return zlib.crc32(repr((p.gkey, salt)).encode())


def operands(p, exact):
    """CPU fp32 tensors on the storage grid: x [B, H, W, Cin], dy [M, N], initial dW [N, K] and dbias [N]."""
    g = _gen(_seed(p, exact))
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        return ri(-1, 1, p.B, p.H, p.W, p.Cin), ri(-1, 1, p.M, p.N), ri(-16, 16, p.N, p.K), ri(-16, 16, p.N)
    rn = lambda *s: torch.randn(*s, generator=g)
    return _q(rn(p.B, p.H, p.W, p.Cin), p.dt), _q(rn(p.M, p.N) / 8, p.dt), rn(p.N, p.K), rn(p.N)


_REF = {}


def reference(p, exact):
    """(operands, (S, A0, sb, ab)) of wgrad_ref.py, computed once per (geometry, exact); the last few are kept."""
    key = (p.gkey, exact)
    if key not in _REF:
        ops = operands(p, exact)
        while len(_REF) >= 6:
            _REF.pop(next(iter(_REF)))
        _REF[key] = (ops, R.wgrad_reference(ops[0], ops[1], p, with_abs=not exact))
    return _REF[key]


def pair_operands(p, exact):
    """The data gradient's own operands: W [N, K] (K = (kh, kw, ci)), bias [Cin] fp32, residual [B H W, Cin] (bf16 grid)."""
    g = _gen(_seed(p, ('pair', exact)))
    if exact:
        # at most 96 entries of +-1 per row of the flipped operand (fixed ci: over (kh, kw, n))
        taps, nnz = p.KH * p.KW, min(96, p.KH * p.KW * p.N)
        idx = torch.rand(p.Cin, taps * p.N, generator=g).topk(nnz, dim=1).indices
        sign = torch.randint(0, 2, idx.shape, generator=g).float() * 2 - 1
        wf = torch.zeros(p.Cin, taps * p.N).scatter_(1, idx, sign).view(p.Cin, taps, p.N)      # [ci][tap][n]
        w = wf.permute(2, 1, 0).reshape(p.N, p.K).contiguous()
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        return w, ri(-8, 8, p.Cin), ri(-16, 16, p.B * p.H * p.W, p.Cin)
    rn = lambda *s: torch.randn(*s, generator=g)
    return _q(rn(p.N, p.K) / math.sqrt(p.K), BF16), rn(p.Cin) * 0.5, _q(rn(p.B * p.H * p.W, p.Cin), BF16)


def flipped_operand(w, p):
    """sdmi.h: dst[ci][kh'][kw'][co] = src[co][KH-1-kh'][KW-1-kw'][ci]."""
    w4 = w.view(p.N, p.KH, p.KW, p.Cin).flip(1, 2)
    return w4.permute(3, 1, 2, 0).reshape(p.Cin, p.KH * p.KW * p.N).contiguous()


# ---- buffers ------------------------------------------------------------------------------------------------
class _Mat:
    """A flat device buffer full of `fill` with a [rows, ld] matrix `front` elements in; .ptr addresses the matrix."""

    def __init__(self, rows, ld, dtype, fill, front, tail, data=None):
        self.rows, self.ld, self.front = rows, ld, front
        self.flat = _poison((front + rows * ld + tail,), dtype, fill)
        self.ptr = self.flat.data_ptr() + front * self.flat.element_size()
        if data is not None:
            self.mat()[:, :data.shape[1]] = data.to(dtype).to(DEV)

    def mat(self, flat=None):
        return (self.flat if flat is None else flat)[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)


class _Inputs:
    """a: W + 1 guard pixels of 8192 before and after, pixel pitch lda > Cin; dy: pitch ldy > N, one guard row behind.
    (extra, fill: that many more guard pixels / rows, of another value -- test_tail_rows_are_never_read.)"""

    def __init__(self, p, x, dy, extra=0, fill=POISON_IN):
        gp = (p.W + 1 + extra) * p.lda
        self.a = _Mat(p.B * p.H * p.W, p.lda, p.dt, fill, gp, gp, x.reshape(-1, p.Cin))
        self.dy = _Mat(p.M, p.ldy, p.dt, fill, 0, (1 + extra) * p.ldy, dy)
        self.all = [self.a, self.dy]
        self.before = None

    def snapshot(self):
        self.before = [m.flat.clone() for m in self.all]

    def unchanged(self):
        return all(_same_bits(m.flat, b) for m, b in zip(self.all, self.before))


class _Out:
    """dW [N][K] and dbias [N] between G guard floats of -3 (holding the initial values where the case accumulates,
    -3 otherwise) and a workspace of exactly splits (N K + N) floats + a tail, all -3."""

    def __init__(self, p, init_dw, init_db):
        self.p = p
        self.dw = _Mat(p.N, p.K, F32, POISON_OUT, G, G, init_dw if p.acc else None)
        self.db = _Mat(1, p.N, F32, POISON_OUT, G, G, init_db[None] if p.acc else None)
        self.ws_n = p.splits * (p.N * p.K + p.N) if p.splits > 1 else 0
        self.ws = _poison((self.ws_n + WS_TAIL,), F32, POISON_OUT)
        self.start = [self.dw.flat.clone(), self.db.flat.clone()]

    def ptrs(self):
        return dict(dw=self.dw.ptr, dbias=self.db.ptr if self.p.bias else 0, workspace=self.ws.data_ptr())

    def untouched(self):
        return _same_bits(self.dw.flat, self.start[0]) and _same_bits(self.db.flat, self.start[1])

    def same_as(self, o):
        return _same_bits(self.dw.flat, o.dw.flat) and _same_bits(self.db.flat, o.db.flat)

    def check_around(self, cid, folded=True):
        """Guards, the workspace tail, the bias partials without dbias, dbias itself without dbias."""
        p = self.p
        for what, m, n in (('dW', self.dw, p.N * p.K), ('dbias', self.db, p.N)):
            f = m.flat.cpu()
            pois = torch.full((G,), POISON_OUT)
            assert _same_bits(f[:G], pois) and _same_bits(f[G + n:], pois), f'{cid}: guard floats around {what} written'
        ws = self.ws.cpu()
        tail = ws[self.ws_n:]
        assert _same_bits(tail, torch.full_like(tail, POISON_OUT)), \
            f'{cid}: workspace written past splits * (N K + N) floats (splits = {p.splits})'
        if not p.bias:
            assert _same_bits(self.db.flat, self.start[1]), f'{cid}: dbias written although the case passes none'
            part = ws[p.splits * p.N * p.K:self.ws_n]
            assert _same_bits(part, torch.full_like(part, POISON_OUT)), f'{cid}: bias partials written without dbias'


def fold_group(outs):
    rows = [dict(o.ptrs(), N=o.p.N, K=o.p.K, splits=o.p.splits, accumulate=int(o.p.acc)) for o in outs]
    arr = _L().struct_array('SdmiWgradArgs', rows)
    _call('sdmi_wgrad_fold_group', problems=ctypes.addressof(arr), n=len(rows))
    torch.cuda.synchronize()


# ---- checks against the reference --------------------------------------------------------------------------------
def check_numbers(cid, route, p, out, exact):
    """dW and dbias of one problem against the reference: every bit (exact) or the derived bound (module docstring)."""
    (x, dy, i_dw, i_db), (S, A0, sb, ab) = reference(p, exact)
    s = p.splits if p.splits > 1 else 0
    got_w = out.dw.mat().cpu()
    got_b = out.db.mat().cpu()[0]
    parts = [('dW', got_w, S, A0, i_dw)] + ([('dbias', got_b, sb, ab, i_db)] if p.bias else [])
    for what, got, z, A, init in parts:
        if p.acc:
            z = z + init.double()
        if exact:
            assert float(z.abs().max()) < 2.0 ** 24
            want = z.float()
            if not _same_bits(got, want):
                bad = (got.double() != z).reshape(-1).nonzero()
                i = int(bad[0])
                raise AssertionError(f'{cid} ({route}): {len(bad)} elements of {what} differ, first at flat index {i}: '
                                     f'got {float(got.reshape(-1)[i])}, exact {float(z.reshape(-1)[i])}')
            continue
        if p.acc:
            A = A + init.double().abs()
        assert bool(torch.isfinite(got).all()), (cid, what)
        err = (got.double() - z).abs()
        bound = (p.M + s + 2) * U * A + 4 * U * z.abs()
        share = float((err / bound.clamp_min(1e-300)).max())
        key = f'{route} {what}'
        NEED[key] = max(NEED.get(key, 0.0), share)
        print(f'{cid}: {route}, {what}: largest err/bound {share:.3f}')
        assert bool((err <= bound).all()), f'{cid} ({route}) {what}: {_worst(err, bound)}'


def _launch_wgrad(p, ins, out, **kw):
    _call('sdmi_wgrad', a=ins.a.ptr, dy=ins.dy.ptr, **out.ptrs(), **{**wgrad_fields(p), **kw})
    torch.cuda.synchronize()


# ---- the four kinds of case ----------------------------------------------------------------------------------------
def run_single(c, exact):
    p = c.probs[0]
    got = wgrad_route(p)
    assert got == c.route, f'{c.id}: expected {c.route}, got {got}'
    (x, dy, i_dw, i_db), _ = reference(p, exact)
    ins = _Inputs(p, x, dy)
    ins.snapshot()
    out = _Out(p, i_dw, i_db)
    _launch_wgrad(p, ins, out)
    out.check_around(c.id)
    check_numbers(c.id, c.route, p, out, exact)
    # repeatability
    out2 = _Out(p, i_dw, i_db)
    _launch_wgrad(p, ins, out2)
    assert out2.same_as(out), f'{c.id}: a second launch gave other bits'
    if p.splits > 1:
        out3 = _Out(p, i_dw, i_db)
        _launch_wgrad(p, ins, out3, defer_fold=1)
        assert out3.untouched(), f'{c.id}: the defer_fold launch wrote dW / dbias'
        fold_group([out3])
        assert out3.same_as(out), f'{c.id}: defer_fold + sdmi_wgrad_fold_group differs from the immediate fold'
        out3.check_around(c.id)
    assert ins.unchanged(), f'{c.id}: the launch changed its inputs'


def run_group(c, exact):
    assert all(wgrad_route(p).endswith('1x1') or wgrad_route(p).endswith('mode1') for p in c.probs)
    refs = [reference(p, exact)[0] for p in c.probs]
    ins = [_Inputs(p, x, dy) for p, (x, dy, _, _) in zip(c.probs, refs)]
    for i in ins:
        i.snapshot()

    def go():
        outs = [_Out(p, r[2], r[3]) for p, r in zip(c.probs, refs)]
        rows = [dict(wgrad_fields(p), a=i.a.ptr, dy=i.dy.ptr, **o.ptrs()) for p, i, o in zip(c.probs, ins, outs)]
        arr = _L().struct_array('SdmiWgradArgs', rows)
        _call('sdmi_wgrad_group', problems=ctypes.addressof(arr), n=len(rows))
        torch.cuda.synchronize()
        return outs
    outs = go()
    for j, (p, o) in enumerate(zip(c.probs, outs)):
        o.check_around(f'{c.id}[{j}]')
        check_numbers(f'{c.id}[{j}]', c.route, p, o, exact)
    assert all(a.same_as(b) for a, b in zip(go(), outs)), f'{c.id}: a second launch gave other bits'
    assert all(i.unchanged() for i in ins), f'{c.id}: the launch changed its inputs'


def run_fold(c, exact):
    outs, inss = [], []
    for p in c.probs:
        (x, dy, i_dw, i_db), _ = reference(p, exact)
        ins, out = _Inputs(p, x, dy), _Out(p, i_dw, i_db)
        ins.snapshot()
        _launch_wgrad(p, ins, out, defer_fold=1)
        assert out.untouched(), f'{c.id}: the defer_fold launch wrote dW / dbias'
        outs.append(out)
        inss.append(ins)
    fold_group(outs)
    for j, (p, o) in enumerate(zip(c.probs, outs)):
        o.check_around(f'{c.id}[{j}]')
        check_numbers(f'{c.id}[{j}]', c.route, p, o, exact)
    assert all(i.unchanged() for i in inss), f'{c.id}: the launches changed their inputs'


def run_pair(c, exact):
    p = c.probs[0]
    got = pair_route(c)
    assert got == c.route, f'{c.id}: expected {c.route}, got {got}'
    (x, dy, i_dw, i_db), _ = reference(p, exact)
    w, bias_d, res = pair_operands(p, exact)
    d = dgrad_fields(p)
    Mx = d['M']
    ins = _Inputs(p, x, dy)
    wd = _Mat(p.Cin, d['ldw'], BF16, POISON_IN, 0, d['ldw'], flipped_operand(w, p))
    bd = _Mat(1, p.Cin, F32, POISON_IN, 4, 4, bias_d[None])
    rs = _Mat(Mx, d['ldr'], BF16, POISON_IN, 0, d['ldr'], res)
    ins.all += [wd, bd, rs]
    ins.snapshot()
    # the earlier launch whose partials this one folds
    fout = None
    if len(c.probs) > 1:
        q = c.probs[1]
        (qx, qdy, q_dw, q_db), _ = reference(q, exact)
        qin = _Inputs(q, qx, qdy)
        fout = _Out(q, q_dw, q_db)
        _launch_wgrad(q, qin, fout, defer_fold=1)
        assert fout.untouched()

    def go(fo):
        out = _Out(p, i_dw, i_db)
        dx = _Mat(Mx, d['ldc'], BF16, POISON_OUT, d['ldc'], d['ldc'])
        ptr = dict(a=ins.a.ptr, dy=ins.dy.ptr, wd=wd.ptr, dx=dx.ptr, bias_d=bd.ptr, res=rs.ptr, dw=out.dw.ptr,
                   db=out.db.ptr, ws=out.ws.data_ptr())
        if fo is not None:
            ptr.update(fdw=fo.dw.ptr, fdb=fo.db.ptr, fws=fo.ws.data_ptr())
        args, keep = pair_structs(c, ptr)
        if fo is None:
            args['fold'] = 0
        _call('sdmi_bwd_pair', **args)
        torch.cuda.synchronize()
        if p.splits > 1:        # the pair leaves this layer's partials to a later fold
            assert out.untouched(), f'{c.id}: the pair launch wrote dW / dbias of a split problem'
            fold_group([out])
        return out, dx
    out, dx = go(fout)
    out.check_around(c.id)
    check_numbers(c.id, c.route, p, out, exact)
    if fout is not None:
        fout.check_around(c.id + '[fold]')
        check_numbers(c.id + '[fold]', c.route + ' fold', c.probs[1], fout, exact)
    # ---- dX
    Z, Az = R.dgrad_reference(dy, w, p, with_abs=not exact)
    z = Z + (bias_d.double()[None] if c.dbias_d else 0.0) + (res.double() if c.res else 0.0)
    flat = dx.flat.cpu()
    got = dx.mat(flat)[:, :p.Cin].clone()
    rest = flat.clone()
    dx.mat(rest)[:, :p.Cin] = POISON_OUT
    assert _same_bits(rest, torch.full_like(rest, POISON_OUT)), f'{c.id}: dX written outside [:M, :Cin]'
    if exact:
        assert float(z.abs().max()) < 256.0
        if not _same_bits(got, z.to(BF16)):
            bad = (got.double() != z).nonzero()
            i, j = (int(v) for v in bad[0])
            raise AssertionError(f'{c.id} ({c.route}): {len(bad)} elements of dX differ, first at row {i} column {j}: '
                                 f'got {float(got[i, j])}, exact {float(z[i, j])}')
    else:
        assert bool(torch.isfinite(got).all()), c.id
        err = (got.double() - z).abs()
        bound = (d['K'] + 3) * U * Az + 4 * U * z.abs()
        bound = bound + BF * (z.abs() + bound)
        share = float((err / bound.clamp_min(1e-300)).max())
        NEED[f'{c.route} dX'] = max(NEED.get(f'{c.route} dX', 0.0), share)
        print(f'{c.id}: {c.route}, dX: largest err/bound {share:.3f}')
        assert bool((err <= bound).all()), f'{c.id} ({c.route}) dX: {_worst(err, bound)}'
    # repeatability (without the fold: its partials are the same, its destination would accumulate twice)
    out2, dx2 = go(None)
    assert out2.same_as(out) and _same_bits(dx2.flat, dx.flat), f'{c.id}: a second launch gave other bits'
    assert ins.unchanged(), f'{c.id}: the launch changed its inputs'


RUN = {'single': run_single, 'group': run_group, 'fold': run_fold, 'pair': run_pair}


# ---- the tests -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', CASES, ids=lambda c: c.id)
def test_exact(c):
    """Exact arithmetic (module docstring): dW, dbias (and dX) equal the integer reference in every bit.  No tolerance."""
    RUN[c.kind](c, True)


@pytest.mark.parametrize('c', CASES, ids=lambda c: c.id)
def test_pinned(c):
    """Gaussian operands: the derived per-element bound (module docstring); bit-exact: the route, everything around the
    outputs, the workspace, deferred fold = immediate fold, repeatability, the inputs."""
    RUN[c.kind](c, False)


TAIL = [c for c in CASES if c.id in ('lin130x40x24+2blocks', 'lin70x136x64+acc', 'lin1000x136x264-s3-nobias+18blocks',
                                     '3x3@8-b3-c16-n24', '3x3@6x10-b9-c32-n136-s2', '1x3-c8-n72')]
assert len(TAIL) == 6


@pytest.mark.parametrize('c', TAIL, ids=lambda c: c.id)
def test_tail_rows_are_never_read(c):
    """Beyond the issue's list, for the scalar-only loaders (MODE 1 / 2), whose last 64-row step of a split runs past the
    split's end and is masked per loader by an out-of-range buffer offset.  With finite poison a loader that lost its
    mask goes unnoticed: the other operand's masked rows are zeros and 0 * 8192 = 0.  Here the pitch gaps and 64 guard rows
    around both operands (so that even an unmasked step stays inside the buffers) hold +inf: 0 * inf = NaN.  Exact
    arithmetic, every bit."""
    p = c.probs[0]
    assert wgrad_route(p) == c.route and c.route[-5:] in ('mode1', 'mode2')
    (x, dy, i_dw, i_db), _ = reference(p, True)
    ins = _Inputs(p, x, dy, extra=64, fill=float('inf'))
    out = _Out(p, i_dw, i_db)
    _launch_wgrad(p, ins, out)
    check_numbers(c.id, c.route, p, out, True)
