"""sdmi_igemm's forward kernels, called through the C ABI with every field spelled out and pinned, element by element,
to a float64 CPU reference computed from the tensors the kernel read (operands and residual rounded to their storage
dtype first; bias, row vector and alpha as the fp32 values the ABI carries).  Every case states the kernel instantiation
it is there for and asserts it after the launch with sdmi_igemm_last_route: when dispatch changes, the case fails with
"expected halo logw5, got sym st2 mode2" instead of passing on another kernel.

Reference (_core / _reference, from the definitions in sdmi.h, explicit loops over the filter taps, rows in chunks):
    z = alpha sum_k a w + bias + rowvec + residual        the exact pre-activation
    A = |alpha| sum_k |a w|                               what the accumulation error is relative to (not |z|: where
                                                          the products cancel |z| says nothing about their rounding)

Every tolerance is one of three kinds (the discipline of test_gpu_bwd_helpers.py and test_gpu_attention_pins.py):

  derived     per element, no norms, no share of elements (U = 2^-24, BF = 2^-8):
                fp32 result        (K + s + 3) U A + 4 U |z|     s = K slices summed by the split-K second stage (0
                                   without a split), 3 = the alpha multiply and the two adds of the epilogue; one form for
                                   the bf16 and the fp32 MFMA paths
                bf16 storage       BF (|exact| + the bound before it) on top: one rounding
                relu               the bound of z
  expf        silu / gelu epilogues: the bound of z times the activation's Lipschitz constant (sup |silu'|, sup |gelu'|,
              computed below in float64: 1.0998 and 1.1290) + r |exact| + a, one (r, a) row of EXPF per evaluated form:
              act_apply (fp32 output and the split-K second stage) and act_apply<true> (bf16-output epilogues).
  bit-exact   every element of the output buffer the launch does not own is unchanged (pitch gap, one guard row before
              and one after, foreign pixels of a sub-sampled placement); the split-K workspace past splits M N floats;
              all inputs; a second launch gives the same bits; defer_epilogue + sdmi_splitk_finish gives the bits of the
              direct launch (and writes nothing to `out` before the finish); and the exact-arithmetic cases
              (test_exact): activations in {-1, 0, 1}, weight rows of at most 96 entries of +-1 at random places (every
              tap and K tile carries some), integer bias / row vector / residual, alpha = 1 -- every product and partial
              sum is an integer below 2^8, so the result equals the integer reference in every bit, bf16 as fp32.

Poison: input pitches are wider than the row where the ABI allows it (lda > K for linear problems, lda2 / lda3, ldr > N,
ldrv > N), and the gaps and a guard row behind every operand hold 8192.0 (finite, exact in bf16, far above any bound
when one stray product reaches a sum, and 0 * 8192 = 0 where a kernel masks through a zero operand).  Output buffers
hold -3.0.

Routes (CU = the device's compute-unit count; the M of a case whose gate depends on CU is derived from it) and the cases
that reach them -- the id of a case lists the edges it carries:
  cfg 64x64 mode0 kt64 / kt128    ups-*, zins2-*, 7x7-*, s2p1111-*, 5x5same-*            (generic gather, fp32 and bf16)
  cfg 64x64 mode1 / mode2         lin70x50x24-*, 3x3-c32-fp32-*, s2p0101-*, 1x1s2-*, bmm-*, sub2x2-*
  cfg 64x64 split                 lin8x200x1024-fp32-split8
  cfg 128x64                      c32-n40-fp32 (mode2), c32-n64-bf16 (mode0), c64-n40-bf16 (mode2)
  cfg 128x128                     c64-n136-b48 (mode2 bf16), c32-n136-b48-fp32, c8-n136-b48 (kt64 mode0), lin12288x136x320
  cfg xs                          1x1+a2+a3-fp32-64, 3x3+a2+a3-fp32-64, 1x1+a2+a3-fp32-128, 3x3+a2-fp32-128, 3x3+a2-bf16-128
  dma 64x64 mode1 / mode2         lin200x130x264, 3x3-c64@8
  dma 64x64 split 2 .. 16         c512-n512@4 (16), c960-n64@4 (16, last slice empty), lin4x2944x512 (2), c128-n64@4 (4),
                                  c256-n64@4 (8), caller16 (more tiles than the 2 CU / 16 workgroups of a slice)
  dma 64x64 xs, parity4           restail@8-*, parity4-8to16
  dma 128x128 lw8 (xs)            c256-n136-b48, c256+a2-n136-b48
  sym st2 mode1 / mode2 (xs)      lin-sym-k320, lin-sym-k328, c64-n256@24, c64+a2-n256@24; lin-sym-walk and
                                  c64-n256@24-walk (exact only: more than 4 CU tiles, every workgroup walks several)
  halo logw 4 / 5 / 6             halo16-*, halo32-*, halo64, halo32x128, halo16-walk (exact only: more tiles than CUs)
  c64                             c64-n64-4x64, c64-n40-4x64, c64-n64-8x128
  splitk_epilogue_kernel / sdmi_splitk_finish: every split case above.
The conditions of the row-major epilogue's gate (epi_rows.h: epilogue_rows_ok) each have halo32-* cases on both sides:
halo32-base is on the fast side of all of them, every halo32-flip-* moves exactly one to the slow side (ldc % 8, `out`
off 16 bytes, ldr % 4, residual off 8 bytes, bias off 16 bytes, rowvec off 16 bytes, ldrv % 4, bias_m, a ragged N
block).  Not flippable through a halo launch: split_k, out_dtype, osy, a ragged M block (dispatch admits none of
them), rowvec with Ho Wo < 64 (halo needs >= 256), gn_part (out of scope) and M max(ldc, ldr) >= 2^30 (a 2 GB output).
wave_epilogue_fast's own gate (igemm_body.h: epilogue_fast_ok) is crossed by the other routes' cases: fp32 output,
split-K, bias_m (bmm-*), ragged M / N blocks, rowvec with Ho Wo = 16 (fast), 81 / 100 / 576 (not a power of two: slow).

Instantiations of dispatch that no argument set reaches with the environment unset, hence NOT covered here:
  igemm_dma_kernel<T, 256, 128, 3, 1|2> and <T, 128, 128, 4, 1|2, 4> (four loader waves): SDMI_IGEMM_DMA = 1 / 2 only;
  igemm_sym_kernel<1|2, 3|4, *>: SDMI_IGEMM_SYM = 3 / 4 only;
  igemm_kernel_tall: launch_cfg is never instantiated with BM > 128;
  conv3x3_c64_kernel<true> (the ROWS form) is not instantiated.
Out of scope: the EPI != 0 epilogues, gn_part, fp8 operands.

Measured on an MI355X (CU = 256), every case: the largest share of its bound any element used is 0.995 on bf16 outputs
(the storage rounding landing on half an ulp; 0.32 - 0.95 on the split-K cases, the deeper the K the lower: their
(K + s + 3) U A term grows past half a bf16 ulp) and 0.13 on fp32 outputs (lin70x50x24-fp32, K = 24; at most 0.04
elsewhere); neither EXPF row needed its r."""
import math
import os
import types
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_bwd_helpers import (BF, DEV, U, _call, _dt, _end_the_session_on_a_gpu_fault,  # noqa: F401
                                        _gen, _L, _poison, _q, _same_bits, _worst)

pytestmark = pytest.mark.gpu

_SWITCHES = [k for k in ('SDMI_IGEMM_DMA', 'SDMI_IGEMM_SYM', 'SDMI_IGEMM_HALO') if k in os.environ]
if _SWITCHES:
    pytest.skip(f'{", ".join(_SWITCHES)} set: the routes asserted here are the default ones', allow_module_level=True)

F32, BF16 = torch.float32, torch.bfloat16
_ID = {F32: 'fp32', BF16: 'bf16'}
CU = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
POISON_IN, POISON_OUT = 8192.0, -3.0

# (r, a) of the expf bound per evaluated form.  "needs r" = the largest (err - every other term) / |exact| any case of
# this file measured on an MI355X against the float64 reference.
EXPF = {
    'act_apply': (4e-7, 2e-7),           # fp32 output, split-K second stage: needs r 0
    'act_apply<true>': (4e-7, 2e-7),     # bf16-output epilogues (v_rcp SiLU, branch-free erf): needs r 0
}
assert all(r <= 4e-6 and a <= 1e-6 for r, a in EXPF.values())
# for a measuring run to print: '<form> r' = the largest r needed, '<route> err/bound' = the largest share of its bound
# any element of that route used
NEED = {}


def _sup_abs_derivative(kind):
    """sup |act'| in float64 on a grid of step 1e-5 over [-10, 10] (|act''| <= 1.2: the grid misses < 1e-9, added)."""
    x = torch.linspace(-10, 10, 2000001, dtype=torch.float64)
    if kind == 'silu':
        s = torch.sigmoid(x)
        d = s * (1 + x * (1 - s))
    else:
        d = 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return float(d.abs().max()) + 1e-9


LIP = {'silu': _sup_abs_derivative('silu'), 'gelu': _sup_abs_derivative('gelu')}
assert 1.09 < LIP['silu'] < 1.11 and 1.12 < LIP['gelu'] < 1.14


# ---- cases -----------------------------------------------------------------------------------------------
P1 = (1, 1, 1, 1)
_DEFAULTS = dict(
    dt=BF16, odt=None, lin=False, B=1, H=1, W=1, Cin=0, N=0, k=1, stride=1, pad=(0, 0, 0, 0), ups=0, zins=0,
    sub=None, parity4=False, x2=0, x3=0, Z=1, shared_w=False, bias_m=False,
    bias=False, bias_off=0, rowvec=False, rv_off=0, ldrv_pad=4, res=False, res_off=0, ldr_pad=8, ldc_pad=8, out_off=0,
    act=None, alpha=1.0, ws=False, split_k=0, exact_only=False)
CASES = []


def _add(cid, route, M=None, K=None, **kw):
    """One case.  route: what sdmi_igemm_last_route must decode to (`splitP` = the launcher's own plan, recomputed
    here).  M, K: a linear problem (H = W = 1, lda > K).  pads are (top, bottom, left, right); x2 / x3 = channels of the
    extra sources; *_pad = elements between the row and its pitch; *_off = elements the pointer is moved off its
    aligned position; ws: pass a workspace (split_k = 0: the launcher decides); split_k: the caller's override."""
    bad = set(kw) - set(_DEFAULTS)
    assert not bad, bad
    c = types.SimpleNamespace(**{**_DEFAULTS, **kw})
    c.id, c.route = cid, route
    if M is not None:
        c.lin, c.B, c.Cin = True, M, K
    c.odt = c.odt or c.dt
    c.vec = 8 if c.dt == BF16 else 4
    c.KH = c.KW = c.k
    Hv = 2 * c.H if c.ups else ((c.H - 1) * c.zins + 1 if c.zins > 1 else c.H)
    Wv = 2 * c.W if c.ups else ((c.W - 1) * c.zins + 1 if c.zins > 1 else c.W)
    c.Ho = (Hv + c.pad[0] + c.pad[1] - c.KH) // c.stride + 1
    c.Wo = (Wv + c.pad[2] + c.pad[3] - c.KW) // c.stride + 1
    if c.parity4:
        c.Ho, c.Wo, c.sub = c.H, c.W, (2, 2, 0, 0)
    c.M = c.B * c.Ho * c.Wo
    c.K1 = c.KH * c.KW * c.Cin
    c.K = c.K1 + c.x2 + c.x3
    c.Zo = 4 if c.parity4 else c.Z                     # output blocks of M rows
    c.ZW = 4 if c.parity4 else (1 if c.shared_w else c.Z)
    c.lda = c.K1 + 2 * c.vec if c.lin else c.Cin
    c.ldc = c.N + c.ldc_pad
    c.ldr = c.ldc if c.sub else c.N + c.ldr_pad
    c.ldrv = c.N + c.ldrv_pad
    c.oH, c.oW = (c.sub[0] * c.Ho, c.sub[1] * c.Wo) if c.sub else (0, 0)
    c.rows = c.B * c.oH * c.oW if c.sub else c.Zo * c.M        # rows of the output tensor
    # everything the operand values and the sums over K depend on (cases that differ in epilogue layout share a core)
    c.gkey = (c.dt, c.lin, c.B, c.H, c.W, c.Cin, c.N, c.k, c.stride, c.pad, c.ups, c.zins, c.parity4, c.x2, c.x3, c.Z,
              c.shared_w)
    CASES.append(c)


def _cdiv(a, b):
    return -(-a // b)


def _build_cases():
    # ---- igemm_kernel, 64 x 64, generic gather (MODE 0), K tiles of 64 and 128 bytes
    _add('ups-c8-bf16+Mrag+N3+ldc%8', 'cfg 64x64 kt64 mode0', B=2, H=6, W=6, Cin=8, N=3, k=3, pad=P1, ups=1, bias=True,
         ldc_pad=5)
    _add('ups-c8-fp32+rowvec100+silu', 'cfg 64x64 kt64 mode0', dt=F32, B=3, H=5, W=5, Cin=8, N=20, k=3, pad=P1, ups=1,
         bias=True, rowvec=True, act='silu')
    _add('zins2-c24-bf16+res+alpha', 'cfg 64x64 kt64 mode0', B=2, H=5, W=5, Cin=24, N=40, k=3, pad=(1, 2, 1, 2), zins=2,
         res=True, alpha=0.37)
    _add('zins2-c24-fp32+N12', 'cfg 64x64 kt128 mode0', dt=F32, B=2, H=5, W=5, Cin=24, N=12, k=3, pad=(1, 2, 1, 2),
         zins=2, bias=True)
    _add('zins2-c96-bf16+fp32out', 'cfg 64x64 kt128 mode0', odt=F32, B=2, H=5, W=5, Cin=96, N=72, k=3,
         pad=(1, 2, 1, 2), zins=2, bias=True, res=True, ldr_pad=2)
    _add('7x7-s2-c8-fp32', 'cfg 64x64 kt128 mode0', dt=F32, B=2, H=15, W=15, Cin=8, N=24, k=7, stride=2,
         pad=(3, 3, 3, 3), bias=True, act='relu')
    _add('7x7-c8-bf16+gelu', 'cfg 64x64 kt128 mode0', B=2, H=9, W=9, Cin=8, N=24, k=7, pad=(3, 3, 3, 3), bias=True,
         act='gelu')
    _add('s2p1111-c32-bf16+relu', 'cfg 64x64 kt128 mode0', B=2, H=16, W=16, Cin=32, N=48, k=3, stride=2, pad=P1,
         bias=True, act='relu')
    _add('5x5same-c8-bf16+rowvec81', 'cfg 64x64 kt64 mode0', B=2, H=9, W=9, Cin=8, N=16, k=5, pad=(2, 2, 2, 2),
         bias=True, rowvec=True)
    # ---- igemm_kernel, 64 x 64, MODE 1 / 2
    _add('s2p0101-c32-fp32', 'cfg 64x64 kt128 mode2', dt=F32, B=2, H=16, W=16, Cin=32, N=40, k=3, stride=2,
         pad=(0, 1, 0, 1), bias=True)
    _add('1x1s2-c64-bf16+rowvec16', 'cfg 64x64 kt64 mode2', B=2, H=8, W=8, Cin=64, N=32, k=1, stride=2, bias=True,
         rowvec=True, ldc_pad=0)
    _add('lin70x50x24-bf16+bias_off+ldr%4', 'cfg 64x64 kt64 mode1', M=70, K=24, N=50, bias=True, bias_off=1, res=True,
         ldr_pad=3)
    _add('lin70x50x24-fp32+alpha', 'cfg 64x64 kt64 mode1', dt=F32, M=70, K=24, N=50, bias=True, res=True, alpha=0.37,
         ldc_pad=3)
    _add('3x3-c32-fp32+rowvec64+gelu', 'cfg 64x64 kt128 mode2', dt=F32, B=2, H=8, W=8, Cin=32, N=40, k=3, pad=P1,
         bias=True, rowvec=True, act='gelu')
    _add('sub2x2-c32-fp32+res', 'cfg 64x64 kt128 mode2', dt=F32, B=2, H=6, W=6, Cin=32, N=24, k=3, pad=P1,
         sub=(2, 2, 1, 0), bias=True, res=True)
    _add('bmm-z6-160x96x64-bf16+bias_m+sharedw', 'cfg 64x64 kt64 mode1', M=160, K=64, N=96, Z=6, shared_w=True,
         bias=True, bias_m=True, res=True, alpha=0.37)
    _add('bmm-z6-160x96x64-fp32', 'cfg 64x64 kt64 mode1', dt=F32, M=160, K=64, N=96, Z=6, bias=True)
    _add('lin8x200x1024-fp32-split8', 'cfg 64x64 kt128 mode1 splitP', dt=F32, M=8, K=1024, N=200, bias=True, res=True,
         ws=True, ldc_pad=0)
    # ---- igemm_kernel, 128 x 64: 32 < N <= 64 and >= 192 row tiles (M ragged in the last one)
    big = dict(B=7, H=60, W=59, k=3, pad=P1)
    assert _cdiv(7 * 60 * 59, 128) >= 192 and (7 * 60 * 59) % 128
    _add('c32-n40-fp32+Mrag+relu', 'cfg 128x64 kt128 mode2', dt=F32, Cin=32, N=40, bias=True, act='relu', **big)
    _add('c32-n64-bf16+Mrag+silu', 'cfg 128x64 kt128 mode0', Cin=32, N=64, bias=True, res=True, act='silu', **big)
    _add('c64-n40-bf16+Mrag', 'cfg 128x64 kt128 mode2', Cin=64, N=40, bias=True, rowvec=True, **big)
    # ---- igemm_kernel, 128 x 128: >= 192 tiles, below every faster kernel's gate
    l16 = dict(B=48, H=16, W=16, k=3, pad=P1)
    _add('c64-n136-b48+rowvec256+silu', 'cfg 128x128 kt128 mode2', Cin=64, N=136, bias=True, rowvec=True, res=True,
         act='silu', **l16)
    _add('c32-n136-b48-fp32', 'cfg 128x128 kt128 mode2', dt=F32, Cin=32, N=136, bias=True, res=True, **l16)
    _add('c8-n136-b48-bf16', 'cfg 128x128 kt64 mode0', Cin=8, N=136, bias=True, **l16)
    _add('lin12288x136x320-bf16', 'cfg 128x128 kt128 mode1', M=12288, K=320, N=136, bias=True, res=True)
    # ---- igemm_kernel with extra sources
    _add('1x1+a2+a3-fp32-64', 'cfg 64x64 kt128 mode1 xs', dt=F32, M=100, K=64, N=72, x2=64, x3=32, bias=True)
    _add('3x3+a2+a3-fp32-64', 'cfg 64x64 kt128 mode2 xs', dt=F32, B=2, H=8, W=8, Cin=32, N=40, k=3, pad=P1, x2=32, x3=64,
         bias=True, res=True)
    _add('1x1+a2+a3-fp32-128', 'cfg 128x128 kt128 mode1 xs', dt=F32, B=48, H=16, W=16, Cin=64, N=136, x2=64, x3=32,
         bias=True)
    _add('3x3+a2-fp32-128', 'cfg 128x128 kt128 mode2 xs', dt=F32, Cin=32, N=136, x2=32, bias=True, rowvec=True, **l16)
    _add('3x3+a2-bf16-128', 'cfg 128x128 kt128 mode2 xs', Cin=64, N=136, x2=64, bias=True, res=True, **l16)
    # ---- igemm_dma_kernel, 64 x 64
    _add('lin200x130x264-bf16+Ktail8+fp32out', 'dma 64x64 st4 lw4 mode1', odt=F32, M=200, K=264, N=130, bias=True,
         res=True, ldr_pad=2)
    _add('lin200x130x264-bf16+Ktail8', 'dma 64x64 st4 lw4 mode1', M=200, K=264, N=130, bias=True, res=True, act='gelu')
    _add('3x3-c64@8-bf16+rowvec64+silu', 'dma 64x64 st4 lw4 mode2', B=3, H=8, W=8, Cin=64, N=136, k=3, pad=P1,
         bias=True, rowvec=True, res=True, act='silu')
    sk = dict(k=3, pad=P1, ws=True, ldc_pad=0)
    _add('c512-n512@4-b4-split16', 'dma 64x64 st4 lw4 mode2 splitP', B=4, H=4, W=4, Cin=512, N=512, bias=True,
         rowvec=True, res=True, **sk)
    _add('c960-n64@4-split16-emptyslice', 'dma 64x64 st4 lw4 mode2 splitP', B=1, H=4, W=4, Cin=960, N=64, bias=True,
         **sk)
    _add('lin4x2944x512-split2', 'dma 64x64 st4 lw4 mode1 splitP', M=4, K=512, N=2944, bias=True, res=True, ws=True,
         ldc_pad=0, alpha=0.37)
    _add('c128-n64@4-split4', 'dma 64x64 st4 lw4 mode2 splitP', B=4, H=4, W=4, Cin=128, N=64, bias=True, res=True,
         ldr_pad=3, **sk)
    _add('c128-n64@4-split4+silu', 'dma 64x64 st4 lw4 mode2 splitP', B=4, H=4, W=4, Cin=128, N=64, k=3, pad=P1, ws=True,
         bias=True, res=True, act='silu')
    _add('c256-n64@4-split8+fp32out+gelu', 'dma 64x64 st4 lw4 mode2 splitP', odt=F32, B=4, H=4, W=4, Cin=256, N=64, k=3,
         pad=P1, ws=True, bias=True, act='gelu')
    _add('c256-n64@4-split8', 'dma 64x64 st4 lw4 mode2 splitP', B=4, H=4, W=4, Cin=256, N=64, bias=True, **sk)
    # caller's split_k = 16 with more 64 x 64 tiles (CU / 8 + 8) than the 2 CU / 16 workgroups a slice gets
    _add('caller16-lin-n451-k1032', 'dma 64x64 st4 lw4 mode1 split16', M=64 * (CU // 64 + 1), K=1032, N=451, bias=True,
         res=True, ws=True, split_k=16, ldc_pad=0)
    # ---- igemm_dma_kernel, 64 x 64: extra sources (kern.res_tail's form at 8 x 8), parity4
    _add('restail@8-c64+a2', 'dma 64x64 st4 lw4 mode2 xs', B=3, H=8, W=8, Cin=64, N=72, k=3, pad=P1, x2=64, bias=True,
         rowvec=True)
    _add('restail@8-c64+a2+a3-split2', 'dma 64x64 st4 lw4 mode2 xs splitP', B=3, H=8, W=8, Cin=64, N=72, x2=64, x3=128,
         bias=True, res=True, **sk)
    _add('parity4-8to16-c64', 'dma 64x64 st4 lw4 mode2', B=2, H=8, W=8, Cin=64, N=72, k=2, parity4=True, bias=True)
    # ---- igemm_dma_kernel, 128 x 128, eight loader waves: K >= 4096 bytes, >= 192 tiles, < 192 tiles of 256 x 128
    _add('c256-n136-b48+silu', 'dma 128x128 st4 lw8 mode2', Cin=256, N=136, bias=True, rowvec=True, res=True, act='silu',
         **l16)
    _add('c256+a2-n136-b48', 'dma 128x128 st4 lw8 mode2 xs', Cin=256, N=136, x2=64, bias=True, res=True, **l16)
    # ---- igemm_sym_kernel, two stages: >= 2 CU tiles of 128 x 128, K > 512 bytes
    ms = 128 * (CU // 2) - 100
    _add('lin-sym-k320+Mrag', 'sym st2 mode1', M=ms, K=320, N=512, bias=True, res=True)
    _add('lin-sym-k328+Ktail8+fp32out+alpha', 'sym st2 mode1', odt=F32, M=ms, K=328, N=512, bias=True, alpha=0.37)
    bs = _cdiv(CU * 128, 24 * 24)
    _add('c64-n256@24+silu', 'sym st2 mode2', B=bs, H=24, W=24, Cin=64, N=256, k=3, pad=P1, bias=True, res=True,
         act='silu')
    _add('c64+a2-n256@24+rowvec576', 'sym st2 mode2 xs', B=bs, H=24, W=24, Cin=64, N=256, k=3, pad=P1, x2=64, bias=True,
         rowvec=True)
    # more than 4 CU tiles: every one of the 2 CU workgroups walks at least two (exact arithmetic only: reference work)
    _add('lin-sym-walk', 'sym st2 mode1', M=128 * (CU + 2), K=320, N=512, bias=True, res=True, exact_only=True)
    _add('c64-n256@24-walk', 'sym st2 mode2', B=_cdiv((2 * CU + 4) * 128, 24 * 24), H=24, W=24, Cin=64, N=256, k=3,
         pad=P1, bias=True, rowvec=True, res=True, exact_only=True)
    # ---- igemm_halo_kernel: 3x3 "same", >= 192 tiles of 256 x 128 (M = 96 * 256, N = 192: one and a half column tiles)
    ep = dict(k=3, pad=P1, bias=True, rowvec=True, res=True, ldc_pad=8, ldr_pad=8, ldrv_pad=4)
    _add('halo16-c64+silu', 'halo logw4', B=96, H=16, W=16, Cin=64, N=192, act='silu', **ep)
    _add('halo16-c192', 'halo logw4', B=96, H=16, W=16, Cin=192, N=192, **ep)
    _add('halo32-base', 'halo logw5', B=24, H=32, W=32, Cin=64, N=192, **ep)
    h32 = dict(B=24, H=32, W=32, Cin=64, N=192)
    _add('halo32-flip-ldc%8', 'halo logw5', **h32, **{**ep, 'ldc_pad': 4})
    _add('halo32-flip-out_off', 'halo logw5', out_off=4, **h32, **ep)
    _add('halo32-flip-ldr%4', 'halo logw5', **h32, **{**ep, 'ldr_pad': 6})
    _add('halo32-flip-res_off', 'halo logw5', res_off=1, **h32, **ep)
    _add('halo32-flip-bias_off', 'halo logw5', bias_off=1, **h32, **ep)
    _add('halo32-flip-rv_off', 'halo logw5', rv_off=1, **h32, **ep)
    _add('halo32-flip-ldrv%4', 'halo logw5', **h32, **{**ep, 'ldrv_pad': 3})
    _add('halo32-flip-bias_m', 'halo logw5', bias_m=True, **h32, **ep)
    _add('halo32-flip-Nrag136+gelu', 'halo logw5', B=24, H=32, W=32, Cin=64, N=136, act='gelu', **ep)
    _add('halo64', 'halo logw6', B=6, H=64, W=64, Cin=64, N=192, **ep)
    _add('halo32x128+relu', 'halo logw6', B=6, H=32, W=128, Cin=64, N=192, act='relu', **ep)
    _add('halo16-walk', 'halo logw4', B=CU // 2 + 8, H=16, W=16, Cin=64, N=192, exact_only=True, **ep)
    # ---- conv3x3_c64_kernel: >= 2 CU tiles of 4 x 64 pixels
    _add('c64-n64-4x64', 'c64', B=2 * CU, H=4, W=64, Cin=64, N=64, k=3, pad=P1, bias=True, res=True)
    _add('c64-n40-4x64+rowvec256+silu', 'c64', B=2 * CU, H=4, W=64, Cin=64, N=40, k=3, pad=P1, bias=True, rowvec=True,
         act='silu')
    _add('c64-n64-8x128', 'c64', B=CU // 2, H=8, W=128, Cin=64, N=64, k=3, pad=P1, bias=True, rowvec=True, res=True,
         ldc_pad=0)


_build_cases()
assert len({c.id for c in CASES}) == len(CASES)
DERIVED = [c for c in CASES if not c.exact_only]
# exact arithmetic: one case per route and operand dtype (the first of each) + the cases only run this way
EXACT = list({(c.route, c.dt): c for c in reversed(DERIVED)}.values())[::-1] + [c for c in CASES if c.exact_only]


# ---- plumbing ------------------------------------------------------------------------------------------
def _route_name(r):
    fam, bm, bn, kt = r & 15, (r >> 4 & 7) * 64, (r >> 7 & 7) * 64, r >> 10 & 7
    mode, xs, epi, split, logw, lw8 = r >> 13 & 3, r >> 15 & 1, r >> 16 & 7, r >> 19 & 31, r >> 24 & 7, r >> 27 & 1
    E = _L().ENUMS
    s = {E['SDMI_ROUTE_CFG']: f'cfg {bm}x{bn} kt{kt * 64} mode{mode}',
         E['SDMI_ROUTE_DMA']: f'dma {bm}x{bn} st{kt} lw{8 if lw8 else 4} mode{mode}',
         E['SDMI_ROUTE_SYM']: f'sym st{kt} mode{mode}', E['SDMI_ROUTE_HALO']: f'halo logw{logw}',
         E['SDMI_ROUTE_C64']: 'c64'}.get(fam, f'unknown family {fam}')
    return s + (' xs' if xs else '') + (f' epi{epi}' if epi else '') + (f' split{split}' if split > 1 else ''), split


def _plan(c):
    """dispatch's own K split for a 64 x 64 launch with a workspace (igemm.hip: sk_target = 384 workgroups, at least four
    K tiles per slice, at most 16 slices)."""
    kbytes = c.K * (2 if c.dt == BF16 else 4)
    t64, nk, s = _cdiv(c.M, 64) * _cdiv(c.N, 64), _cdiv(kbytes, 128 if kbytes >= 512 else 64), 1
    while t64 * s < 384 and s * 2 <= nk // 4 and s < 16:
        s *= 2
    return s


def _alpha(c):
    return float(torch.tensor(c.alpha, dtype=torch.float32))


class _Buf:
    """A flat device buffer full of `fill` with a [rows, ld] matrix `off` elements in; .ptr addresses the matrix."""

    def __init__(self, rows, ld, dtype, fill, off=0, tail=0):
        self.rows, self.ld, self.off = rows, ld, off
        self.flat = _poison((off + rows * ld + tail,), dtype, fill)
        self.ptr = self.flat.data_ptr() + off * self.flat.element_size()

    def mat(self, flat=None):
        return (self.flat if flat is None else flat)[self.off:self.off + self.rows * self.ld].view(self.rows, self.ld)

    def put(self, data, rowidx=None):
        d = data.to(self.flat.dtype).to(DEV)
        if rowidx is None:
            self.mat()[:d.shape[0], :d.shape[1]] = d
        else:
            self.mat()[rowidx.to(DEV), :d.shape[1]] = d
        return self


def _in(rows, ld, dtype, data, off=0, rowidx=None):
    """Input operand: `data` in the first columns of [rows, ld], 8192 in the pitch gap, in one guard row behind it and in
    the `off` elements in front."""
    return _Buf(rows + 1, ld, dtype, POISON_IN, off=off, tail=8).put(data, rowidx)


def _out(c):
    """Output: [1 + rows + 1, ldc] of -3 (a guard row before and after), `out` at a 16-byte aligned position + out_off."""
    front = _cdiv(c.ldc, 8) * 8 + c.out_off
    return _Buf(c.rows, c.ldc, c.odt, POISON_OUT, off=front, tail=c.ldc + 8)


def _rowidx(c):
    """Row of the output tensor that holds output row (z, m), [Zo * M]."""
    if not c.sub:
        return torch.arange(c.Zo * c.M)
    m = torch.arange(c.M)
    b, rem = m // (c.Ho * c.Wo), m % (c.Ho * c.Wo)
    oy, ox = rem // c.Wo, rem % c.Wo
    out = []
    for z in range(c.Zo):
        ooy, oox = (z >> 1, z & 1) if c.parity4 else c.sub[2:]
        out.append((b * c.oH + oy * c.sub[0] + ooy) * c.oW + ox * c.sub[1] + oox)
    return torch.cat(out)


# ---- operands and the float64 reference ------------------------------------------------------------------
def _seed(c, salt):
    return zlib.crc32(repr((c.gkey, salt)).encode())


def _operands(c, exact):
    """CPU fp32 tensors on the storage grid: x [B, H, W, Cin] ([Z, M, K1] batched), w [ZW, N, K], x2 / x3 [M, .]."""
    g = _gen(_seed(c, exact))
    xs = (c.Z, c.B, c.H, c.W, c.Cin)
    if exact:
        rnd = lambda *s: torch.randint(-1, 2, s, generator=g).float()
        nnz = min(96, c.K)
        idx = torch.rand(c.ZW * c.N, c.K, generator=g).topk(nnz, dim=1).indices
        sign = torch.randint(0, 2, idx.shape, generator=g).float() * 2 - 1
        w = torch.zeros(c.ZW * c.N, c.K).scatter_(1, idx, sign).view(c.ZW, c.N, c.K)
    else:
        rnd = lambda *s: _q(torch.randn(*s, generator=g), c.dt)
        w = _q(torch.randn(c.ZW, c.N, c.K, generator=g) / math.sqrt(c.K), c.dt)
    x = rnd(*xs)
    x2 = rnd(c.M, c.x2) if c.x2 else None
    x3 = rnd(c.M, c.x3) if c.x3 else None
    return x, w, x2, x3


def _epilogue_terms(c, exact):
    """bias [N], bias_m [M], rowvec [B, N] (fp32), residual [Zo * M, N] (on the output grid); all generated whether or not
    the case uses them, so cases that share a core share these too."""
    g = _gen(_seed(c, ('epi', exact)))
    if exact:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        return ri(-8, 8, c.N), ri(-8, 8, c.M), ri(-8, 8, c.B, c.N), ri(-16, 16, c.Zo * c.M, c.N)
    rn = lambda *s: torch.randn(*s, generator=g)
    return rn(c.N) * 0.5, rn(c.M) * 0.5, rn(c.B, c.N) * 0.5, _q(rn(c.Zo * c.M, c.N), BF16)


def _src(n_out, stride, pad, k, size, ups, zins):
    """Source index of tap k for every output coordinate, and whether it exists (sdmi.h: zero outside the image; ups:
    nearest x2 view; zins: only every zins-th virtual pixel is real)."""
    i = torch.arange(n_out) * stride - pad + k
    if ups:
        ok, s = (i >= 0) & (i < 2 * size), i // 2
    elif zins > 1:
        ok, s = (i >= 0) & (i % zins == 0) & (i // zins < size), i // zins
    else:
        ok, s = (i >= 0) & (i < size), i
    return ok, s.clamp(0, size - 1)


_CORE = {}


def _core(c, exact):
    """(operands, S = sum_k a w, A0 = sum_k |a w|) as float64 [Zo * M, N]; A0 is None for exact arithmetic.  The two
    most recent are kept (cases that differ only in their epilogue layout follow one another)."""
    key = (c.gkey, exact)
    if key in _CORE:
        return _CORE[key]
    ops = _operands(c, exact)
    x, w, x2, x3 = ops
    S = torch.zeros(c.Zo * c.M, c.N, dtype=torch.float64)
    A0 = None if exact else torch.zeros_like(S)
    hw = c.Ho * c.Wo
    per = max(1, 8192 // hw)                                   # images per chunk of rows
    for z in range(c.Zo):
        wz = w[z % c.ZW].double()
        pad_t, pad_l = (1 - (z >> 1), 1 - (z & 1)) if c.parity4 else (c.pad[0], c.pad[2])
        xz = x[z % x.shape[0]].double()
        for b0 in range(0, c.B, per):
            b1 = min(c.B, b0 + per)
            r0, r1 = z * c.M + b0 * hw, z * c.M + b1 * hw
            for kh in range(c.KH):
                oky, sy = _src(c.Ho, c.stride, pad_t, kh, c.H, c.ups, c.zins)
                for kw in range(c.KW):
                    okx, sx = _src(c.Wo, c.stride, pad_l, kw, c.W, c.ups, c.zins)
                    a = xz[b0:b1][:, sy][:, :, sx] * (oky[:, None] & okx[None, :])[None, :, :, None]
                    a = a.reshape(-1, c.Cin)
                    wt = wz[:, (kh * c.KW + kw) * c.Cin:(kh * c.KW + kw + 1) * c.Cin]
                    S[r0:r1] += a @ wt.T
                    if A0 is not None:
                        A0[r0:r1] += a.abs() @ wt.abs().T
            k0 = c.K1
            for xe in (x2, x3):                                # extra sources: 1x1 taps at the output pixel
                if xe is not None:
                    a, wt = xe[b0 * hw:b1 * hw].double(), wz[:, k0:k0 + xe.shape[1]]
                    S[r0:r1] += a @ wt.T
                    if A0 is not None:
                        A0[r0:r1] += a.abs() @ wt.abs().T
                    k0 += xe.shape[1]
    while len(_CORE) >= 2:
        _CORE.pop(next(iter(_CORE)))
    _CORE[key] = (ops, S, A0)
    return _CORE[key]


def _reference(c, exact):
    """z and A of the module docstring, [Zo * M, N] float64, from the terms the case passes."""
    _, S, A0 = _core(c, exact)
    bias, bias_m, rv, res = _epilogue_terms(c, exact)
    al = _alpha(c)
    z = al * S
    if c.bias:
        z = z + (bias_m.double().repeat(c.Zo)[:, None] if c.bias_m else bias.double()[None, :])
    if c.rowvec:
        z = z + rv.double().repeat_interleave(c.Ho * c.Wo, 0).repeat(c.Zo, 1)
    if c.res:
        z = z + _q(res, c.odt).double()
    return z, (None if A0 is None else abs(al) * A0)


# ---- launch ----------------------------------------------------------------------------------------------
def _launch(c, exact):
    """Build the poisoned buffers, launch, and check everything bit-exact that does not need the reference: the route,
    the untouched parts of the output and the workspace, repeatability, deferred = direct, unchanged inputs.
    -> (out rows [Zo * M, N] in the output dtype on the CPU, K slices summed by a second stage (0: none), route name)."""
    (x, w, x2, x3), _, _ = _core(c, exact)
    bias, bias_m, rv, res = _epilogue_terms(c, exact)
    rowidx = _rowidx(c)
    a_b = _in(c.Z * c.M, c.lda, c.dt, x.reshape(c.Z * c.M, c.K1)) if c.lin else \
        _in(c.B * c.H * c.W + c.W, c.Cin, c.dt, x.reshape(-1, c.Cin))
    w_b = _in(c.ZW * c.N, c.K, c.dt, w.reshape(c.ZW * c.N, c.K))
    ins = [a_b, w_b]
    kw = dict(a=a_b.ptr, w=w_b.ptr, dtype=_dt(c.dt), out_dtype=_dt(c.odt), M=c.M, N=c.N, K=c.K, lda=c.lda, ldw=c.K,
              ldc=c.ldc, B=c.B, H=c.H, W=c.W, Cin=c.Cin, Ho=c.Ho, Wo=c.Wo, KH=c.KH, KW=c.KW, stride=c.stride,
              pad_t=c.pad[0], pad_l=c.pad[2], ups=c.ups, zins=c.zins, act=_L().ACT[c.act], alpha=_alpha(c),
              bias_m=int(c.bias_m), batch=4 if c.parity4 else c.Z, parity4=int(c.parity4))
    if c.Z > 1:
        kw.update(sa=c.M * c.lda, sw=0 if c.shared_w else c.N * c.K, sc=c.M * c.ldc, sr=c.M * c.ldr)
    if c.parity4:
        kw.update(sw=c.N * c.K)
    if c.sub:
        kw.update(oH=c.oH, oW=c.oW, osy=c.sub[0], osx=c.sub[1], ooy=c.sub[2], oox=c.sub[3])
    for name, ld, kname, xe, kval in (('a2', 'lda2', 'K1', x2, c.K1), ('a3', 'lda3', 'K2', x3, c.K1 + c.x2)):
        if xe is not None:
            b = _in(c.M, xe.shape[1] + c.vec, c.dt, xe)
            ins.append(b)
            kw.update({name: b.ptr, ld: b.ld, kname: kval})
    if c.bias:
        b = _in(1, c.M if c.bias_m else c.N, F32, (bias_m if c.bias_m else bias)[None], off=4 + c.bias_off)
        ins.append(b)
        kw.update(bias=b.ptr)
    if c.rowvec:
        b = _in(c.B, c.ldrv, F32, rv, off=4 + c.rv_off)
        ins.append(b)
        kw.update(rowvec=b.ptr, ldrv=c.ldrv)
    if c.res:
        b = _in(c.rows, c.ldr, c.odt, res, off=8 + c.res_off, rowidx=rowidx)
        ins.append(b)
        kw.update(residual=b.ptr, ldr=c.ldr)
    kw.update(split_k=c.split_k if c.split_k else (0 if c.ws else 1))
    ws = None
    if c.ws:
        # the workspace is exactly splits * M * N floats + a poisoned tail (the plan is a host-side query that reads no
        # memory: any non-null workspace tells it that splitting is allowed)
        plan = _L().query('sdmi_igemm_split_plan', **{**kw, 'workspace': 64})
        ws = _Buf(1, plan * c.M * c.N, F32, POISON_OUT, tail=1024)
        kw.update(workspace=ws.ptr)
    before = [b.flat.clone() for b in ins]

    out = _out(c)
    _call('sdmi_igemm', out=out.ptr, **kw)
    name, splits = _route_name(_L().lib().sdmi_igemm_last_route())
    want = c.route.replace(' splitP', f' split{_plan(c)}' if _plan(c) > 1 else '')
    assert name == want, f'{c.id}: expected {want}, got {name}'
    got_flat = out.flat.cpu()
    got = out.mat(got_flat)[rowidx, :c.N].clone()
    rest = got_flat.clone()
    out.mat(rest)[rowidx, :c.N] = POISON_OUT
    assert _same_bits(rest, torch.full_like(rest, POISON_OUT)), \
        f'{c.id}: the launch wrote outside its [:M, :N] (pitch gap, guard rows or foreign pixels)'
    if ws is not None:
        assert splits == (plan if plan > 1 else 1), (splits, plan)
        tail = ws.flat[splits * c.M * c.N:] if splits > 1 else ws.flat
        assert _same_bits(tail, torch.full_like(tail, POISON_OUT)), f'{c.id}: workspace written past splits * M * N'
    # repeatability
    out2 = _out(c)
    _call('sdmi_igemm', out=out2.ptr, **kw)
    assert _same_bits(out2.flat, out.flat), f'{c.id}: a second launch gave other bits'
    # deferred second stage = direct
    if splits > 1 and c.act is None and c.ldc == c.N and not c.bias_m:
        out3 = _out(c)
        _call('sdmi_igemm', out=out3.ptr, defer_epilogue=1, **kw)
        assert _same_bits(out3.flat, torch.full_like(out3.flat, POISON_OUT)), f'{c.id}: the deferred launch wrote to out'
        record = _L().lib().sdmi_igemm_last_route()
        _call('sdmi_splitk_finish', out=out3.ptr, **{**kw, 'split_k': splits})
        assert _same_bits(out3.flat, out.flat), f'{c.id}: deferred + sdmi_splitk_finish differs from the direct launch'
        assert _L().lib().sdmi_igemm_last_route() == record, 'sdmi_splitk_finish changed the route record'
    assert all(_same_bits(b.flat, t) for b, t in zip(ins, before)), f'{c.id}: the launch changed its inputs'
    return got, (splits if splits > 1 else 0), name


def _act64(z, kind):
    return {'silu': F.silu, 'gelu': F.gelu, 'relu': F.relu}[kind](z) if kind else z


# ---- the tests -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', DERIVED, ids=lambda c: c.id)
def test_pinned(c):
    """Gaussian operands (weights scaled by K^-1/2).  derived bound on z (expf bound behind silu / gelu), bf16 storage on
    top; bit-exact: the route, everything around the output, the workspace tail, repeatability, deferred = direct, the
    inputs."""
    got, s, route = _launch(c, False)
    z, A = _reference(c, False)
    got = got.double()
    assert bool(torch.isfinite(got).all()), c.id
    bound = (c.K + s + 3) * U * A + 4 * U * z.abs()
    exact = _act64(z, c.act)
    form = None
    if c.act in ('silu', 'gelu'):
        form = 'act_apply' if (c.odt == F32 or s) else 'act_apply<true>'
        r, a = EXPF[form]
        bound = LIP[c.act] * bound + a
    err = (got - exact).abs()
    bf = c.odt == BF16
    if form:
        before_rounding = (err - BF * exact.abs()) / (1 + BF) if bf else err
        need = ((before_rounding - bound).clamp_min(0.0) / exact.abs().clamp_min(1e-300)).max()
        NEED[f'{form} r'] = max(NEED.get(f'{form} r', 0.0), float(need))
        bound = bound + r * exact.abs()
    if bf:
        bound = bound + BF * (exact.abs() + bound)
    share = float((err / bound.clamp_min(1e-300)).max())
    key = f'{route} [{_ID[c.odt]} out] err/bound'
    NEED[key] = max(NEED.get(key, 0.0), share)
    print(f'{c.id}: {route}, largest err/bound {share:.3f}')
    assert bool((err <= bound).all()), f'{c.id} ({route}): {_worst(err, bound)}'


@pytest.mark.parametrize('c', EXACT, ids=lambda c: c.id)
def test_exact(c):
    """Exact arithmetic (module docstring): the output equals the integer reference in every bit.  No tolerance."""
    if c.act or c.alpha != 1.0:
        c = types.SimpleNamespace(**{**vars(c), 'act': None, 'alpha': 1.0})
    got, _, route = _launch(c, True)
    z, _ = _reference(c, True)
    assert float(z.abs().max()) < 256.0
    want = z.to(c.odt)
    if not _same_bits(got, want):
        bad = (got.double() != z).nonzero()
        i, j = (int(v) for v in bad[0])
        raise AssertionError(f'{c.id} ({route}): {len(bad)} elements differ, first at row {i} column {j}: '
                             f'got {float(got[i, j])}, exact {float(z[i, j])}')
