"""Kernel providers used by engine.py.

`Kern`      -- inference: direct libsdmi launches (no autograd bookkeeping, fused epilogues).
`KernGrad`  -- training: the same operations as `torch.autograd.Function`s whose backward passes are
               libsdmi kernels too (dgrad = the implicit-GEMM kernel on a flipped operand, wgrad,
               GroupNorm/LayerNorm/attention backward ...).  Parameter gradients are written by
               the kernels straight into the model's flat fp32 gradient arena (`p.grad` views),
               so autograd only routes activation gradients.

Both resolve weights through a WeightBank: fp32 operands are views of the master arena, bf16
operands views of the bf16 shadow arena (same offsets); only channel-padded and non-adjacent
fused operands are materialised.
"""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _lib, bwd, derived, ops, policy
from ._lib import call

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def _p(t):
    return 0 if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


_DEBUG = False            # (set by hand: prints the norm of every gradient the backward kernels produce)


def _dbg(tag, **tensors):
    if _DEBUG:
        msg = ' '.join(f'{k}={float(v.float().norm()):.4e}' if v is not None else f'{k}=None'
                       for k, v in tensors.items())
        print(f'[bwd] {tag}: {msg}', flush=True)


FP8_ACT_SCALE = 8.0        # activations -> e4m3fn: +-56 representable, 2^-9 resolution near zero
_LAZY_CAT = bool(policy.flag('LAZY_CAT'))
_GEGLU_FUSE = bool(policy.flag('GEGLU_FUSE'))     # training: GEGLU in the FF GEMM's epilogue


class CatPair:
    """Two NHWC tensors standing for their channel concatenation (inference: read in place)."""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.shape = tuple(a.shape[:-1]) + (a.shape[-1] + b.shape[-1],)
        self.dtype, self.device = a.dtype, a.device

    def dim(self):
        return self.a.dim()

    def materialize(self):
        return ops.concat_channels(self.a, self.b)


_RES_MERGE = bool(policy.flag('RES_MERGE'))
_FF_MERGE = bool(policy.flag('FF_MERGE'))
_CROSS_FOLD = bool(policy.flag('CROSS_FOLD'))
_CROSS_MAX_SLOTS = 16      # most slots the folded cross-attention path takes (16-row groups per head from 9 slots)
_LN_FOLD = bool(policy.flag('LN_FOLD'))
_ST_FUSED = bool(policy.flag('ST_FUSED'))     # fused SpatialTransformer block (sdmi_st_block)
_ST_FF_SPLIT = bool(policy.flag('ST_FF_SPLIT'))   # ... its feed-forward over workgroup pairs where the grid is half the chip
_WGRAD_HALO = bool(policy.flag('WGRAD_HALO'))    # direct 3x3 weight gradient on channel pairs (wgrad3x3_halo_kernel)
_CROSS_ONE = 64            # folded slot cross-attention as ONE launch (sdmi_cross_fold) up to this many tokens per image
_ROLLOUT_FUSED = bool(policy.flag('ROLLOUT_FUSED'))   # fused SlotFormer rollout layer (sdmi_rollout_layer)
_UPS_PARITY = bool(policy.flag('UPS_PARITY'))   # upsample convolutions as four 2x2 parity convolutions in one launch
_UPS_TRAIN = policy.flag('UPS_PARITY') == 1     # ... and trained as the 4x4 stride-2 transposed convolutions they are
# the fused inference block only when its grid (one workgroup per 64 / 32 token rows) fills a good part of the chip: at
# B = 64 the 8^2 level gives 64 workgroups that each stream the block's 4 MB of weights -- 119 us against 108 us for the
# per-layer launches (tests set these module variables)
_ST_MIN_WGS = 128
# token rows per workgroup: 0 = 64 when that gives >= 192 workgroups, else 32; 64 / 32 force one
_ST_ROWS = 0


def _copy_group(items):
    """[(src ptr, dst ptr, bytes)] -> sdmi_copy_group launches of up to 32 copies each."""
    for c0 in range(0, len(items), 32):
        arr = _lib.struct_array('SdmiCopyItem', (dict(src=sp, dst=dp, bytes=nb) for sp, dp, nb in items[c0:c0 + 32]))
        call('sdmi_copy_group', _st(), items=ctypes.addressof(arr), n=len(arr))


def _scatter_add(segs):
    """[(src ptr, dst ptr, fp32 count)]: dst += src, one sdmi_scatter_add launch per 32 segments."""
    for c0 in range(0, len(segs), 32):
        arr = _lib.struct_array('SdmiScatterItem', (dict(src=sp, dst=dp, count=cnt) for sp, dp, cnt in segs[c0:c0 + 32]))
        call('sdmi_scatter_add', _st(), items=ctypes.addressof(arr), n=len(arr))


# ------------------------------------------------------------------------------------------
# weight streams of the fused SpatialTransformer block (csrc/st_fused.hip): per-wave sequences of 2 KB
# units = the XOR-swizzled LDS image of 16 weight rows x 64 k, in the order the kernel multiplies them
# ------------------------------------------------------------------------------------------
def _st_unit_index(entries):
    """entries[w] = [(element offset of the matrix, row pitch, first row, first k), ...] per unit, 8 waves
    -> int64 [8 * U * 1024] gather index into the flat source (unit byte b of wave w, unit u at
    ((w * U + u) * 1024 + b / 2)): physical 16-byte chunk p of row r holds logical chunk p ^ ((r >> 1) & 7)."""
    r = np.arange(16, dtype=np.int64)[:, None, None]
    p_ = np.arange(8, dtype=np.int64)[None, :, None]
    e = np.arange(8, dtype=np.int64)[None, None, :]
    col = (p_ ^ ((r >> 1) & 7)) * 8 + e                       # [16, 8, 8]
    out = []
    for ent in entries:
        for off, ld, row0, k0 in ent:
            out.append((off + (row0 + r) * ld + k0 + col).reshape(-1))
    return torch.from_numpy(np.concatenate(out))


def st_geometry(C):
    NSL, KT = C // 128, C // 64
    return dict(NSL=NSL, KT=KT, NHC=C // 32, R=C // 32 * 8, UA=4 * KT * NSL, UB1=KT * NSL,
                UIMG=KT + 2 * NSL, UB2=KT * NSL + (C // 32) * (2 * KT + 2 * NSL))


def st_index_a(C):
    """Phase A source = [W_in (C x C) | W_q' | W_k' | W_v' (C x C each)] flat."""
    g = st_geometry(C)
    ent = []
    for w in range(8):
        e = []
        for m in range(4):                                  # proj_in, q, k, v
            for kt in range(g['KT']):
                for s_ in range(g['NSL']):
                    e.append((m * C * C, C, (w * g['NSL'] + s_) * 16, kt * 64))
        ent.append(e)
    return _st_unit_index(ent)


def st_index_b(C):
    """Phase B shared source = [W_o (C x C) | W_po (C x C) | W_1' (8C x C) | W_m = W_po W_ff (C x 4C)] flat."""
    g = st_geometry(C)
    NSL, KT = g['NSL'], g['KT']
    o_po, o_1, o_m = C * C, 2 * C * C, 2 * C * C + 8 * C * C
    ent = []
    for w in range(8):
        e = []
        for kt in range(KT):                                # attn1.to_out
            for s_ in range(NSL):
                e.append((0, C, (w * NSL + s_) * 16, kt * 64))
        for kt in range(KT):                                # x2 @ W_po^T
            for s_ in range(NSL):
                e.append((o_po, C, (w * NSL + s_) * 16, kt * 64))
        for hc in range(g['NHC']):
            for kt in range(KT):                            # value | gate rows of hidden chunk hc
                e.append((o_1, C, hc * 128 + w * 16, kt * 64))
                e.append((o_1, C, 4 * C + hc * 128 + w * 16, kt * 64))
            for k2 in range(2):                             # the chunk's 128 k of the merged output weight
                for s_ in range(NSL):
                    e.append((o_m, 4 * C, (w * NSL + s_) * 16, hc * 128 + k2 * 64))
        ent.append(e)
    return _st_unit_index(ent)


def st_index_img(C):
    """Per-image source = [Wq[b] padded to 128 rows (128 x C) | W2[b] with K padded to 128 (C x 128)] flat."""
    g = st_geometry(C)
    ent = []
    for w in range(8):
        e = [(0, C, w * 16, kt * 64) for kt in range(g['KT'])]
        for k2 in range(2):
            for s_ in range(g['NSL']):
                e.append((128 * C, 128, (w * g['NSL'] + s_) * 16, k2 * 64))
        ent.append(e)
    return _st_unit_index(ent)


def rollout_index_a(C=256):
    """Phase A of the fused rollout layer (csrc/rollout_layer.hip): source = [W_q' | W_k' | W_v'] (3C x C) flat."""
    NSL, KT = C // 128, C // 64
    return _st_unit_index([[(m * C * C, C, (w * NSL + s_) * 16, kt * 64)
                            for m in range(3) for kt in range(KT) for s_ in range(NSL)] for w in range(8)])


def rollout_index_b(C, F):
    """Phase B source = [W_o (C x C) | W_1' (F x C) | W_2 (C x F)] flat: out_proj, then per hidden chunk of 128 the
    chunk's linear1 rows and its 128 k of linear2."""
    NSL, KT = C // 128, C // 64
    o1, o2 = C * C, C * C + F * C
    ent = []
    for w in range(8):
        e = [(0, C, (w * NSL + s_) * 16, kt * 64) for kt in range(KT) for s_ in range(NSL)]
        for hc in range(F // 128):
            e += [(o1, C, hc * 128 + w * 16, kt * 64) for kt in range(KT)]
            e += [(o2, F, (w * NSL + s_) * 16, hc * 128 + k2 * 64) for k2 in range(2) for s_ in range(NSL)]
        ent.append(e)
    return _st_unit_index(ent)


# Physion readout on sdmi_readout_fwd / sdmi_readout_bwd wherever the kernels cover the geometry (readout_covers); the
# rest, and everything with this off (tests, tools/bench_readout.py), runs engine.readout_composed.  Not a policy
# switch: the choice is geometric.
_READOUT_FUSED = True
# The VQA test stage (slotdiffusion_amd/vqa.py) on sdmi_vqa_score wherever readout_covers and vqa_score_covers hold; the
# rest, and everything with this off (tests, tools/bench_vqa_test.py), runs the composed stage.  Geometric as well.
_VQA_FUSED = True
READOUT_AGG = {'sum': _lib.ENUMS['SDMI_AGG_SUM'], 'mean': _lib.ENUMS['SDMI_AGG_MEAN'], 'max': _lib.ENUMS['SDMI_AGG_MAX']}
_READOUT_INDEX = {}


def readout_covers(N, C, F):
    """Geometry of sdmi_readout_fwd / sdmi_readout_bwd (sdmi.h)."""
    return 2 <= N <= 16 and 32 <= C <= 256 and C % 32 == 0 and 32 <= F <= 256 and F % 32 == 0


def vqa_score_covers(N, C, F, W, K, J):
    """Geometry of sdmi_vqa_score (sdmi.h): the readout's, and the bank / threshold / task counts."""
    return readout_covers(N, C, F) and 1 <= W <= 65535 and 1 <= K <= 32 and 1 <= J <= 64


def readout_pack_index(C, F, dtype, device='cpu'):
    """int64 [F * 2C]: position in linear1.weight [F, 2C] (flat) of every element of the packed operand `w1p` of
    sdmi_readout_fwd (sdmi.h) -- per 32-feature chunk and k step, the MFMA B fragments of W_a then W_b, lane by lane."""
    key = (C, F, dtype, str(device))
    if key not in _READOUT_INDEX:
        kw, ke = (16, 8) if dtype == torch.bfloat16 else (8, 4)      # k per step, k per lane
        ar = lambda n: torch.arange(n, device=device)
        fc, ks, h, l, e = torch.meshgrid(ar(F // 32), ar(C // kw), ar(2), ar(64), ar(ke), indexing='ij')
        row = 32 * fc + l % 32
        col = h * C + kw * ks + ke * (l // 32) + e
        _READOUT_INDEX[key] = (row * (2 * C) + col).reshape(-1)
    return _READOUT_INDEX[key]


# SAVi slot transition (ResidualMLPPredictor / RNNPredictorWrapper) as ONE sdmi_pred_step launch wherever the kernel
# covers the geometry (pred_step_covers) on a bf16 model that records no gradient; the rest, and everything with this off
# (tests, tools/bench_pred.py), runs the composed chain engine.slot_transition.  Not a policy switch.
_PRED_FUSED = True
_PRED_INDEX = {}


def pred_step_covers(D, H):
    """Geometry of sdmi_pred_step (sdmi.h): both multiples of 32 inside its LDS budget.  H = 0: no LSTM wrapper."""
    return 32 <= D <= 256 and D % 32 == 0 and (H == 0 or (32 <= H <= 512 and H % 32 == 0))


def pred_pack_index(N, K, gates=1, device='cpu'):
    """int64 [N * K]: position in a weight [N, K] (flat) of every element of its packed operand for sdmi_pred_step
    (sdmi.h) -- per chunk of 16 output rows and k step of 32, the MFMA B fragment lane by lane (lane l: row l % 16,
    columns 8 (l // 16) ..).  gates = 4: the LSTM's [4H, K]; a chunk is 16 hidden units and holds the i, f, g, o
    fragments of every k step side by side."""
    key = (N, K, gates, str(device))
    if key not in _PRED_INDEX:
        ar = lambda n: torch.arange(n, device=device)
        per = N // gates
        c, s, g, l, e = torch.meshgrid(ar(per // 16), ar(K // 32), ar(gates), ar(64), ar(8), indexing='ij')
        row = g * per + 16 * c + l % 16
        col = 32 * s + 8 * (l // 16) + e
        _PRED_INDEX[key] = (row * K + col).reshape(-1)
    return _PRED_INDEX[key]


def pred_pack(W, base, wrap, device=None):
    """Operands of sdmi_pred_step out of a {key: tensor} dict: `base` = key prefix of a ResidualMLPPredictor or None,
    `wrap` = key prefix of the RNNPredictorWrapper's own tensors or None.  Weights are rounded to bf16 and packed
    (pred_pack_index); [W_ih | W_hh] is one operand over K = D + H and b_ih + b_hh one vector."""
    out = {}
    dev = device or next(iter(W.values())).device
    pk = lambda w, gates=1: w.to(dev).to(torch.bfloat16).reshape(-1)[
        pred_pack_index(w.shape[0], w.shape[1], gates, dev)].contiguous()
    f = lambda k: W[k].detach().to(dev).float().contiguous()
    if base is not None:
        out.update(ln_g=f(base + '.ln.weight'), ln_b=f(base + '.ln.bias'), w1p=pk(f(base + '.mlp.0.weight')),
                   b1=f(base + '.mlp.0.bias'), w2p=pk(f(base + '.mlp.2.weight')), b2=f(base + '.mlp.2.bias'))
    if wrap is not None:
        wg = torch.cat([f(wrap + '.rnn.weight_ih_l0'), f(wrap + '.rnn.weight_hh_l0')], 1)
        out.update(wgp=pk(wg, 4), bg=(f(wrap + '.rnn.bias_ih_l0') + f(wrap + '.rnn.bias_hh_l0')).contiguous(),
                   wop=pk(f(wrap + '.out_projector.weight')), bo=f(wrap + '.out_projector.bias'),
                   H=wg.shape[0] // 4)
    return out


# the transformer slot transition (predictor.py:20-44) as ONE sdmi_pred_tf launch in engine.encode_stream: bf16 inference
# inside this geometry.  Off (tests, tools/bench_extract.py): the stream runs engine.slot_transition, so both sides of an
# A/B run in one process.  Like _PRED_FUSED not a policy switch: the policy table is at the size test_host_cpu.py caps.
_PRED_TF = True
_PRED_TF_MATS = (('wqkv', 'self_attn.in_proj_weight'), ('wo', 'self_attn.out_proj.weight'), ('w1', 'linear1.weight'),
                 ('w2', 'linear2.weight'))
_PRED_TF_VECS = (('ln1_g', 'norm1.weight'), ('ln1_b', 'norm1.bias'), ('bqkv', 'self_attn.in_proj_bias'),
                 ('bo', 'self_attn.out_proj.bias'), ('ln2_g', 'norm2.weight'), ('ln2_b', 'norm2.bias'),
                 ('b1', 'linear1.bias'), ('b2', 'linear2.bias'))


def pred_tf_covers(N, D, heads, ffn, layers):
    """Geometry of sdmi_pred_tf (sdmi.h): one 16-row tile of slots, head dims on the 16-deep MFMA, inside its LDS
    budget."""
    if heads < 1 or D % heads:
        return False
    hd = D // heads
    return (1 <= N <= 16 and 32 <= D <= 256 and D % 32 == 0 and hd % 16 == 0 and hd <= 64 and
            32 <= ffn <= 1024 and ffn % 32 == 0 and 1 <= layers <= 4)


def pred_tf_pack(W, base, layers, device=None):
    """Operands of sdmi_pred_tf out of a {key: tensor} dict: `base` = key prefix of the TransformerPredictor.  Every
    matrix is rounded to bf16 and packed (pred_pack_index), the layers' operands one behind the other; the vectors are
    fp32 [layers, n].  F = ffn width."""
    dev = device or next(iter(W.values())).device
    f = lambda i, k: W[f'{base}.transformer_encoder.layers.{i}.{k}'].detach().to(dev).float().contiguous()
    pk = lambda w: w.to(torch.bfloat16).reshape(-1)[pred_pack_index(w.shape[0], w.shape[1], 1, dev)]
    out = {k: torch.cat([pk(f(i, n)) for i in range(layers)]).contiguous() for k, n in _PRED_TF_MATS}
    out.update({k: torch.stack([f(i, n) for i in range(layers)]).contiguous() for k, n in _PRED_TF_VECS})
    out.update(F=out['b1'].shape[1], layers=layers)
    return out


# the glue between two steps of the fused SlotFormer rollout (tail tokens, out_proj, cast, in_proj, window shift, positions)
# as ONE sdmi_rollout_feed launch in engine.slot_rollout(feed=True), which LDMSlotFormer.unroll takes for bf16 inference
# inside rollout_feed_covers.  Off (tests, tools/bench_rollout_stage.py): unroll is rollout().  Like _PRED_TF not a policy
# switch.
_ROLLOUT_FEED = True


def rollout_feed_covers(N, L, Lp, C, Ds):
    """Geometry of sdmi_rollout_feed (sdmi.h): the N newest token rows are one 16-row tile, the window is whole steps of
    N rows inside its Lp rows, both widths are multiples of the 32-deep MFMA inside the kernel's LDS arrays."""
    return (1 <= N <= 16 and N <= L <= Lp and L % N == 0 and 32 <= C <= 256 and C % 32 == 0 and
            32 <= Ds <= 256 and Ds % 32 == 0)


def rollout_feed_pack(w_out, b_out, w_in, b_in, device=None):
    """Operands of sdmi_rollout_feed: out_proj.weight [Ds, C] and in_proj.weight [C, Ds] rounded to bf16 and packed
    (pred_pack_index), the biases fp32."""
    dev = device or w_out.device
    pk = lambda w: w.detach().to(dev).to(torch.bfloat16).reshape(-1)[
        pred_pack_index(w.shape[0], w.shape[1], 1, dev)].contiguous()
    f = lambda b: b.detach().to(dev).float().contiguous()
    return dict(wout=pk(w_out), bout=f(b_out), win_w=pk(w_in), bin=f(b_in), C=w_out.shape[1], Ds=w_out.shape[0])


def st_train_units(C):
    """Unit order of the training kernels' weight streams (csrc/st_train.hip), per wave: lists of
    (matrix key, first row, first k, transposed).  Forward: a = [proj_in | q | k | v], b = [to_out | q2 | to_out2 | per
    hidden chunk: ff1 value rows, ff1 gate rows, ff2 k-chunk | proj_out].  Backward (rows / k of the TRANSPOSED
    matrices): b1 = [proj_out^T | per hidden chunk: ff2^T rows, ff1^T value k-chunk, gate k-chunk | to_out2^T],
    b2 = [q2^T | to_out^T], ba = [q^T | k^T | v^T | proj_in^T]."""
    NSL, KT, NHC = C // 128, C // 64, C // 32
    out = dict(a=[], b=[], b1=[], b2=[], ba=[])
    for w in range(8):
        full = lambda m, tr: [(m, (w * NSL + s_) * 16, kt * 64, tr) for kt in range(KT) for s_ in range(NSL)]
        a = [u for m in ('in', 'q', 'k', 'v') for u in full(m, False)]
        b = [u for m in ('o', 'q2', 'o2') for u in full(m, False)]
        b1 = full('po', True)
        for hc in range(NHC):
            for kt in range(KT):
                b.append(('ff1', hc * 128 + w * 16, kt * 64, False))
                b.append(('ff1', 4 * C + hc * 128 + w * 16, kt * 64, False))
            for k2 in range(2):
                for s_ in range(NSL):
                    b.append(('ff2', (w * NSL + s_) * 16, hc * 128 + k2 * 64, False))
            b1 += [('ff2', hc * 128 + w * 16, kt * 64, True) for kt in range(KT)]
            for part in range(2):
                b1 += [('ff1', (w * NSL + s_) * 16, part * 4 * C + hc * 128 + k2 * 64, True)
                       for k2 in range(2) for s_ in range(NSL)]
        b += full('po', False)
        b1 += full('o2', True)
        out['a'].append(a)
        out['b'].append(b)
        out['b1'].append(b1)
        out['b2'].append(full('q2', True) + full('o', True))
        out['ba'].append([u for m in ('q', 'k', 'v', 'in') for u in full(m, True)])
    return out


def st_pack_descs(rows, units, mats, dst):
    """Fill `rows` (records of SdmiStPackDesc) for one unit stream: `units` (st_train_units, per wave) of the bf16
    matrices `mats` into the stream tensor `dst`, 2 KB per unit."""
    base = dst.data_ptr()
    for i, (key, r0, k0, tr) in enumerate(u for wave in units for u in wave):
        m = mats[key]
        ld = m.shape[1]
        if tr:      # unit rows walk the matrix's columns: element (r, k) = M[k0 + k][r0 + r]
            derived.put(rows, i, src=m.data_ptr() + 2 * (k0 * ld + r0), dst=base + i * 2048, rs=1, cs=ld)
        else:
            derived.put(rows, i, src=m.data_ptr() + 2 * (r0 * ld + k0), dst=base + i * 2048, rs=ld, cs=1)


def ups_parity_split(w):
    """Nearest-2x upsampling followed by a 3x3 convolution (unet.py:108-121) reads only 2 x 2 DISTINCT input pixels
    per output pixel: output parity (py, px) is a 2 x 2 convolution of the low-resolution input whose taps are sums
    of the 3 x 3 taps that fall on the same input pixel -- rows: parity 0 -> {w0 | w1 + w2} at offsets (-1, 0)
    (pad top 1), parity 1 -> {w0 + w1 | w2} at offsets (0, +1) (pad bottom 1); columns alike.  16 instead of 36
    multiply-adds per output pixel and input channel.  w [Cout, Cin, 3, 3] fp32 -> {(py, px): [Cout, 2*2*Cin] fp32}
    (tap-major K, the layout sdmi_igemm takes)."""
    co, ci = w.shape[0], w.shape[1]
    taps = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}
    out = {}
    for py in (0, 1):
        for px in (0, 1):
            we = torch.zeros((co, 2, 2, ci), dtype=torch.float32, device=w.device)
            for r in (0, 1):
                for c in (0, 1):
                    for ky in taps[py][r]:
                        for kx in taps[px][c]:
                            we[:, r, c, :] += w[:, :, ky, kx]
            out[py, px] = we.reshape(co, 4 * ci)
    return out


# The same layer as ONE transposed convolution: ConvTranspose2d(4, stride 2, padding 1) of the low-resolution input with
# the composite filter W4 -- per dimension composite tap u gathers the source taps UPS_TAPS[u].  The training path
# (GemmFn, WeightBank.ups_train_ok) makes its operands from W4 on the device (sdmi.h: SDMI_PACK_UPS_*) and folds dW4
# back with sdmi_ups_fold_dw; the two functions below are the host restatement of those kernels, sums in their order.
UPS_TAPS = ((2,), (1, 2), (0, 1), (0,))


def ups_composite(w):
    """w [Cout, Cin, 3, 3] -> W4 [Cout, Cin, 4, 4]: W4[.., u, v] = sum over ky in UPS_TAPS[u], kx in UPS_TAPS[v] of
    w[.., ky, kx], ky ascending, kx ascending inside one ky, in w's dtype.  Tap (r, c) of parity (py, px) in
    ups_parity_split is W4[.., 3 - 2r - py, 3 - 2c - px]."""
    w4 = torch.empty(w.shape[:2] + (4, 4), dtype=w.dtype, device=w.device)
    for u in range(4):
        for v in range(4):
            terms = [w[:, :, ky, kx] for ky in UPS_TAPS[u] for kx in UPS_TAPS[v]]
            acc = terms[0]
            for t in terms[1:]:
                acc = acc + t
            w4[:, :, u, v] = acc
    return w4


def ups_fold(dw4):
    """dW4 [Cout, Cin, 4, 4] -> dw [Cout, Cin, 3, 3]: the transpose of ups_composite -- dw[.., ky, kx] = sum over (u, v)
    with ky in UPS_TAPS[u], kx in UPS_TAPS[v] (u in {2 - ky, 3 - ky}), u ascending, v ascending inside one u."""
    dw = torch.empty(dw4.shape[:2] + (3, 3), dtype=dw4.dtype, device=dw4.device)
    for ky in range(3):
        for kx in range(3):
            a, b = 2 - ky, 2 - kx
            dw[:, :, ky, kx] = ((dw4[:, :, a, b] + dw4[:, :, a, b + 1]) + dw4[:, :, a + 1, b]) + dw4[:, :, a + 1, b + 1]
    return dw


class WeightBank:
    """name(s) -> GEMM operand [N, K] in the requested dtype (K padded to the vector width)."""

    def __init__(self, model, dtype):
        self.model = model
        self.t = model.tensors()
        self.dtype = dtype
        self.cache = {}
        # autograd anchor: parameters reach the kernels by name, so parameterised Functions take
        # this requires-grad dummy to make their outputs part of the graph
        self.anchor = torch.zeros(1, device=model.arena().device, requires_grad=True)
        # a second anchor for the denoiser's Functions: `autograd.grad(loss, [slots, anchor_dec])`
        # then runs exactly the denoiser's backward (and stops at the slots), so that its gradient
        # range can be all-reduced while the slot encoder's backward is still running
        self.anchor_dec = torch.zeros(1, device=model.arena().device, requires_grad=True)
        # weight-gradient launches and the ordering of everything that writes the gradient arena (bwd.GradSchedule);
        # its side streams on / off is `overlap_wgrad`
        self.sched = bwd.GradSchedule(bool(policy.flag('WGRAD_STREAM')))
        self.defer_colsum = bool(policy.flag('DEFER_COLSUM'))
        # data gradient + weight gradient of a layer in ONE launch on the main stream (sdmi_bwd_pair) where
        # bwd.plan_layer finds the layer fit for it
        self.pair_bwd = bool(policy.flag('BWD_PAIR'))
        self._fz = None
        # derived operands re-made once per optimiser step, each family by ONE launch over its device-side descriptor
        # table (derived.StepTable): dgrad operands (wd / wd_sub, one table per dtype), e4m3fn operands with device-side
        # scales (w8_dev: descriptor i = slot i of _q_amax / _q_inv) and the unit streams of the fused
        # SpatialTransformer training kernels (st_train_streams)
        self.dgrad_ops = derived.StepTable('dgrad operand', 'SdmiPackDesc', self._dgrad_fill, self._dgrad_launch,
                                           self._dgrad_first, self._arena_ptrs)
        self._q_amax = self._q_inv = None
        self.fp8_ops = derived.StepTable('fp8 operand', 'SdmiFp8Desc', self._fp8_fill, self._fp8_launch,
                                         lambda m, one: self._fp8_launch(None, one(), m.slot),       # on its own slot
                                         lambda: self._arena_ptrs() + (_p(self._q_amax), _p(self._q_inv)))
        self.st_streams = derived.StepTable('fused training block', 'SdmiStPackDesc', self._st_fill, self._st_launch,
                                            lambda m, one: self._st_launch(None, one()), self._arena_ptrs)

    def anchor_for(self, names):
        n = names if isinstance(names, str) else names[0]
        return self.anchor_dec if n.startswith('dm_decoder') else self.anchor

    overlap_wgrad = property(lambda self: self.sched.overlap, lambda self, on: setattr(self.sched, 'overlap', bool(on)))

    def queue_colsum(self, partial, nblk, C, out0, out1, after=None):
        self.sched.queue_colsum(partial, nblk, C, out0, out1, after)

    def join_by_hand(self):
        """Backward kernels called outside an autograd pass: the caller calls join() itself."""
        self.sched.join_by_hand()

    def join(self):
        self.sched.join()

    def invalidate(self):
        """The master weights changed (optimiser step / checkpoint load): derived operands of
        TRAINABLE parameters are dropped; those of frozen ones (VQ-VAE, DINO ViT) stay valid."""
        fz = self._frozen_names()
        keep = {}
        for key, val in self.cache.items():
            names = key[0] if (isinstance(key, tuple) and isinstance(key[0], tuple)) else \
                (key[1] if (isinstance(key, tuple) and key[0] == 'bias') else None)
            if names is not None and all(n in fz for n in names):
                keep[key] = val
        self.cache = keep
        for fam in (self.dgrad_ops, self.fp8_ops, self.st_streams):
            fam.mark_stale()

    def _frozen_names(self):
        if self._fz is None:
            self._fz = {p.name for p in getattr(self.model, '_spec', []) if not p.trainable}
        return self._fz

    def _arena_ptrs(self):
        """Base pointers of the arenas the derived operands are made from (derived.StepTable's source check)."""
        m = self.model
        return (m.arena().data_ptr(), m.shadow_arena().data_ptr() if m.compute_dtype != torch.float32 else None)

    def f(self, name):
        return self.t[name]

    def _flat(self, name, dtype):
        """Operand view straight out of the (master | shadow) arena; None if it needs padding."""
        p = self.t[name]
        vec = ops.vec_of(dtype)
        if p.dim() == 4:
            co, ci, kh, kw = p.shape
            if ci % vec:
                return None
            shape = (co, kh * kw * ci)
        else:
            if p.shape[-1] % vec:
                return None
            shape = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, p.numel())
        if dtype == torch.float32:
            src = self.model.arena_slice(name)
        else:
            src = self.model.arena_slice(name, self.model.shadow_arena())
        return src.view(shape)

    def w(self, names, dtype=None):
        dtype = dtype or self.dtype
        if isinstance(names, str):
            names = (names,)
        key = (names, dtype)
        if key in self.cache:
            return self.cache[key]
        parts = [self._flat(n, dtype) for n in names]
        out = None
        if all(p is not None for p in parts):
            adjacent = all(parts[i].data_ptr() + parts[i].numel() * parts[i].element_size() ==
                           parts[i + 1].data_ptr() for i in range(len(parts) - 1))
            if len(parts) == 1:
                out = parts[0]
            elif adjacent:                                 # fused operand = one arena slice
                k = parts[0].shape[1]
                n = sum(p.shape[0] for p in parts)
                base = self.model.arena() if dtype == torch.float32 else self.model.shadow_arena()
                o = self.model._offsets[names[0]][0]
                out = base[o:o + n * k].view(n, k)
        if out is None and all(p is not None for p in parts) and len({p.shape[1] for p in parts}) == 1:
            # operand views exist but are not adjacent (the 22 time-embedding projections): gather them
            # with ONE grouped copy instead of a cast + a copy per part
            out = torch.empty((sum(p.shape[0] for p in parts), parts[0].shape[1]), dtype=dtype,
                              device=parts[0].device)
            o, items = 0, []
            for p in parts:
                items.append((_p(p), _p(out[o:]), p.numel() * p.element_size()))
                o += p.shape[0]
            _copy_group(items)
        if out is None:
            mats = []
            vec = ops.vec_of(dtype)
            for nme in names:
                p = self.t[nme]
                if p.dim() == 4:
                    co, ci, kh, kw = p.shape
                    flat = self.model.arena_slice(nme).view(co * kh * kw, ci)
                    cpad = (ci + vec - 1) // vec * vec
                    mats.append(ops.cast2d(flat, dtype, cols=ci, ldd=cpad).view(co, kh * kw * cpad))
                else:
                    k = p.shape[1]
                    kpad = (k + vec - 1) // vec * vec
                    mats.append(ops.cast2d(self.model.arena_slice(nme).view(p.shape[0], k), dtype,
                                           cols=k, ldd=kpad))
            if len(mats) == 1:
                out = mats[0]
            else:
                out = torch.empty((sum(m.shape[0] for m in mats), mats[0].shape[1]), dtype=dtype,
                                  device=mats[0].device)
                o = 0
                for m in mats:
                    ops.cast2d(m, dtype, out=out[o:o + m.shape[0]])
                    o += m.shape[0]
        self.cache[key] = out
        return out

    def w8(self, name):
        """e4m3fn operand of a conv / linear weight with its per-tensor scale: (bytes [N][K],
        1 / scale), scale = 448 / amax.  Weight preparation (inference: once per weight update); the
        amax read-back synchronises, so the first use must precede any graph capture (the samplers'
        warm-up pass does)."""
        key = ('fp8', name)
        if key not in self.cache:
            p = self.t[name]
            flat = self._flat(name, torch.float32)
            if flat is None:
                raise _lib.SdmiError(f'{name}: fp8 operands need 16-byte input-channel rows')
            amax = float(p.detach().abs().max())
            scale = 448.0 / max(amax, 1e-12)
            self.cache[key] = (ops.quant_fp8(flat.float().contiguous(), scale), 1.0 / scale)
        return self.cache[key]

    W8_SLOTS = 1024

    def w8_dev(self, name):
        """e4m3fn operand of a TRAINABLE conv / linear weight with a scale the device derives from the tensor's own
        amax: (bytes [N][K], inv = one-element fp32 view holding amax / 448 -- SdmiGemmArgs.alpha_dev).  The operands
        live in persistent buffers; after an optimiser step (invalidate()) the first request re-quantises ALL of
        them from the fp32 master arena with one sdmi_fp8_quant_group call (memset + amax launch + quantise launch,
        descriptor table on the device, no read-back) -- part of the captured train step, so every replay
        quantises the weights it multiplies with."""
        m = self.fp8_ops.get(name)
        if m is None:
            flat = self._flat(name, torch.float32)
            if flat is None or flat.numel() % 16:
                raise _lib.SdmiError(f'{name}: fp8 operands need 16-byte input-channel rows')
            if self._q_amax is None:
                self._q_amax = torch.zeros(self.W8_SLOTS, dtype=torch.int32, device=flat.device)
                self._q_inv = torch.zeros(self.W8_SLOTS, dtype=torch.float32, device=flat.device)
            slot = len(self.fp8_ops.members)
            if slot >= self.W8_SLOTS:
                raise _lib.SdmiError('fp8 operand table full')
            m = self.fp8_ops.add(name, SimpleNamespace(q=torch.empty(flat.shape, dtype=torch.uint8, device=flat.device),
                                                       inv=self._q_inv[slot:slot + 1], src=flat, slot=slot), flat.device)
        return m.q, m.inv

    @staticmethod
    def _fp8_fill(m, rows, blk):
        derived.put(rows, 0, src=m.src.data_ptr(), dst=m.q.data_ptr(), n=m.src.numel(), block_begin=blk)
        return blk + (m.src.numel() + 4095) // 4096

    def _fp8_launch(self, _, tab, slot=0):
        call('sdmi_fp8_quant_group', _st(), descs=_p(tab.dev), n_desc=tab.rows, src_dtype=_lib.F32,
             total_blocks=tab.blocks, amax_bits=_p(self._q_amax[slot:]), inv_scale=_p(self._q_inv[slot:]))

    def fp8_train_ok(self, x, wnames, geom):
        """Training forward in the fp8 configuration (models.set_compute_dtype('fp8')): the denoiser's 3x3
        convolutions multiply e4m3fn operands -- the layers Kern.fp8_ok names at inference; the backward pass keeps
        bf16 operands (the saved activation and the bf16 shadow weights)."""
        kh, kw, stride, pad, ups = geom
        return (getattr(self.model, 'fp8_unet', False) and isinstance(wnames, str) and x.dim() == 4
                and x.dtype == torch.bfloat16 and kh * kw > 1 and not ups and x.shape[-1] % 16 == 0
                and x.shape[-1] >= 64 and wnames.startswith(self.model.fp8_prefix))

    def conv_skip_weights(self, n, dtype):
        """[W_out3 (3x3, tap-major K) | W_skip (1x1)] along K and the summed bias of ResBlock `n`: its second
        convolution and its skip convolution as ONE implicit GEMM (sdmi.h: a2 / a3).  Cached."""
        key = ('convskip', n, dtype)
        if key not in self.cache:
            with torch.no_grad():
                w2 = self.w(n + '.out_layers.3.weight', dtype)
                ws = self.w(n + '.skip_connection.weight', dtype)
                w = torch.cat([w2.reshape(w2.shape[0], -1), ws.reshape(ws.shape[0], -1)], 1).contiguous()
                b = (self.t[n + '.out_layers.3.bias'].float() + self.t[n + '.skip_connection.bias'].float())
                self.cache[key] = (w, b.contiguous())
        return self.cache[key]

    def ups_parity_weights(self, wname, dtype):
        """{(py, px): [Cout][2][2][Cin] in `dtype`} of an upsample convolution (ups_parity_split).  Cached."""
        key = ('upsparity', wname, dtype)
        if key not in self.cache:
            with torch.no_grad():
                parts = ups_parity_split(self.t[wname].float())
                w4 = torch.stack([parts[py, px] for py in (0, 1) for px in (0, 1)]).to(dtype).contiguous()
                self.cache[key] = {(z >> 1, z & 1): w4[z] for z in range(4)}       # views of one [4][Cout][4 Cin] tensor
        return self.cache[key]

    def ffout_proj_weights(self, t, n, dtype):
        """Feed-forward output and proj_out of a SpatialTransformer are two linear layers with only a
        residual add in between (attention.py:250-251, 305-308):
            out = (g Wff^T + bff + tres) Wpo^T + bpo + xres = [g | tres] [Wpo Wff | Wpo]^T + (Wpo bff + bpo) + xres
        -> combined weight [C, 4C + C] in `dtype` and fp32 bias (weight preparation, cached)."""
        key = ('ffoutproj', t, dtype)
        if key not in self.cache:
            with torch.no_grad():
                wff, bff = self.t[t + '.ff.net.2.weight'].float(), self.t[t + '.ff.net.2.bias'].float()
                wpo = self.t[n + '.proj_out.weight'].float().reshape(wff.shape[0], -1)
                bpo = self.t[n + '.proj_out.bias'].float()
                w = torch.cat([wpo @ wff, wpo], 1).to(dtype).contiguous()
                self.cache[key] = (w, (wpo @ bff + bpo).contiguous())
        return self.cache[key]

    def cross_fold_weights(self, t, dtype):
        """Weight-side operands of the folded slot cross-attention of transformer block `t`
        (engine.UNetRunner.cross_fold): (W_q * gamma_norm2)^T [C_k, C_d], (W_q beta_norm2) [1, C_d],
        ones [1, C_k] in `dtype`.  Weight preparation, cached until the weights change."""
        key = ('crossfold', t, dtype)
        if key not in self.cache:
            with torch.no_grad():
                g, be = self.t[t + '.norm2.weight'].float(), self.t[t + '.norm2.bias'].float()
                wq = self.t[t + '.attn2.to_q.weight'].float()
                self.cache[key] = ((wq * g).t().contiguous().to(dtype).unsqueeze(0),
                                   (wq @ be).to(dtype).view(1, 1, -1).contiguous(),
                                   torch.ones((1, 1, wq.shape[1]), dtype=dtype, device=wq.device))
        return self.cache[key]

    def ln_folded(self, ln_name, wnames, bnames, dtype):
        """Operands of a LayerNorm folded into the linear layer behind it (sdmi.h: ln_colsum):
        W' = W * gamma in `dtype`, colsum[n] = sum_k W'[n][k] of the rounded W', bias' = W beta + b.
        Weight preparation, once per weight update (cached like the bf16 operand shadows)."""
        if isinstance(wnames, str):
            wnames = (wnames,)
        key = ('lnfold', ln_name, wnames, dtype)
        if key not in self.cache:
            with torch.no_grad():
                g, be = self.t[ln_name + '.weight'].float(), self.t[ln_name + '.bias'].float()
                W = torch.cat([self.t[n].float().reshape(-1, g.numel()) for n in wnames])
                Wp = (W * g).to(dtype).contiguous()
                bias = W @ be
                if bnames is not None:
                    bias = bias + self.b(bnames).float()
                self.cache[key] = (Wp, Wp.float().sum(1).contiguous(), bias.contiguous())
        return self.cache[key]

    def cf_index(self, rows, cols, device):
        key = ('cf_index', rows, cols)
        if key not in self.cache:
            self.cache[key] = ops.cross_fold_pack_index(rows, cols).to(device)
        return self.cache[key]

    def st_index(self, which, C, device):
        key = ('st_index', which, C)
        if key not in self.cache:
            self.cache[key] = {'a': st_index_a, 'b': st_index_b, 'img': st_index_img}[which](C).to(device)
        return self.cache[key]

    def st_fused_weights(self, n, dtype):
        """Packed operands of the fused SpatialTransformer block `n` (sdmi.h: sdmi_st_block): weight streams of
        phase A / B and their fp32 epilogue vectors.  Same folds as ln_folded / ffout_proj_weights (LayerNorm
        gamma into the weights, beta into the bias; ff.net.2 and proj_out pre-multiplied).  Weight preparation,
        cached until the weights change."""
        key = ('st_fused', n, dtype)
        if key not in self.cache:
            with torch.no_grad():
                t = n + '.transformer_blocks.0'
                f = lambda k: self.t[k].float()
                C = f(n + '.proj_in.bias').numel()
                dev = self.t[n + '.proj_in.bias'].device
                w_in = f(n + '.proj_in.weight').reshape(C, C)
                g1, b1 = f(t + '.norm1.weight'), f(t + '.norm1.bias')
                wqkv = torch.cat([f(t + '.attn1.to_q.weight'), f(t + '.attn1.to_k.weight'), f(t + '.attn1.to_v.weight')])
                wqkv_p = (wqkv * g1).to(dtype)
                src_a = torch.cat([w_in.to(dtype).reshape(-1), wqkv_p.reshape(-1)])
                vec_a = torch.cat([f(n + '.proj_in.bias'), wqkv_p.float().sum(1), wqkv @ b1]).contiguous()
                wa = src_a[self.st_index('a', C, dev)].contiguous()
                wo, bo = f(t + '.attn1.to_out.0.weight'), f(t + '.attn1.to_out.0.bias')
                bo2 = f(t + '.attn2.to_out.0.bias')
                g3, b3 = f(t + '.norm3.weight'), f(t + '.norm3.bias')
                w1, bb1 = f(t + '.ff.net.0.proj.weight'), f(t + '.ff.net.0.proj.bias')
                w1_p = (w1 * g3).to(dtype)
                wff, bff = f(t + '.ff.net.2.weight'), f(t + '.ff.net.2.bias')
                wpo, bpo = f(n + '.proj_out.weight').reshape(C, C), f(n + '.proj_out.bias')
                src_b = torch.cat([wo.to(dtype).reshape(-1), wpo.to(dtype).reshape(-1), w1_p.reshape(-1),
                                   (wpo @ wff).to(dtype).reshape(-1)])
                wbs = src_b[self.st_index('b', C, dev)].contiguous()
                vec_b = torch.cat([bo, bo2, w1_p.float().sum(1), w1 @ b3 + bb1, wpo @ bff + bpo]).contiguous()
                self.cache[key] = dict(wa=wa, va=vec_a, wb=wbs, vb=vec_b, C=C)
        return self.cache[key]

    def rollout_weights(self, l, dtype):
        """Packed operands of the fused rollout layer `l` (sdmi.h: sdmi_rollout_layer): the unit streams of phase A / B
        and their fp32 epilogue vectors, LayerNorm gamma folded into the weights and beta into the biases as in
        ln_folded.  Weight preparation, cached until the weights change."""
        key = ('rollout', l, dtype)
        if key not in self.cache:
            with torch.no_grad():
                f = lambda k: self.t[l + k].float()
                wqkv, bqkv = f('.self_attn.in_proj_weight'), f('.self_attn.in_proj_bias')
                C = wqkv.shape[1]
                dev = wqkv.device
                g1, b1 = f('.norm1.weight'), f('.norm1.bias')
                wqkv_p = (wqkv * g1).to(dtype)
                ia = self.cache.get(('rollout_index', 'a', C))
                if ia is None:
                    ia = self.cache[('rollout_index', 'a', C)] = rollout_index_a(C).to(dev)
                wa = wqkv_p.reshape(-1)[ia].contiguous()
                va = torch.cat([wqkv_p.float().sum(1), wqkv @ b1 + bqkv]).contiguous()
                wo, bo = f('.self_attn.out_proj.weight'), f('.self_attn.out_proj.bias')
                g2, b2 = f('.norm2.weight'), f('.norm2.bias')
                w1, bb1, w2, bb2 = f('.linear1.weight'), f('.linear1.bias'), f('.linear2.weight'), f('.linear2.bias')
                F = w1.shape[0]
                w1_p = (w1 * g2).to(dtype)
                ib = self.cache.get(('rollout_index', 'b', C, F))
                if ib is None:
                    ib = self.cache[('rollout_index', 'b', C, F)] = rollout_index_b(C, F).to(dev)
                src_b = torch.cat([wo.to(dtype).reshape(-1), w1_p.reshape(-1), w2.to(dtype).reshape(-1)])
                vb = torch.cat([bo, w1_p.float().sum(1), w1 @ b2 + bb1, bb2]).contiguous()
                self.cache[key] = dict(wa=wa, va=va, wb=src_b[ib].contiguous(), vb=vb, C=C, F=F)
        return self.cache[key]

    def rollout_feed_weights(self, name):
        """Packed operands of sdmi_rollout_feed for the rollouter `name` (rollout_feed_pack) from the master weights,
        rounded to bf16 as the shadow arena rounds them.  Weight preparation, cached until the weights change."""
        key = ('rollout_feed', name)
        if key not in self.cache:
            with torch.no_grad():
                ip, op = f'{name}.in_proj', f'{name}.out_proj'
                self.cache[key] = rollout_feed_pack(self.t[op + '.weight'], self.t[op + '.bias'],
                                                    self.t[ip + '.weight'], self.t[ip + '.bias'])
        return self.cache[key]

    def readout_weights(self, dtype, name='linear1.weight'):
        """linear1.weight [F, 2C] of the Physion readout as the packed operand of sdmi_readout_fwd / _bwd (sdmi.h) in
        `dtype`: one gather out of the master (fp32) / shadow (bf16) arena.  Cached until the weights change."""
        key = ('readout', name, dtype)
        if key not in self.cache:
            with torch.no_grad():
                F, C2 = self.t[name].shape
                src = self._flat(name, dtype)
                idx = readout_pack_index(C2 // 2, F, dtype, src.device)
                self.cache[key] = src.reshape(-1)[idx].contiguous()
        return self.cache[key]

    def pred_step_weights(self, base, wrap):
        """Packed operands of the fused slot transition (pred_pack) from the master weights, rounded to bf16 as the
        shadow arena rounds them.  Weight preparation, cached until the weights change."""
        key = ('pred_step', base, wrap)
        if key not in self.cache:
            with torch.no_grad():
                self.cache[key] = pred_pack(self.t, base, wrap)
        return self.cache[key]

    def pred_tf_weights(self, base, layers):
        """Packed operands of the fused transformer transition (pred_tf_pack) from the master weights, rounded to bf16
        as the shadow arena rounds them.  Weight preparation, cached until the weights change."""
        key = ('pred_tf', base, layers)
        if key not in self.cache:
            with torch.no_grad():
                self.cache[key] = pred_tf_pack(self.t, base, layers)
        return self.cache[key]

    # ---- weight streams of the fused SpatialTransformer TRAINING kernels (sdmi.h: sdmi_st_train_fwd, sdmi_st_pack)
    def st_train_mats(self, n):
        """{key: (bf16 operand view [N][K], K)} of block `n` straight out of the shadow arena."""
        t = n + '.transformer_blocks.0'
        names = {'in': n + '.proj_in.weight', 'q': t + '.attn1.to_q.weight', 'k': t + '.attn1.to_k.weight',
                 'v': t + '.attn1.to_v.weight', 'o': t + '.attn1.to_out.0.weight', 'q2': t + '.attn2.to_q.weight',
                 'o2': t + '.attn2.to_out.0.weight', 'ff1': t + '.ff.net.0.proj.weight', 'ff2': t + '.ff.net.2.weight',
                 'po': n + '.proj_out.weight'}
        out = {}
        for k, nm in names.items():
            v = self._flat(nm, torch.bfloat16)
            assert v is not None and v.is_contiguous()
            out[k] = v
        return out

    ST_STREAMS = ('a', 'b', 'b1', 'b2', 'ba')

    def st_train_streams(self, n):
        """dict(wa, wb, wb1, wb2, wba, C) -- bf16 unit streams of block `n` for sdmi_st_train_fwd / _bwd.  The streams live
        in persistent buffers; after an optimiser step (invalidate()) the first request re-packs the streams of ALL
        registered blocks with one sdmi_st_pack launch (descriptor table on the device: part of the captured train step)."""
        m = self.st_streams.get(n)
        if m is None:
            mats = self.st_train_mats(n)
            C = mats['in'].shape[0]
            dev = mats['in'].device
            units = st_train_units(C)
            count = {k: sum(len(w) for w in units[k]) for k in self.ST_STREAMS}
            st = {'w' + k: torch.empty((count[k] * 1024,), dtype=torch.bfloat16, device=dev) for k in self.ST_STREAMS}
            descs = np.zeros(sum(count.values()), dtype=self.st_streams.desc)
            o = 0
            for k in self.ST_STREAMS:
                st_pack_descs(descs[o:o + count[k]], units[k], mats, st['w' + k])
                o += count[k]
            m = self.st_streams.add(n, SimpleNamespace(streams=dict(st, C=C), descs=descs), dev, rows=len(descs))
        return m.streams

    @staticmethod
    def _st_fill(m, rows, blk):
        rows[:] = m.descs
        return blk

    @staticmethod
    def _st_launch(_, tab):
        call('sdmi_st_pack', _st(), descs=_p(tab.dev), n_units=tab.rows)

    def b(self, names):
        """fp32 bias vector, fused across names (view when adjacent)."""
        if names is None:
            return None
        if isinstance(names, str):
            return self.t[names]
        key = ('bias', names)
        if key in self.cache:
            return self.cache[key]
        parts = [self.t[n] for n in names]
        out = torch.empty((sum(p.numel() for p in parts),), dtype=torch.float32,
                          device=parts[0].device)
        if all(p.dtype == torch.float32 and p.is_contiguous() for p in parts):
            o, items = 0, []
            for p in parts:
                items.append((_p(p), _p(out[o:]), p.numel() * 4))
                o += p.numel()
            _copy_group(items)
            self.cache[key] = out
            return out
        o = 0
        for p in parts:
            ops.cast2d(p.view(-1, 1), torch.float32, out=out[o:o + p.numel()].view(-1, 1))
            o += p.numel()
        self.cache[key] = out
        return out

    def wd(self, names, dtype, kh, kw, cin_x):
        """dgrad operand of the (fused) forward operand: [Cin][kh'][kw'][CoutPad], taps flipped.

        The operands live in persistent buffers; after an optimiser step (invalidate()) the first
        request re-packs ALL of them with one sdmi_pack_dgrad_batch launch (descriptor table on
        the device) instead of one small launch per layer.  Operands whose forward operand is a
        materialised copy (no fixed arena address) are packed individually."""
        return self._dgrad(('dgrad', names if not isinstance(names, str) else (names,), dtype), names, dtype, kh, kw, cin_x)

    def wd_sub(self, names, dtype, kh, kw, cin_x, kh0, kw0, step):
        """Parity sub-filter of the dgrad operand (taps kh0::step, kw0::step of the flipped filter,
        [Cin][nkh][nkw][CoutPad]) for the data gradient of a strided convolution; kept and re-packed
        with the other dgrad operands (one sdmi_pack_dgrad_batch launch per optimiser step)."""
        names = names if not isinstance(names, str) else (names,)
        sub = (kh0, kw0, step, len(range(kh0, kh, step)), len(range(kw0, kw, step)))
        return self._dgrad(('dgradsub', names, dtype, kh0, kw0, step), names, dtype, kh, kw, cin_x, sub)

    def ups_train_ok(self, x, wnames, geom, plain):
        """An upsample convolution trained in the 4x4 stride-2 transposed form (GemmFn) -- the sampler's gate
        (Kern.conv), on operands that come straight out of the shadow arena; `plain`: no rowvec / residual / out_dtype /
        ldc.  The fp8 configuration keeps its layers as they are."""
        kh, kw, stride, pad, ups = geom
        if not (_UPS_TRAIN and ups and plain and isinstance(wnames, str) and (kh, kw, stride) == (3, 3, 1)
                and tuple(pad) == (1, 1, 1, 1) and x.dim() == 4 and x.dtype == torch.bfloat16 and x.shape[-1] % 64 == 0
                and not getattr(self.model, 'fp8_unet', False)):
            return False
        p = self.t[wnames]
        return p.dim() == 4 and p.shape[1] == x.shape[-1] and p.shape[0] % 8 == 0 and _grads_of(self, wnames) is not None

    def ups_fwd(self, wname, dtype):
        """Forward operand [4][Cout][2*2*Cin] of an upsample convolution in the transposed form (sdmi.h:
        SDMI_PACK_UPS_FWD; ops.conv2d's parity4).  A member of the dgrad-operand table like `ups_wd`: both are re-made
        from the shadow weights by the step's one sdmi_pack_dgrad_batch launch."""
        co, ci = self.t[wname].shape[:2]
        sub = (0, 0, _lib.ENUMS['SDMI_PACK_UPS_FWD'], 4, 4)
        return self._dgrad(('upsfwd', (wname,), dtype), (wname,), dtype, 3, 3, ci, sub).view(4, co, 4 * ci)

    def ups_wd(self, wname, dtype):
        """... and its data-gradient operand [Cin][4*4*Cout] (SDMI_PACK_UPS_DGRAD): the weight of the 4x4 stride-2
        pad-1 convolution dY -> dx."""
        sub = (0, 0, _lib.ENUMS['SDMI_PACK_UPS_DGRAD'], 4, 4)
        return self._dgrad(('upswd', (wname,), dtype), (wname,), dtype, 3, 3, self.t[wname].shape[1], sub)

    def _dgrad(self, key, names, dtype, kh, kw, cin_x, sub=None):
        m = self.dgrad_ops.get(key)
        if m is not None:
            return m.dst
        w = self.w(names, dtype)
        n = w.shape[0]
        vec = ops.vec_of(dtype)
        npad = (n + vec - 1) // vec * vec
        taps = kh * kw if sub is None else sub[3] * sub[4]
        old = self.dgrad_ops.members.get(key)       # (an operand outside the table comes back every epoch: same buffer)
        dst = old.dst if old is not None else \
            (torch.zeros if npad != n else torch.empty)((cin_x * taps, npad), dtype=dtype, device=w.device)
        stable = self._in_arena(w)
        m = self.dgrad_ops.add(key, SimpleNamespace(dst=dst, src=w, Cout=n, KH=kh, KW=kw, Cin=cin_x, CoutPad=npad, sub=sub),
                               w.device, group=dtype, tabled=stable)
        if not stable:
            m.src = None                            # a materialised copy: made again, not kept
        return dst

    @staticmethod
    def _dgrad_fill(m, rows, blk):
        derived.put(rows, 0, src=m.src.data_ptr(), dst=m.dst.data_ptr(), Cout=m.Cout, KH=m.KH, KW=m.KW, Cin=m.Cin,
                    CoutPad=m.CoutPad, block_begin=blk)
        taps = m.KH * m.KW
        if m.sub is not None:                       # parity sub-filter: selected taps only
            kh0, kw0, kstep, nkh, nkw = m.sub
            derived.put(rows, 0, kh0=kh0, kw0=kw0, kstep=kstep, nkh=nkh, nkw=nkw)
            taps = nkh * nkw
        return blk + taps * ((m.Cout + 63) // 64) * ((m.Cin + 63) // 64)

    @staticmethod
    def _dgrad_launch(dtype, tab):
        call('sdmi_pack_dgrad_batch', _st(), descs=_p(tab.dev), n_desc=tab.rows, dtype=_DT[dtype], total_blocks=tab.blocks)

    def _dgrad_first(self, m, one):
        if m.sub is None:                           # the plain launch takes no table: legal inside a graph capture
            call('sdmi_pack_dgrad', _st(), src=_p(m.src), dst=_p(m.dst), dtype=_DT[m.group], Cout=m.Cout, KH=m.KH,
                 KW=m.KW, Cin=m.Cin, CoutPad=m.CoutPad)
        else:                                       # (eager only: a one-entry table)
            self._dgrad_launch(m.group, one())

    def _in_arena(self, t):
        m = self.model
        for a in (m.arena(), m.shadow_arena() if m.compute_dtype != torch.float32 else None):
            if a is not None and a.data_ptr() <= t.data_ptr() < a.data_ptr() + a.numel() * a.element_size():
                return True
        return False


class Kern:
    """Inference provider."""
    training = False

    def __init__(self, wb):
        self.wb = wb

    def conv(self, x, wname, bname=None, *, kh=3, kw=3, stride=1, pad=(1, 1, 1, 1), ups=False,
             rowvec=None, residual=None, out_dtype=None, ldc=None, zero_pad=True):
        if isinstance(x, CatPair):
            if kh == 1 and kw == 1 and stride == 1 and not ups:
                return ops.conv2d(x.a, self.wb.w(wname, x.dtype), self.wb.b(bname), kh=1, kw=1, pad=pad,
                                  rowvec=rowvec, residual=residual, out_dtype=out_dtype, ldc=ldc, x2=x.b)
            x = x.materialize()
        if ups and _UPS_PARITY and kh == 3 and kw == 3 and stride == 1 and pad == (1, 1, 1, 1) and \
                x.dtype == torch.bfloat16 and x.shape[-1] % 64 == 0 and rowvec is None and residual is None and \
                out_dtype is None and ldc is None:
            # nearest-2x upsample + 3x3 convolution = four 2x2 convolutions of the low-resolution input, one per
            # output parity, written interleaved (WeightBank.ups_parity_weights): 2.25x fewer multiply-adds
            B, H, W_, _ = x.shape
            ws = self.wb.ups_parity_weights(wname, x.dtype)
            out = torch.empty((B, 2 * H, 2 * W_, ws[0, 0].shape[0]), dtype=x.dtype, device=x.device)
            bias = self.wb.b(bname)
            # all four parities in one launch (sdmi.h: parity4; the filters are one [4][N][4 Cin] tensor)
            w4 = next(iter(ws.values()))._base
            return ops.conv2d(x, w4, bias, kh=2, kw=2, out=out, parity4=True)
        if x.dtype == torch.uint8 or self.fp8_ok(x, wname, kh * kw, ups):
            # BASELINE "fp8 MFMA UNet": e4m3fn operands (activations at a fixed scale -- written by
            # the GroupNorm in front when there is one -- weights at 448 / amax), fp32 accumulation,
            # the scales undone in the epilogue's alpha
            w8, inv = self.wb.w8(wname)
            x8 = x if x.dtype == torch.uint8 else ops.quant_fp8(x, FP8_ACT_SCALE)
            return ops.conv2d(x8, w8, self.wb.b(bname), kh=kh, kw=kw,
                              stride=stride, pad=pad, rowvec=rowvec, residual=residual,
                              out_dtype=out_dtype or self.wb.dtype, ldc=ldc, alpha=inv / FP8_ACT_SCALE)
        return ops.conv2d(x, self.wb.w(wname, x.dtype), self.wb.b(bname), kh=kh, kw=kw,
                          stride=stride, pad=pad, ups=ups, rowvec=rowvec, residual=residual,
                          out_dtype=out_dtype, ldc=ldc, zero_pad=zero_pad)

    def fp8_ok(self, x, wname, taps, ups):
        """fp8 operands for the UNet's 3x3 convolutions (bf16 storage path, >= 64 input channels in
        16-byte rows); everything else -- 1x1 / linear layers, attention, the 3 / 4-channel
        in / out convolutions, the VQ-VAE and the slot encoder -- stays bf16."""
        return (getattr(self.wb.model, 'fp8_unet', False) and x.dtype == torch.bfloat16 and taps > 1
                and not ups and x.shape[-1] % 16 == 0 and x.shape[-1] >= 64
                and wname.startswith(self.wb.model.fp8_prefix))

    def linear(self, x, wnames, bnames=None, *, act=None, residual=None, out_dtype=None):
        return ops.linear(x, self.wb.w(wnames, x.dtype), self.wb.b(bnames), act=act,
                          residual=residual, out_dtype=out_dtype)

    def gn(self, x, name, *, eps, act=None, residual=None, dropout=None, for_conv=None, rowsum_of=None):
        if isinstance(x, CatPair):
            f8 = FP8_ACT_SCALE if (for_conv and self.fp8_ok(x, for_conv, 9, False)) else None
            return ops.group_norm(x.a, self.wb.f(name + '.weight'), self.wb.f(name + '.bias'), eps=eps,
                                  act=act, residual=residual, fp8_scale=f8, x2=x.b)
        return self._gn(x, name, eps=eps, act=act, residual=residual, dropout=dropout, for_conv=for_conv)

    def _gn(self, x, name, *, eps, act=None, residual=None, dropout=None, for_conv=None):
        """dropout = site name: training-mode dropout behind the activation (no-op at inference).
        for_conv = weight name of the 3x3 convolution that is the output's only reader: in the fp8
        configuration the norm writes that convolution's e4m3fn operand directly."""
        f8 = FP8_ACT_SCALE if (for_conv and self.fp8_ok(x, for_conv, 9, False)) else None
        return ops.group_norm(x, self.wb.f(name + '.weight'), self.wb.f(name + '.bias'), eps=eps,
                              act=act, residual=residual, fp8_scale=f8)

    def linear_multi(self, x, wname_list):
        """Several bias-free projections of one input -> tuple of outputs."""
        return tuple(self.linear(x, n) for n in wname_list)

    # fan-out forms: (result, alias(es) of x for x's other consumers) -- plain x at inference
    def gn_fan(self, x, name, *, eps, act=None, residual=None, n_alias=1, for_conv=None):
        return (self.gn(x, name, eps=eps, act=act, residual=residual, for_conv=for_conv),) + (x,) * n_alias

    def ln_fan(self, x, name):
        return self.ln(x, name), x

    def ln_linear_fan(self, x, ln_name, wnames, bnames=None, *, act=None, geglu=False, eps=1e-5):
        """linear(LayerNorm(x)) (-> GEGLU) in ONE launch at inference: the norm is folded into the
        GEMM (sdmi.h: ln_colsum), the gated activation into its epilogue.  -> (out, x for the
        residual branch).  bf16 (throughput) path only: the fp32 path keeps the reference's kernel
        sequence for the parity tests.  SDMI_LN_FOLD=0: the unfused sequence everywhere."""
        # (the folded GEMM costs ~1.45x a plain one on 128 x 128 tiles but saves a dependent launch per site: it wins end
        # to end at every size -- 94.75 vs 95.6 / 95.8 ms per sampling pass, round 3)
        if not _LN_FOLD or x.dtype != torch.bfloat16:
            h = self.linear(self.ln(x, ln_name, eps), wnames, bnames, act=act)
            return (self.geglu(h) if geglu else h), x
        w, colsum, bias = self.wb.ln_folded(ln_name, wnames, bnames, x.dtype)
        return ops.linear(x, w, bias, act=act, ln_colsum=colsum, ln_eps=eps, geglu=geglu), x

    def conv_fan(self, x, wname, bname=None, **kw):
        return self.conv(x, wname, bname, **kw), x

    def linear_fan(self, x, wnames, bnames=None):
        return self.linear(x, wnames, bnames), x

    def deconv(self, x, wname, bname, *, k, stride, pad, act='relu'):
        return deconv_forward(self.wb, x, wname, bname, k, stride, pad, act)

    def broadcast_pos(self, x, pos, dtype):
        return BroadcastPosFn.forward(None, x, pos, dtype)

    def sa_combine(self, o, B, N):
        BN, H, W_, ld = o.shape
        recon = torch.empty((B, H, W_, 4), dtype=torch.float32, device=o.device)
        masks = torch.empty((B, N, H * W_), dtype=torch.float32, device=o.device)
        call('sdmi_sa_combine', _st(), o=_p(o), recon=_p(recon), masks=_p(masks), dtype=_DT[o.dtype],
             B=B, N=N, HW=H * W_, ldo=ld)
        return recon, masks

    def ln(self, x, name, eps=1e-5):
        return ops.layer_norm(x, self.wb.f(name + '.weight'), self.wb.f(name + '.bias'), eps=eps)

    def attn_self(self, qkv, heads, head_dim=32):
        C = heads * head_dim
        fits = ops.ATTN_MFMA_MAX_KV if (qkv.dtype == torch.bfloat16 and head_dim == 32) else ops.ATTN_LDS_MAX_KV
        if qkv.shape[1] > fits:          # e.g. the 785 tokens x head_dim 64 of the DINO ViT
            return ops.attention_long(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, head_dim)
        return ops.attention(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads,
                             head_dim=head_dim)

    def attn_cross(self, q, kv, heads):
        C = heads * 32
        return ops.attention(q, kv[..., :C], kv[..., C:], heads)

    def res_tail(self, h, n, skip):
        """out = out_layers.3(h) + (skip_connection(skip) if the block changes its channel count else skip).
        bf16 inference: the 3x3 convolution and the 1x1 skip convolution are ONE implicit GEMM over
        [im2col(h) | skip] (or [im2col(h) | a | b] for a skip that is a lazy concat)."""
        has_skip = (n + '.skip_connection.weight') in self.wb.t
        if has_skip and _RES_MERGE and torch.is_tensor(h) and h.dtype == torch.bfloat16 and h.shape[-1] % 64 == 0:
            srcs = (skip.a, skip.b) if isinstance(skip, CatPair) else (skip,)
            if all(t.shape[-1] % 64 == 0 and t.dtype == h.dtype for t in srcs):
                w, b = self.wb.conv_skip_weights(n, h.dtype)
                return ops.conv2d(h, w, b, kh=3, kw=3, pad=(1, 1, 1, 1), x2=srcs[0],
                                  x3=(srcs[1] if len(srcs) > 1 else None))
        if has_skip:
            skip = self.conv(skip, n + '.skip_connection.weight', n + '.skip_connection.bias', kh=1, kw=1,
                             pad=(0, 0, 0, 0))
        elif hasattr(skip, 'materialize'):             # (a lazy concat that keeps its channel count)
            skip = skip.materialize()
        return self.conv(h, n + '.out_layers.3.weight', n + '.out_layers.3.bias', residual=skip)

    def ff_out_proj(self, g, tres, xres, t, n):
        """ff.net.2 (+ token residual) followed by proj_out (+ block residual): ONE GEMM over the two
        sources [g | tres] with pre-multiplied weights at bf16 inference, the two launches otherwise."""
        if _FF_MERGE and g.dtype == torch.bfloat16 and g.shape[-1] % 64 == 0 and tres.shape[-1] % 64 == 0:
            w, b = self.wb.ffout_proj_weights(t, n, g.dtype)
            B, HW, C = tres.shape
            out = ops.conv2d(g.view(B, HW, 1, g.shape[-1]), w, b, kh=1, kw=1, pad=(0, 0, 0, 0),
                             residual=xres.view(B, HW, 1, C), x2=tres.view(B, HW, 1, C))
            return out.view(B, HW, C)
        tok = self.linear(g, t + '.ff.net.2.weight', t + '.ff.net.2.bias', residual=tres)
        return self.linear(tok, n + '.proj_out.weight', n + '.proj_out.bias', residual=xres)

    def cross_prepare(self, kv, t, heads):
        """Once per sampling call (slots and weights are fixed over the NFEs): the slot keys (7 of the image models in
        8-row groups per head; the video models' 11 / 15 in 16-row groups, savi_diffusion.py:143-144) folded
        into the query projection, the values into the output projection -- per image
          Wq[b] = (scale K_b restricted per head) (W_q gamma)   [heads*8, C]   (+ LayerNorm-fold terms)
          W2[b] = W_o (V_b restricted per head)^T               [C, heads*8]
        so that slot cross-attention is two small per-image GEMMs per evaluation (cross_block)."""
        if not (_CROSS_FOLD and kv.dtype == torch.bfloat16 and kv.shape[1] <= _CROSS_MAX_SLOTS):
            return None
        wt, tb, ones = self.wb.cross_fold_weights(t, kv.dtype)
        B, C = kv.shape[0], kv.shape[-1] // 2
        gw = 8 if kv.shape[1] <= 8 else 16             # score columns per head (softmax group width)
        R = heads * gw
        kexp, vexp = ops.expand_heads(kv, heads, float(C // heads) ** -0.5, gw)
        # (the fused block pads the score matrix to 128 columns: 16-row groups fit C = 256 -- 8 heads -- only)
        fused = _ST_FUSED and C in (256, 384) and R <= 128
        if fused:
            # the fused block (sdmi_st_block) takes the same operands padded to 128 score columns, as a unit
            # stream: Wq[b] / W2[b] are produced straight into the padded storage (pads stay zero)
            # (allocated per call: the fold dict hands out VIEWS of these -- a cached buffer would be overwritten by the
            # next context of the same batch size (cond / uncond, two live generators) while an earlier fold is alive)
            src = torch.zeros((B, 128 * C + C * 128), dtype=kv.dtype, device=kv.device)
            vec = torch.zeros((B, 256), dtype=torch.float32, device=kv.device)
            wq = src[:, :R * C].view(B, R, C)
            w2 = src[:, 128 * C:].view(B, C, 128)[:, :, :R]
            colsum, biasq = vec[:, :R].unsqueeze(-1), vec[:, 128:128 + R].unsqueeze(-1)
        else:
            wq = torch.empty((B, R, C), dtype=kv.dtype, device=kv.device)
            w2 = torch.empty((B, C, R), dtype=kv.dtype, device=kv.device)
            colsum = torch.empty((B, R, 1), dtype=torch.float32, device=kv.device)
            biasq = torch.empty((B, R, 1), dtype=torch.float32, device=kv.device)
        ops.bmm_nt(kexp, wt, wq)
        ops.bmm_nt(wq, ones, colsum)
        ops.bmm_nt(kexp, tb, biasq)
        wo = self.wb.w(t + '.attn2.to_out.0.weight', kv.dtype)
        ops.bmm_nt(wo.view(1, C, C).expand(B, -1, -1), vexp, w2)
        fold = dict(wq=wq, colsum=colsum.squeeze(-1), biasq=biasq.squeeze(-1), w2=w2, slots=kv.shape[1])
        if fused:
            fold['st_img'] = ops.gather_rows(src, self.wb.st_index('img', C, kv.device))
            fold['st_vec'] = vec
        return fold

    def cross_block(self, tok, t, kvp, heads):
        """norm2 -> slot cross-attention -> to_out + residual of transformer block `t` -> new tok."""
        fold = kvp.get('fold') if isinstance(kvp, dict) else None
        if fold is not None:
            B, HW, C = tok.shape
            # few tokens per image (the 4^2 / 8^2 levels): the layer is a per-image weight stream -- one launch, one
            # workgroup per 16 tokens (sdmi_cross_fold) instead of two batched GEMMs on mostly empty 64 x 64 tiles
            if _CROSS_ONE and HW % 16 == 0 and HW <= _CROSS_ONE and tok.is_contiguous() and fold['slots'] <= 8 and \
                    (C, fold['wq'].shape[1]) in ops.CROSS_FOLD_SHAPES:
                if 'cf_wq' not in fold:          # once per sampling call: the operands in MFMA-fragment order
                    R = fold['wq'].shape[1]
                    iq = self.wb.cf_index(R, C, tok.device)
                    i2 = self.wb.cf_index(C, R, tok.device)
                    fold['cf_wq'] = ops.gather_rows(fold['wq'].reshape(B, R * C), iq)
                    fold['cf_w2'] = ops.gather_rows(fold['w2'].reshape(B, C * R), i2)
                return ops.cross_fold(tok, fold['cf_wq'], fold['colsum'], fold['biasq'], fold['cf_w2'],
                                      self.wb.b(t + '.attn2.to_out.0.bias'), 1e-5, fold['slots'], packed=True)
            P = ops.cross_scores(tok, fold['wq'], fold['colsum'], fold['biasq'], 1e-5, fold['slots'])
            return ops.bmm_nt(P, fold['w2'], torch.empty_like(tok), bias=self.wb.b(t + '.attn2.to_out.0.bias'),
                              residual=tok)
        kv = kvp['kv'] if isinstance(kvp, dict) else kvp
        q, tres = self.ln_linear_fan(tok, t + '.norm2', t + '.attn2.to_q.weight')
        a = self.attn_cross(q, kv, heads)
        return self.linear(a, t + '.attn2.to_out.0.weight', t + '.attn2.to_out.0.bias', residual=tres)

    def st_fused(self, x, n, heads, kvp):
        """The whole SpatialTransformer block `n` in two launches (sdmi.h: sdmi_st_block) -- bf16 inference,
        C = 256 / 384, 64 | tokens per image <= 256, folded slot cross-attention (<= 7 slots; C = 256: <= 16).  None when the
        block does not qualify (the caller runs the per-layer launches)."""
        fold = kvp.get('fold') if isinstance(kvp, dict) else None
        B, H, W, C = x.shape
        S = H * W
        if not (_ST_FUSED and fold is not None and 'st_img' in fold and x.dtype == torch.bfloat16 and
                C in (256, 384) and heads * 32 == C and S % 64 == 0 and S <= 256 and x.is_contiguous()):
            return None
        rows = _ST_ROWS or (64 if B * S // 64 >= 192 else 32)
        if B * S // rows < _ST_MIN_WGS:
            return None
        wts = self.wb.st_fused_weights(n, x.dtype)
        tok = torch.empty((B, S, C), dtype=x.dtype, device=x.device)
        qkv = torch.empty((B, S, 3 * C), dtype=x.dtype, device=x.device)
        out = torch.empty_like(x)
        # algorithmic work of the block (bench.py's roofline legs): its GEMMs + the two attention contractions
        g = st_geometry(C)
        flops = 2.0 * B * S * (C * C * 4 + C * C + 2 * 128 * C + 8 * C * C + 5 * C * C) + 4.0 * B * S * S * C
        wbytes = 2.0 * (wts['wa'].numel() + wts['wb'].numel()) + 2.0 * fold['st_img'].numel()
        # a grid that leaves half the chip idle (64 images at 8^2: 128 workgroups of 32 rows): the feed-forward of phase B
        # split over workgroup PAIRS, each streaming half of the hidden chunks; the pair's fp32 partials are summed (+ bias
        # + x) by the kernel behind like a split-K convolution's second stage (ops.defer_splitk: the next GroupNorm's
        # prologue, or sdmi_splitk_finish in front of any other reader)
        split = 2 if (_ST_FF_SPLIT and ops._DEFER[0] and B * S // rows <= 128) else 1
        part = torch.empty((2 * B * S * C,), dtype=torch.float32, device=x.device) if split == 2 else None
        call('sdmi_st_block', _st(), x=_p(x), tok=_p(tok), qkv=_p(qkv), out=_p(out),
             gn_gamma=_p(self.wb.f(n + '.norm.weight')), gn_beta=_p(self.wb.f(n + '.norm.bias')),
             wstream_a=_p(wts['wa']), vec_a=_p(wts['va']), wstream_b=_p(wts['wb']), vec_b=_p(wts['vb']),
             wstream_img=_p(fold['st_img']), vec_img=_p(fold['st_vec']), B=B, S=S, C=C, slots=fold['slots'],
             phase=0, gn_eps=1e-6, ln_eps=1e-5, attn_scale=32.0 ** -0.5, rows=rows, part=_p(part), ff_split=split,
             _meta=dict(flops=flops, bytes=2.0 * B * S * C * 2 + wbytes))
        if split == 2:
            bias = wts['vb'][18 * C:19 * C]
            kw = dict(out=_p(out), workspace=_p(part), bias=_p(bias), residual=_p(x), ldr=C, dtype=_lib.BF16,
                      out_dtype=_lib.BF16, M=B * S, N=C, ldc=C, B=B, H=H, W=W, Ho=H, Wo=W, alpha=1.0, act=0, batch=1)
            ops._PENDING[out.data_ptr()] = ops._PendingSplit(out, kw, 2, (part, bias, None, x, 1.0))
        return out

    def rollout_layer(self, x, l, L, heads):
        """One pre-LN encoder layer `l` of the SlotFormer rollouter in two launches (sdmi.h: sdmi_rollout_layer) -- bf16
        inference, x [B, Lp, 256] with L real tokens per sequence in Lp rows (a multiple of 64, <= 256), 8 heads of 32,
        ffn_dim a multiple of 128 up to 1024.  None when the layer does not qualify (the caller runs the per-layer
        launches)."""
        B, Lp, C = x.shape
        w1 = self.wb.t[l + '.linear1.weight']
        F = w1.shape[0]
        if not (_ROLLOUT_FUSED and x.dtype == torch.bfloat16 and x.is_contiguous() and C == 256 and heads == 8 and
                Lp % 64 == 0 and Lp <= 256 and 1 <= L <= Lp and F % 128 == 0 and F <= 4 * C):
            return None
        wts = self.wb.rollout_weights(l, x.dtype)
        qkv = torch.empty((B, Lp, 3 * C), dtype=x.dtype, device=x.device)
        out = torch.empty_like(x)
        flops = 2.0 * B * Lp * (4 * C * C + 2 * C * F) + 4.0 * B * Lp * L * C
        call('sdmi_rollout_layer', _st(), x=_p(x), qkv=_p(qkv), out=_p(out), wstream_a=_p(wts['wa']), vec_a=_p(wts['va']),
             wstream_b=_p(wts['wb']), vec_b=_p(wts['vb']), B=B, L=L, Lp=Lp, C=C, heads=heads, ffn_dim=F, phase=0,
             ln_eps=1e-5, attn_scale=32.0 ** -0.5,
             _meta=dict(flops=flops, bytes=2.0 * B * Lp * C * 2 + 2.0 * (wts['wa'].numel() + wts['wb'].numel())))
        return out

    def rollout_feed(self, x, win, win_next, x_next, pos, pred, step, N, L, name):
        """The glue between rollout steps `step` and `step + 1` as ONE launch (sdmi.h: sdmi_rollout_feed): x [B, Lp, C]
        bf16 = the last layer's output, win the window without positions (None: the last step, only pred is written),
        pred [B, P, N, Ds] fp32 whose slice `step` is written; win_next / x_next [B, Lp, C] are filled for the next
        step.  The caller checks rollout_feed_covers."""
        B, Lp, C = x.shape
        P, Ds = pred.shape[1], pred.shape[3]
        wts = self.wb.rollout_feed_weights(name)
        assert wts['C'] == C and wts['Ds'] == Ds and pred.is_contiguous() and x.is_contiguous()
        last = win is None
        call('sdmi_rollout_feed', _st(), x=_p(x), win=_p(win), win_next=0 if last else _p(win_next),
             x_next=0 if last else _p(x_next), pos=_p(pos), pred=pred.data_ptr() + step * N * Ds * 4,
             ld_pred=P * N * Ds, wout=_p(wts['wout']), bout=_p(wts['bout']), win_w=_p(wts['win_w']), bin=_p(wts['bin']),
             B=B, N=N, L=L, Lp=Lp, C=C, Ds=Ds,
             _meta=dict(flops=4.0 * B * N * C * Ds, bytes=4.0 * C * Ds + (0.0 if last else 6.0 * B * L * C)))

    def geglu(self, h):
        return ops.geglu(h)

    def add_pos(self, x, pos):
        return ops.add_pos(x, pos)

    def shift_window(self, win, new, L):
        return shift_window(win, new, L)

    def tail_tokens(self, x, n, L):
        return tail_tokens(x, n, L)

    def stack_time(self, xs):
        return StackTimeFn.apply(*xs)

    def rowvec_slices(self, rowvecs, bounds):
        """[B, total] -> {i: rowvecs[:, off:off+c]} (strided views; the kernels take the row pitch)."""
        return [rowvecs[:, off:off + c] for off, c in bounds]

    def concat(self, a, b):
        """Channel concatenation for the UNet's skip connections.  At inference the two readers of the
        result -- the ResBlock's first GroupNorm and its 1x1 skip convolution -- take the two tensors
        in place (CatPair: sdmi.h x2 / a2), so nothing is materialised."""
        if _LAZY_CAT and a.dim() == 4 and a.shape[-1] % 64 == 0 and b.shape[-1] % 64 == 0:
            return CatPair(a, b)
        return ops.concat_channels(a, b)

    def cast(self, x, dtype):
        return x if x.dtype == dtype else ops.act(x, None, dtype)

    def lstm_cell(self, z, c_prev):
        return ops.lstm_cell(z, c_prev)[:2]

    def pred_step(self, x, base, wrap, norm_first, state):
        """The whole slot transition as ONE sdmi_pred_step launch: x [R, D] fp32, `base` = key prefix of the MLP
        predictor or None (x is then the transformer predictor's output), `wrap` = key prefix of the LSTM wrapper or
        None, state = (h, c) | None -> (y, (h, c) | None); None when the launch does not apply (the caller runs the
        composed chain): fp32 model, geometry outside pred_step_covers."""
        W = self.wb.t
        H = W[wrap + '.rnn.weight_hh_l0'].shape[1] if wrap else 0
        if not (_PRED_FUSED and self.wb.dtype == torch.bfloat16 and x.dtype == torch.float32 and
                pred_step_covers(x.shape[-1], H)):
            return None
        mode = (ops.PRED_MLP if base else 0) | (ops.PRED_RNN if wrap else 0)
        h, c = state if state is not None else (None, None)
        y, h, c = ops.pred_step(x, self.wb.pred_step_weights(base, wrap), mode, norm_first, h, c)
        return y, ((h, c) if wrap else None)

    def pred_tf(self, x, base, layers, heads):
        """The transformer slot transition as ONE sdmi_pred_tf launch: x [B, N, D] fp32, `base` = key prefix of the
        TransformerPredictor -> [B, N, D] fp32; None when the launch does not apply (the caller runs
        engine.transformer_predictor): fp32 model, geometry outside pred_tf_covers."""
        B, N, D = x.shape
        F = self.wb.t[f'{base}.transformer_encoder.layers.0.linear1.weight'].shape[0]
        if not (self.wb.dtype == torch.bfloat16 and x.dtype == torch.float32 and pred_tf_covers(N, D, heads, F, layers)):
            return None
        return ops.pred_tf(x.contiguous(), self.wb.pred_tf_weights(base, layers), heads)

    def cast_pad(self, x, dtype, cols, ldd):
        """First `cols` channels of x [..., ld] -> dtype [..., ldd] (zero padded)."""
        return ops.cast2d(x, dtype, cols=cols, ldd=ldd)

    def dropout(self, x, site='unet'):
        return x

    def linear_drop_res(self, x, wname, bname, res):
        """res + dropout(linear(x)); without dropout the residual add is the GEMM epilogue."""
        return self.linear(x, wname, bname, residual=res)

    def slot_attention(self, kv, init, name, iters, eps):
        wb = self.wb
        D = kv.shape[-1] // 2
        P = dict(lnq_g=wb.f(f'{name}.project_q.0.weight'), lnq_b=wb.f(f'{name}.project_q.0.bias'),
                 wq=wb.f(f'{name}.project_q.1.weight'), w_ih=wb.f(f'{name}.gru.weight_ih'),
                 w_hh=wb.f(f'{name}.gru.weight_hh'), b_ih=wb.f(f'{name}.gru.bias_ih'),
                 b_hh=wb.f(f'{name}.gru.bias_hh'), lnm_g=wb.f(f'{name}.mlp.0.weight'),
                 lnm_b=wb.f(f'{name}.mlp.0.bias'), w1=wb.f(f'{name}.mlp.1.weight'),
                 b1=wb.f(f'{name}.mlp.1.bias'), w2=wb.f(f'{name}.mlp.3.weight'),
                 b2=wb.f(f'{name}.mlp.3.bias'))
        return ops.slot_attention(kv[..., :D], kv[..., D:], init, P, iters=iters, eps=eps)


# ==========================================================================================
# training provider: autograd Functions with libsdmi backward kernels
# ==========================================================================================
def _grads_of(wb, names):
    """Contiguous gradient-arena destination for (fused) params, or None if not adjacent."""
    m = wb.model
    g = m.grad_arena()
    if isinstance(names, str):
        names = (names,)
    offs = [m._offsets[n] for n in names]
    for i in range(len(offs) - 1):
        if offs[i][0] + offs[i][1] != offs[i + 1][0]:
            return None
    return g[offs[0][0]:offs[-1][0] + offs[-1][1]]


class _RowvecSink:
    """Gradient matrix [B, total] shared by the column slices RowvecSplitFn hands out: every consumer
    writes its slice (rowgroup_sum with an output pitch); allocated at the first write of a backward."""

    def __init__(self, B, total):
        self.B, self.total, self.buf = B, total, None
        self.filled = set()        # offsets whose slice a GroupNorm backward has written already

    def buffer(self, device):
        if self.buf is None:
            self.buf = torch.empty((self.B, self.total), dtype=torch.float32, device=device)
        return self.buf


class RowvecSplitFn(torch.autograd.Function):
    """rowvecs [B, total] -> its column slices (one per ResBlock: the time-embedding rows).  Plain
    slicing costs three framework kernels per slice in backward (zeros, copy, accumulate): here the
    consumers' backward kernels write straight into one shared gradient matrix, which this backward
    just returns.  The slices must tile [0, total) and each be consumed exactly once."""

    @staticmethod
    def forward(ctx, rowvecs, bounds):
        B, total = rowvecs.shape
        assert bounds[0][0] == 0 and bounds[-1][0] + bounds[-1][1] == total
        sink = _RowvecSink(B, total)
        ctx.sink = sink
        outs = []
        for off, c in bounds:
            v = rowvecs[:, off:off + c]
            outs.append(v)
        ctx.set_materialize_grads(False)
        ctx.n = len(bounds)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        sink = ctx.sink
        assert sink.buf is not None and all(g is not None for g in grads), 'every slice needs its consumer'
        buf, sink.buf = sink.buf, None
        sink.filled.clear()
        return buf, None


_CUS = {}


def _n_cus(device):
    """Compute units of `device` (cached)."""
    key = str(device)
    if key not in _CUS:
        _CUS[key] = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return _CUS[key]


class GemmFn(torch.autograd.Function):
    """out = conv/linear(x, W) + bias (+ rowvec[b]) (+ residual).  Activation-free."""

    @staticmethod
    def forward(ctx, x, rowvec, residual, anchor, wb, wnames, bnames, geom, out_dtype, ldc, n_alias=0):
        """n_alias = 1: also returns an alias of x for x's OTHER consumer (identity / skip branch);
        its gradient comes back into this backward and is summed inside the dgrad kernel's epilogue
        instead of by an autograd accumulation kernel."""
        kh, kw, stride, pad, ups = geom
        w = wb.w(wnames, x.dtype)
        b = wb.b(bnames)
        x8 = getattr(x, '_sdmi_fp8', None)           # e4m3fn copy written by the GroupNorm in front (KernGrad.gn)
        ctx.ups4 = wb.ups_train_ok(x, wnames, geom, rowvec is None and residual is None and out_dtype is None
                                   and ldc is None)
        if ctx.ups4:
            # nearest-2x upsample + 3x3 convolution = ConvTranspose2d(4, stride 2, padding 1) of the low-resolution input
            # with the composite filter (sdmi.h: SDMI_PACK_UPS_*): four 2x2 parity convolutions in one launch here, a
            # strided convolution of dY and a folded 4x4 weight gradient in backward -- 16 multiply-adds per output pixel
            # and input channel instead of 36, all three ways
            out = torch.empty((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], w.shape[0]), dtype=x.dtype, device=x.device)
            ops.conv2d(x, wb.ups_fwd(wnames, x.dtype), b, kh=2, kw=2, out=out, parity4=True)
        elif x8 is not None and x8.shape == x.shape and wb.fp8_train_ok(x, wnames, geom):
            # e4m3fn operands in the forward GEMM: activations at the fixed scale of the inference path -- only where a
            # GroupNorm (+ SiLU) bounds them and wrote the operand itself: the stride-2 downsample convolutions read
            # the raw residual stream and keep bf16 in training -- weights at 448 / amax with amax taken on the device
            # this step (WeightBank.w8_dev); fp32 accumulation, both scales undone in the epilogue.  x stays bf16 for
            # the backward pass.
            w8, inv = wb.w8_dev(wnames)
            out = ops.conv2d(x8, w8, b, kh=kh, kw=kw, stride=stride, pad=pad,
                             rowvec=rowvec, residual=residual, out_dtype=out_dtype or x.dtype, ldc=ldc,
                             alpha=1.0 / FP8_ACT_SCALE, alpha_dev=inv)
        elif x.dim() == 4 and (kh, kw) != (0, 0):
            out = ops.conv2d(x, w, b, kh=kh, kw=kw, stride=stride, pad=pad, ups=ups, rowvec=rowvec,
                             residual=residual, out_dtype=out_dtype, ldc=ldc)
        else:
            out = ops.linear(x, w, b, residual=residual, out_dtype=out_dtype)
        ctx.save_for_backward(x)
        ctx.cfg = (wb, wnames, bnames, geom, rowvec is not None, residual is not None,
                   rowvec.shape if rowvec is not None else None)
        ctx.rv_sink = getattr(rowvec, '_sdmi_sink', None)      # (RowvecSplitFn: shared gradient matrix)
        ctx.set_materialize_grads(False)
        if n_alias:
            return out, x.view_as(x)
        return out

    @staticmethod
    def backward(ctx, dy, dalias=None):
        (x,) = ctx.saved_tensors
        if dalias is not None:
            dalias = dalias.contiguous()
        wb, wnames, bnames, geom, has_rv, has_res, rv_shape = ctx.cfg
        dx, dy, (N, ldy, B, Ho, Wo, dt) = GemmFn.core(wb, x, dy, wnames, bnames, geom,
                                                       ctx.needs_input_grad[0], dalias, ctx.ups4)
        drv = None
        if has_rv and ctx.needs_input_grad[1]:
            if ctx.rv_sink is not None:        # a column slice of the shared [B, total] gradient matrix
                sink, off = ctx.rv_sink
                drv = sink.buffer(x.device)[:, off:off + N]
                if off not in sink.filled:     # (else: the GroupNorm behind this conv summed its dx already)
                    call('sdmi_rowgroup_sum', _st(), x=_p(dy), out=_p(drv), dtype=_DT[dt], groups=B,
                         rows_per=Ho * Wo, N=N, ldx=ldy, ldo=drv.stride(0))
            else:
                drv = torch.empty(rv_shape, dtype=torch.float32, device=x.device)
                call('sdmi_rowgroup_sum', _st(), x=_p(dy), out=_p(drv), dtype=_DT[dt], groups=B,
                     rows_per=Ho * Wo, N=N, ldx=ldy)
        dres = None
        if has_res and ctx.needs_input_grad[2]:
            dres = dy if dy.shape[-1] == N else None
            assert dres is not None
        _dbg(f'gemm {wnames if isinstance(wnames, str) else wnames[0]}', dy=dy, dx=dx, drv=drv)
        return dx, drv, dres, None, None, None, None, None, None, None, None

    @staticmethod
    def core(wb, x, dy, wnames, bnames, geom, need_dx, dalias=None, ups4=False):
        """Weight / bias gradient and data gradient of one conv / linear: build the problem, plan (bwd.plan_layer),
        execute the plan.  -> (dx or None, dy in the compute dtype, (N, ldy, B, Ho, Wo, dt)).  ups4: the forward ran in
        the transposed form (WeightBank.ups_train_ok)."""
        dt = x.dtype
        vec = ops.vec_of(dt)
        N = wb.w(wnames, dt).shape[0]
        dy = dy.contiguous()
        # bring dY to the compute dtype with a vector-multiple row pitch
        if dy.dtype != dt or dy.shape[-1] % vec:
            npad = (N + vec - 1) // vec * vec
            dy = ops.cast2d(dy, dt, cols=N, ldd=npad)
        if ups4:
            return GemmFn._ups4(wb, x, dy, wnames, bnames, N, need_dx, dalias)
        P = bwd.LayerProblem.of(x, dy, geom, dt, N)
        info = (N, P.ldy, P.B, P.Ho, P.Wo, dt)
        # weight / bias gradients go straight into the gradient arena where it has the kernel's [N][K] layout
        names = (wnames,) if isinstance(wnames, str) else tuple(wnames)
        dst = _grads_of(wb, names)
        bdst = _grads_of(wb, bnames) if bnames is not None else None
        direct = dst is not None and wb.t[names[0]].numel() // wb.t[names[0]].shape[0] == P.K
        plan = bwd.plan_layer(P, need_dx=need_dx, direct=direct, has_bias=bnames is not None, bias_dst=bdst is not None,
                              dalias_cols=(dalias.shape[-1] if dalias is not None else None), n_cus=_n_cus(x.device),
                              pair_bwd=wb.pair_bwd, wgrad_halo=_WGRAD_HALO)
        if plan.path == 'pair':
            wd = wb.wd(wnames, dt, P.kh, P.kw, P.Cin)
            dx = torch.empty(x.shape if not P.is_conv else (P.B, P.H, P.W, P.Cin), dtype=dt, device=x.device)
            wb.sched.launch_pair(
                P, plan.pair,
                dict(P.dgrad_fields(), a=_p(dy), w=_p(wd), out=_p(dx), split_k=1, residual=_p(dalias)),
                dict(P.wgrad_fields(), a=_p(x), dy=_p(dy), dw=_p(dst), dbias=_p(bdst), accumulate=1), x.device)
            return dx, dy, info
        wb.sched.side_wgrad(names[0], (_p(dst), _p(bdst)),
                            lambda: GemmFn._wgrad(wb, x, dy, P, plan, names, bnames, dst, direct), (x, dy))
        # ---- data gradient: the forward kernel on the flipped operand
        dx = None
        if need_dx:
            wd = wb.wd(wnames, dt, P.kh, P.kw, P.Cin)
            if P.is_conv and P.stride > 1 and not P.ups:
                dx, dalias = GemmFn._dgrad_strided(
                    dy, wd, P.B, P.H, P.W, P.Ho, P.Wo, P.Cin, P.ldy, P.kh, P.kw, P.stride, P.pad, dt, dalias,
                    sub_of=lambda a0, b0: wb.wd_sub(wnames, dt, P.kh, P.kw, P.Cin, a0, b0, P.stride))
            elif P.is_conv:
                f = P.dgrad_fields()
                out = torch.empty((P.B, f['Ho'], f['Wo'], P.Cin), dtype=dt, device=x.device)
                ws = None if P.stride > 1 else ops.splitk_workspace(f['M'], P.Cin, f['K'], dy.element_size(), x.device)
                fuse = dalias is not None and not P.ups
                call('sdmi_igemm', _st(), a=_p(dy), w=_p(wd), out=_p(out), workspace=_p(ws),
                     split_k=(0 if ws is not None else 1), residual=(_p(dalias) if fuse else 0), **f)
                if fuse:
                    dalias = None
                if P.ups:
                    dx = torch.empty_like(x)
                    call('sdmi_pool2x2_sum', _st(), x=_p(out), y=_p(dx), dtype=_DT[dt], B=P.B, H=P.H, W=P.W, C=P.Cin)
                else:
                    dx = out
            else:
                dx = ops.linear(dy.view(-1, P.ldy), wd,
                                residual=(dalias.view(-1, P.Cin) if dalias is not None else None)).view(x.shape)
                dalias = None
            if dalias is not None:          # (no epilogue to fold it into: nearest-x2 / partial parity cover)
                call('sdmi_add', _st(), x=_p(dx), z=_p(dalias), y=_p(dx), dtype=_DT[dt], n=dx.numel())
        elif dalias is not None:
            dx = dalias
        return dx, dy, info

    @staticmethod
    def _dgrad_strided(dy, wd, B, H, W_, Ho, Wo, Cin, ldy, kh, kw, s, pad, dt, extra=None, sub_of=None):
        """Data gradient of a stride-s convolution by input-pixel parity (bwd.LayerProblem.parity_dgrads)."""
        full, subs = bwd.LayerProblem.conv(B, H, W_, Ho, Wo, Cin, ldy, ldy, kh, kw, s, pad, dt).parity_dgrads()
        w4 = wd.view(Cin, kh, kw, ldy)
        dx = torch.empty((B, H, W_, Cin), dtype=dt, device=dy.device)
        if not full:
            ops.zero_(dx)
        # `extra` (gradient of x's other consumer) rides in the epilogue when every pixel is written
        fuse = extra is not None and full
        for a0, b0, f in subs:
            sub = sub_of(a0, b0) if sub_of is not None else w4[:, a0::s, b0::s, :].contiguous()
            call('sdmi_igemm', _st(), a=_p(dy), w=_p(sub), out=_p(dx), split_k=1, residual=(_p(extra) if fuse else 0), **f)
        return dx, (None if fuse else extra)

    @staticmethod
    def _ups4(wb, x, dy, wname, bname, N, need_dx, dalias):
        """Backward of an upsample convolution in the transposed form (bwd.LayerProblem.upsampled).  Main stream: dx =
        the 4x4 stride-2 pad-1 convolution of dY with the composite operand, the gradient of x's other consumer in its
        epilogue.  Side stream, two launches: dW4 [Cin][4][4][Cout] by sdmi_wgrad with the roles of x and dY swapped (its
        M-split partials left in the workspace), then sdmi_ups_fold_dw, which folds them into the arena's
        [Cout][3][3][Cin] and, with extra workgroups, writes the bias-gradient partials that the join folds with the
        step's other column sums."""
        dt = x.dtype
        P = bwd.LayerProblem.upsampled(x, N)
        dst = _grads_of(wb, wname)
        bias = {}
        if bname is not None:
            rows = P.B * P.H * P.W
            chunk = next((c for c in (256, 128, 64) if rows % c == 0), rows)
            part = torch.empty((rows // chunk, N), dtype=torch.float32, device=x.device)
            bias = dict(dy=_p(dy), bias_part=_p(part), dtype=_DT[dt], rows=rows, rows_per=chunk)
        done = []

        def wgrad():
            splits = bwd.standalone_splits(P)
            ws = torch.empty((splits * (P.N * P.K + P.N),), dtype=torch.float32, device=x.device)
            call('sdmi_wgrad', _st(), a=_p(dy), dy=_p(x), dw=_p(ws), dbias=0, workspace=_p(ws), splits=splits,
                 accumulate=0, defer_fold=1, **P.wgrad_fields())
            call('sdmi_ups_fold_dw', _st(), dw4=_p(ws), dw=_p(dst), Cin=P.N, Cout=P.Cin, accumulate=1, splits=splits,
                 **bias)
            done.append(torch.cuda.Event())
            done[0].record()
        wb.sched.side_wgrad(wname, (_p(dst), 0), wgrad, (x, dy))
        if bias:
            wb.queue_colsum(part, rows // chunk, N, _grads_of(wb, bname), None, after=done[0])
        dx = dalias
        if need_dx:
            dx = ops.conv2d(dy, wb.ups_wd(wname, dt), None, kh=4, kw=4, stride=2, pad=(1, 1, 1, 1), residual=dalias)
        return dx, dy, (N, N, P.B, P.H, P.W, dt)

    @staticmethod
    def _wgrad(wb, x, dy, P, plan, names, bnames, dst, direct):
        """The stand-alone weight / bias gradient launches of problem P (on whatever stream is current)."""
        N, K, Cin = P.N, P.K, P.Cin
        ws = torch.empty((plan.splits * (N * K + N),), dtype=torch.float32, device=x.device)
        # (temporaries of non-direct destinations are overwritten by the kernel, then added to the arena)
        acc = 1 if direct else 0
        dwbuf = dst if direct else torch.empty((N, K), dtype=torch.float32, device=x.device)
        btmp, stage_bias = None, False
        if bnames is not None:
            bdst = _grads_of(wb, bnames)
            if direct and bdst is not None:
                btmp = bdst
            else:
                stage_bias = True
                btmp = torch.empty((N,), dtype=torch.float32, device=x.device)
                if acc:
                    ops.zero_(btmp)
        call('sdmi_wgrad', _st(), a=_p(x), dy=_p(dy), dw=_p(dwbuf), dbias=_p(btmp), workspace=_p(ws), splits=plan.splits,
             accumulate=acc, **P.wgrad_fields())
        # non-direct destinations (channel-padded Cin, non-adjacent fused parameters) ACCUMULATE like
        # the direct path does: a parameter used several times per step (per-frame modules,
        # gradient accumulation over micro-batches) keeps every contribution
        if not direct:
            g = wb.model.grad_arena()
            taps = P.kh * P.kw
            o, segs, keep = 0, [], []
            for nme in names:
                off, cnt = wb.model._offsets[nme]
                rows = wb.t[nme].shape[0]
                ci_true = cnt // (rows * taps)
                src = dwbuf[o:o + rows]
                if ci_true != Cin:                     # channel-padded Cin: [rows*taps, Cin(pad)] -> true Cin
                    src = ops.cast2d(src.reshape(rows * taps, Cin), torch.float32, cols=ci_true, ldd=ci_true)
                    keep.append(src)
                segs.append((_p(src), _p(g[off:]), cnt))
                o += rows
            _scatter_add(segs)
        if stage_bias:
            g = wb.model.grad_arena()
            o, segs = 0, []
            for nme in (bnames if not isinstance(bnames, str) else (bnames,)):
                off, cnt = wb.model._offsets[nme]
                segs.append((_p(btmp[o:]), _p(g[off:]), cnt))
                o += cnt
            _scatter_add(segs)


class MultiLinearFn(torch.autograd.Function):
    """outs[i] = x @ W_i^T for several (fused) weights sharing ONE input -- the UNet's 16
    cross-attention K/V projections of the slot context (attention.py:187-189).  The data gradients
    are chained through the GEMM epilogue (dx_i = dy_i W_i + dx_{i-1}), so the shared input
    receives one tensor instead of 16 autograd accumulations."""

    @staticmethod
    def forward(ctx, x, anchor, wb, wname_list):
        ctx.save_for_backward(x)
        ctx.cfg = (wb, wname_list)
        ctx.set_materialize_grads(False)
        return tuple(ops.linear(x, wb.w(n, x.dtype)) for n in wname_list)

    @staticmethod
    def backward(ctx, *dys):
        (x,) = ctx.saved_tensors
        wb, wname_list = ctx.cfg
        geom = (0, 0, 1, (0, 0, 0, 0), False)
        dx = None
        for n, dy in zip(wname_list, dys):
            if dy is None:
                continue
            d, _, _ = GemmFn.core(wb, x, dy, n, None, geom, ctx.needs_input_grad[0], dx)
            dx = d if d is not None else dx
        return dx, None, None, None


class GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, anchor, wb, name, eps, act, n_alias=0, drop=None, rsink=None, f8=None):
        """rsink = (sink, offset): x = conv(.) + a per-image row vector whose gradient -- the pixel sums
        of this norm's dx -- goes into that slice of the shared row-vector gradient matrix (written
        by the backward kernel itself: no separate reduction launch).
        drop = (p, seed, seed_dev): dropout fused behind the activation (the mask is regenerated
        from the seed in backward).  n_alias aliases of x are returned next to y for x's other consumers (ResBlock skip,
        UNet skip-concat, SpatialTransformer residual): their gradients come back into this
        backward and are summed by the GroupNorm backward kernel (dextra0/1) -- no separate
        accumulation kernels.
        f8 = [scale]: the fp8 configuration -- the launch also writes the e4m3fn operand of the convolution behind
        the norm (appended to the list; KernGrad.gn hands it to GemmFn.forward on the output tensor)."""
        gamma, beta = wb.f(name + '.weight'), wb.f(name + '.bias')
        y, stats = ops.group_norm(x, gamma, beta, eps=eps, act=act, residual=residual,
                                  return_stats=True, drop=drop, fp8_scale=(f8[0] if f8 else None),
                                  fp8_also=(f8 if f8 else None))
        ctx.save_for_backward(x, stats, residual)
        ctx.cfg = (wb, name, act)
        ctx.drop = drop if (drop is not None and drop[0] > 0.0) else None
        ctx.rsink = rsink
        ctx.set_materialize_grads(False)
        if n_alias:
            return (y,) + tuple(x.view_as(x) for _ in range(n_alias))
        return y

    @staticmethod
    def backward(ctx, dy, *dal):
        x, stats, residual = ctx.saved_tensors
        wb, name, act = ctx.cfg
        extras = [d.contiguous() for d in dal if d is not None]
        assert len(extras) <= 2 and all(e.dtype == x.dtype for e in extras)
        if dy is None:                     # y unused: only the aliases carry gradient
            dx = extras[0]
            for e in extras[1:]:
                dx = AddFn.apply(dx, e)
            return dx, None, None, None, None, None, None, None, None, None, None
        dy = dy.contiguous()
        B, C = x.shape[0], x.shape[-1]
        HW = x.numel() // (B * C)
        G = 32
        nsplit = max(1, min(16, HW // 64))
        partial = torch.empty((B * nsplit * C * 2 + B * G * 2,), dtype=torch.float32,
                              device=x.device)
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if residual is not None else None
        dg = _grads_of(wb, name + '.weight')
        db = _grads_of(wb, name + '.bias')
        geo = dict(dtype=_DT[x.dtype], B=B, HW=HW, C=C, groups=G, nsplit=nsplit)
        defer = wb.defer_colsum
        if defer:          # the dbeta / dgamma folds of the whole step run in a few grouped launches
            wb.queue_colsum(partial, _lib.query('sdmi_groupnorm_bwd_entries', **geo), C, db, dg)
        rs_kw, rs_view = {}, None
        if ctx.rsink is not None and not extras:
            sink, off = ctx.rsink
            rs_view = sink.buffer(x.device)[:, off:off + C]
            if _lib.query('sdmi_groupnorm_bwd_fused', **geo):
                rs_kw = dict(dxsum=_p(rs_view), ld_dxsum=rs_view.stride(0))
        call('sdmi_groupnorm_bwd', _st(), x=_p(x), dy=_p(dy), dx=_p(dx), gamma=_p(wb.f(name + '.weight')),
             beta=_p(wb.f(name + '.bias')), stats=_p(stats), dgamma=_p(dg), dbeta=_p(db),
             partial=_p(partial), defer_colsum=int(defer), **geo, **rs_kw,
             act=_lib.ACT[act], residual=_p(residual), dresidual=_p(dres), accumulate=1,
             dextra0=(_p(extras[0]) if extras else 0), dextra1=(_p(extras[1]) if len(extras) > 1 else 0),
             **(dict(drop_p=float(ctx.drop[0]), drop_seed=int(ctx.drop[1]), drop_seed_dev=_p(ctx.drop[2]))
                if ctx.drop else {}))
        if rs_view is not None:
            if not rs_kw:              # two-pass geometry: the sums take their own launch after all
                call('sdmi_rowgroup_sum', _st(), x=_p(dx), out=_p(rs_view), dtype=_DT[dx.dtype], groups=B,
                     rows_per=HW, N=C, ldx=C, ldo=rs_view.stride(0))
            ctx.rsink[0].filled.add(ctx.rsink[1])
        _dbg(f'gn {name}', dy=dy, dx=dx, dres=dres)
        return dx, dres, None, None, None, None, None, None, None, None, None


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, wb, name, n_alias=0):
        C = x.shape[-1]
        stats = torch.empty((x.numel() // C, 2), dtype=torch.float32, device=x.device)
        y = ops.layer_norm(x, wb.f(name + '.weight'), wb.f(name + '.bias'), stats=stats)
        ctx.save_for_backward(x, stats)
        ctx.cfg = (wb, name)
        ctx.set_materialize_grads(False)
        if n_alias:                        # alias of x for the residual branch (see GroupNormFn)
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dalias=None):
        x, stats = ctx.saved_tensors
        wb, name = ctx.cfg
        if dalias is not None:
            dalias = dalias.contiguous()
        if dy is None:
            return dalias, None, None, None, None
        return LayerNormFn.bwd_core(wb, name, x, stats, dy.contiguous(), dalias), None, None, None, None

    @staticmethod
    def bwd_core(wb, name, x, stats, dy, dalias=None):
        """dx of y = LayerNorm(x) (+ dalias: the gradient of x's other consumer, summed in the kernel); dgamma / dbeta
        into the gradient arena (deferred column sums)."""
        C = x.shape[-1]
        rows = x.numel() // C
        nblk = max(1, min(512, rows // 16))
        partial = torch.empty((nblk * C * 2,), dtype=torch.float32, device=x.device)
        dx = torch.empty_like(x)
        dg, db = _grads_of(wb, name + '.weight'), _grads_of(wb, name + '.bias')
        defer = wb.defer_colsum
        if defer:
            wb.queue_colsum(partial, nblk, C, dg, db)
        call('sdmi_layernorm_bwd', _st(), x=_p(x), dy=_p(dy), dx=_p(dx),
             gamma=_p(wb.f(name + '.weight')), stats=_p(stats), dgamma=_p(dg), dbeta=_p(db),
             partial=_p(partial), dtype=_DT[x.dtype], rows=rows, C=C, nblk=nblk, accumulate=1,
             dextra=_p(dalias), defer_colsum=int(defer))
        _dbg(f'ln {name}', dy=dy, dx=dx)
        return dx


class AttnFn(torch.autograd.Function):
    """self: qkv fused [B,S,3C]; cross: q [B,S,C] + kv [B,N,2C]."""

    @staticmethod
    def forward(ctx, q_or_qkv, kv, heads, head_dim=32):
        C = heads * head_dim
        if kv is None:
            q, k, v = q_or_qkv[..., :C], q_or_qkv[..., C:2 * C], q_or_qkv[..., 2 * C:]
        else:
            q, k, v = q_or_qkv, kv[..., :C], kv[..., C:]
        B, Sq = q.shape[0], q.shape[1]
        lse = torch.empty((B, heads, Sq), dtype=torch.float32, device=q.device)
        out = ops.attention(q, k, v, heads, lse=lse, head_dim=head_dim)
        ctx.save_for_backward(q_or_qkv, kv, out, lse)
        ctx.heads, ctx.hd = heads, head_dim
        return out

    @staticmethod
    def backward(ctx, dout):
        a, kv, out, lse = ctx.saved_tensors
        da, dkv = AttnFn.bwd_core(a, kv, out, lse, dout.contiguous(), ctx.heads, ctx.hd)
        return da, dkv, None, None

    @staticmethod
    def bwd_core(a, kv, out, lse, dout, heads, hd=32):
        """(d q|k|v, None) of self-attention over the fused a = q|k|v, or (dq, d k|v) of cross-attention."""
        C = heads * hd
        da = torch.empty_like(a)
        dkv = torch.empty_like(kv) if kv is not None else None
        if kv is None:
            q, k, v = a[..., :C], a[..., C:2 * C], a[..., 2 * C:]
            dq, dk, dv = da[..., :C], da[..., C:2 * C], da[..., 2 * C:]
        else:
            q, k, v = a, kv[..., :C], kv[..., C:]
            dq, dk, dv = da, dkv[..., :C], dkv[..., C:]
        B, Sq, Skv = q.shape[0], q.shape[1], k.shape[1]
        call('sdmi_attention_bwd', _st(), q=_p(q), k=_p(k), v=_p(v), out=_p(out), dout=_p(dout),
             lse=_p(lse), dq=_p(dq), dk=_p(dk), dv=_p(dv), dtype=_DT[q.dtype], B=B, heads=heads,
             Sq=Sq, Skv=Skv, ldq=q.stride(1), ldk=k.stride(1), ldv=v.stride(1), ldo=out.stride(1),
             scale=hd ** -0.5, head_dim=hd)
        _dbg(f'attn Sq={Sq} Skv={Skv}', dout=dout, da=da, dkv=dkv)
        return da, dkv


class LongAttnFn(torch.autograd.Function):
    """Self-attention over sequences beyond the LDS-resident kernels (ops.attention_long) with its
    backward as batched GEMMs per head:  dP = dO v^T,  dv = P^T dO,  dS = softmax'(P, dP),
    dq = dS k,  dk = dS^T q  (the score / probability matrices live in HBM).  qkv [B,S,3C]."""

    @staticmethod
    def forward(ctx, qkv, heads, head_dim):
        C = heads * head_dim
        assert qkv.shape[1] % ops.vec_of(qkv.dtype) == 0, 'sequence length must keep 16-byte rows'
        out, P = ops.attention_long(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, head_dim,
                                    keep_p=True)
        ctx.save_for_backward(qkv, P)
        ctx.heads, ctx.hd = heads, head_dim
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, P = ctx.saved_tensors
        heads, hd = ctx.heads, ctx.hd
        C = heads * hd
        B, S, _ = qkv.shape
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dp = torch.empty((B, S, S), dtype=qkv.dtype, device=qkv.device)
        for h in range(heads):
            q, k, v = (qkv[..., j * C + h * hd:j * C + (h + 1) * hd] for j in range(3))
            dq, dk, dv = (dqkv[..., j * C + h * hd:j * C + (h + 1) * hd] for j in range(3))
            do = dout[..., h * hd:(h + 1) * hd]
            p = P[h]
            ops.bmm_nt(do, v, dp)                                            # dP = dO v^T
            ops.bmm_nt(ops.transpose2d(p), ops.transpose2d(do), dv)          # dv = P^T dO
            ops.softmax_rows_bwd_(p, dp, scale=float(hd) ** -0.5)            # dp <- dS
            ops.bmm_nt(dp, ops.transpose2d(k), dq)                           # dq = dS k
            ops.bmm_nt(ops.transpose2d(dp), ops.transpose2d(q), dk)          # dk = dS^T q
        return dqkv, None, None


class GegluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h):
        ctx.save_for_backward(h)
        return ops.geglu(h)

    @staticmethod
    def backward(ctx, dy):
        (h,) = ctx.saved_tensors
        dy = dy.contiguous()
        dh = torch.empty_like(h)
        C = h.shape[-1] // 2
        call('sdmi_geglu_bwd', _st(), h=_p(h), dy=_p(dy), dh=_p(dh), dtype=_DT[h.dtype],
             rows=h.numel() // (2 * C), C=C)
        return dh


class GegluLinearFn(torch.autograd.Function):
    """y = GEGLU(x W^T + b) as ONE GEMM launch whose epilogue stores the pre-activation h as well
    (sdmi.h: geglu + out2); backward = geglu_bwd on the kept h, then the linear layer's gradients."""

    @staticmethod
    def forward(ctx, x, anchor, wb, wname, bname):
        w = wb.w(wname, x.dtype)
        h = torch.empty(x.shape[:-1] + (w.shape[0],), dtype=x.dtype, device=x.device)
        y = ops.linear(x, w, wb.b(bname), geglu=True, out2=h)
        ctx.save_for_backward(x, h)
        ctx.cfg = (wb, wname, bname)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, h = ctx.saved_tensors
        wb, wname, bname = ctx.cfg
        dy = dy.contiguous()
        dh = torch.empty_like(h)
        C = h.shape[-1] // 2
        call('sdmi_geglu_bwd', _st(), h=_p(h), dy=_p(dy), dh=_p(dh), dtype=_DT[h.dtype],
             rows=h.numel() // (2 * C), C=C)
        dx = GemmFn.core(wb, x, dh, wname, bname, (0, 0, 1, (0, 0, 0, 0), False), ctx.needs_input_grad[0])[0]
        return dx, None, None, None, None


def _gn_bwd_plain(wb, name, x, stats, dy, extras=()):
    """dx of y = GroupNorm(x) (no activation / residual / dropout) + the gradients of x's other consumers."""
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    G = 32
    nsplit = max(1, min(16, HW // 64))
    partial = torch.empty((B * nsplit * C * 2 + B * G * 2,), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dg, db = _grads_of(wb, name + '.weight'), _grads_of(wb, name + '.bias')
    geo = dict(dtype=_DT[x.dtype], B=B, HW=HW, C=C, groups=G, nsplit=nsplit)
    defer = wb.defer_colsum
    if defer:
        wb.queue_colsum(partial, _lib.query('sdmi_groupnorm_bwd_entries', **geo), C, db, dg)
    call('sdmi_groupnorm_bwd', _st(), x=_p(x), dy=_p(dy), dx=_p(dx), gamma=_p(wb.f(name + '.weight')),
         beta=_p(wb.f(name + '.bias')), stats=_p(stats), dgamma=_p(dg), dbeta=_p(db), partial=_p(partial),
         defer_colsum=int(defer), **geo, act=0, residual=0, dresidual=0, accumulate=1,
         dextra0=(_p(extras[0]) if extras else 0), dextra1=(_p(extras[1]) if len(extras) > 1 else 0))
    return dx


_ST_TRAIN = bool(policy.flag('ST_TRAIN'))        # fused training form of the SpatialTransformer block
# ... when its grid has at least this many workgroups (tests set it to 0).  At B = 64 the 16^2 level has 256 workgroups of
# 64 rows, the 8^2 level 128 of 32 rows: fusing the 8^2 blocks as well LOSES 0.1 - 0.2 ms per step (half the chip streams
# the block's weights while the other half idles; 26.41 / 26.41 ms with them fused, 26.33 / 26.22 ms per-layer, same box)
_ST_TRAIN_MIN_WGS = 200
_ST_TRAIN_BWD = bool(policy.flag('ST_TRAIN_BWD'))
_ST_WGRAD_GROUP = bool(policy.flag('ST_WGRAD_GROUP'))   # the block's weight gradients as two grouped launches    # ... and its backward data path (sdmi_st_train_bwd)


class StBlockFn(torch.autograd.Function):
    """A whole SpatialTransformer block of the denoiser in training (attention.py:297-308, 247-251, 182-206, 44-65):
    forward = TWO launches (sdmi.h: sdmi_st_train_fwd) that also store what the backward pass reads.
    x [B,H,W,C] bf16, kv [B,N,2C] bf16 (attn2.to_k | to_v of the slots) -> out [B,H,W,C]."""

    capture = None          # tests set a dict here: the backward pass leaves its intermediate gradients in it
    SAVED = ('hgn', 'gn_stats', 'tok', 'n1', 'st1', 'qkv', 'a1', 'lse1', 'x1', 'n2', 'st2', 'q2', 'a2', 'lse2', 'x2', 'n3',
             'st3', 'h', 'g', 'x3')

    @staticmethod
    def run_forward(wb, x, kv, n, heads, rows):
        """-> (out, {saved tensors}).  Plain launch (also what the tests drive)."""
        B, H, W, C = x.shape
        S = H * W
        dev, bf, f32 = x.device, torch.bfloat16, torch.float32
        e = lambda *sh: torch.empty(sh, dtype=bf, device=dev)
        f = lambda *sh: torch.empty(sh, dtype=f32, device=dev)
        sv = dict(hgn=e(B, S, C), gn_stats=f(B, 32, 2), tok=e(B, S, C), n1=e(B, S, C), st1=f(B * S, 2), qkv=e(B, S, 3 * C),
                  a1=e(B, S, C), lse1=f(B, heads, S), x1=e(B, S, C), n2=e(B, S, C), st2=f(B * S, 2), q2=e(B, S, C),
                  a2=e(B, S, C), lse2=f(B, heads, S), x2=e(B, S, C), n3=e(B, S, C), st3=f(B * S, 2), h=e(B, S, 8 * C),
                  g=e(B, S, 4 * C), x3=e(B, S, C))
        out = torch.empty_like(x)
        st = wb.st_train_streams(n)
        t = n + '.transformer_blocks.0'
        F_ = lambda k: _p(wb.f(k))
        flops = 2.0 * B * S * C * C * 20 + 4.0 * B * S * S * C + 4.0 * B * S * kv.shape[1] * C
        call('sdmi_st_train_fwd', _st(), x=_p(x), out=_p(out), **{k: _p(v) for k, v in sv.items()},
             kv2=_p(kv), ldkv=kv.stride(1), wstream_a=_p(st['wa']), wstream_b=_p(st['wb']),
             gn_gamma=F_(n + '.norm.weight'), gn_beta=F_(n + '.norm.bias'), b_in=F_(n + '.proj_in.bias'),
             ln1_g=F_(t + '.norm1.weight'), ln1_b=F_(t + '.norm1.bias'), b_o=F_(t + '.attn1.to_out.0.bias'),
             ln2_g=F_(t + '.norm2.weight'), ln2_b=F_(t + '.norm2.bias'), b_o2=F_(t + '.attn2.to_out.0.bias'),
             ln3_g=F_(t + '.norm3.weight'), ln3_b=F_(t + '.norm3.bias'), b_ff1=F_(t + '.ff.net.0.proj.bias'),
             b_ff2=F_(t + '.ff.net.2.bias'), b_po=F_(n + '.proj_out.bias'), B=B, S=S, C=C, slots=kv.shape[1], phase=0,
             rows=rows, gn_eps=1e-6, ln_eps=1e-5, attn_scale=32.0 ** -0.5,
             _meta=dict(flops=flops, bytes=2.0 * B * S * C * 23 + 2.0 * 36.5 * C * C))
        return out, sv

    @staticmethod
    def forward(ctx, x, kv, anchor, wb, n, heads, rows):
        out, sv = StBlockFn.run_forward(wb, x, kv, n, heads, rows)
        ctx.save_for_backward(x, kv, *[sv[k] for k in StBlockFn.SAVED])
        ctx.cfg = (wb, n, heads, rows)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, kv = ctx.saved_tensors[:2]
        sv = dict(zip(StBlockFn.SAVED, ctx.saved_tensors[2:]))
        wb, n, heads, rows = ctx.cfg
        if _ST_TRAIN_BWD:
            dx, dkv = StBlockFn.backward_fused(wb, n, heads, x, kv, sv, dout.contiguous(), rows)
        else:
            dx, dkv = StBlockFn.backward_layers(wb, n, heads, x, kv, sv, dout.contiguous())
        return dx, dkv, None, None, None, None, None

    @staticmethod
    def backward_fused(wb, n, heads, x, kv, sv, dout, rows):
        """The block's backward data path as three fused launches (sdmi.h: sdmi_st_train_bwd) around the two attention
        backward kernels and the GroupNorm backward; the weight / bias gradients of the eight linear layers are
        stand-alone launches on side streams as their dY tensors appear; LayerNorm dgamma / dbeta from the per-workgroup
        column sums the fused launches leave (deferred grouped fold)."""
        t = n + '.transformer_blocks.0'
        lin = (0, 0, 1, (0, 0, 0, 0), False)
        B, S, C = sv['tok'].shape
        dev = x.device
        do = dout.view(B, S, C)
        nwg = B * S // rows
        st = wb.st_train_streams(n)
        e = lambda *sh: torch.empty(sh, dtype=torch.bfloat16, device=dev)
        part = lambda: torch.empty((nwg * C * 2,), dtype=torch.float32, device=dev)
        grp = []                      # (weight-gradient problems of this block for ONE grouped launch)

        def wgrad(a, dy, wn, bn):
            names = (wn,) if isinstance(wn, str) else tuple(wn)
            dst, bdst = _grads_of(wb, names), (_grads_of(wb, bn) if bn is not None else None)
            if not _ST_WGRAD_GROUP or dst is None or (bn is not None and bdst is None):
                GemmFn.core(wb, a, dy, wn, bn, lin, False)
                return
            P = bwd.LayerProblem.of(a, dy, lin, torch.bfloat16, dy.shape[-1])
            grp.append((P, bn is not None, a, dy,
                        dict(P.wgrad_fields(), a=_p(a), dy=_p(dy), dw=_p(dst), dbias=_p(bdst), accumulate=1)))

        def flush_group():
            if not grp:
                return
            wb.sched.launch_group([g[4] for g in grp], bwd.plan_group([g[:2] for g in grp]),
                                  [t_ for g in grp for t_ in g[2:4]], dev)
            del grp[:]
        F_ = lambda k: _p(wb.f(k))
        geo = dict(B=B, S=S, C=C, rows=rows)
        rf = 2.0 * B * S * C * C
        # ---- phase B1
        dx3, dh, dx2, da2, p3 = e(B, S, C), e(B, S, 8 * C), e(B, S, C), e(B, S, C), part()
        call('sdmi_st_train_bwd', _st(), phase=1, dout=_p(do), h=_p(sv['h']), x2=_p(sv['x2']), st3=_p(sv['st3']),
             ln3_g=F_(t + '.norm3.weight'), dx3=_p(dx3), dh=_p(dh), dx2=_p(dx2), da2=_p(da2), ln3_part=_p(p3),
             wstream_b1=_p(st['wb1']), **geo, _meta=dict(flops=14.0 * rf, bytes=2.0 * B * S * C * 22 + 28.0 * C * C))
        wb.queue_colsum(p3, nwg, C, _grads_of(wb, t + '.norm3.weight'), _grads_of(wb, t + '.norm3.bias'))
        wgrad(sv['x3'], do, n + '.proj_out.weight', n + '.proj_out.bias')
        wgrad(sv['g'], dx3, t + '.ff.net.2.weight', t + '.ff.net.2.bias')
        wgrad(sv['n3'], dh, t + '.ff.net.0.proj.weight', t + '.ff.net.0.proj.bias')
        wgrad(sv['a2'], dx2, t + '.attn2.to_out.0.weight', t + '.attn2.to_out.0.bias')
        flush_group()
        dq2, dkv = AttnFn.bwd_core(sv['q2'], kv, sv['a2'], sv['lse2'], da2, heads)
        # ---- phase B2
        dx1, da1, p2 = e(B, S, C), e(B, S, C), part()
        call('sdmi_st_train_bwd', _st(), phase=2, dq2=_p(dq2), x1=_p(sv['x1']), st2=_p(sv['st2']),
             ln2_g=F_(t + '.norm2.weight'), dx2=_p(dx2), dx1=_p(dx1), da1=_p(da1), ln2_part=_p(p2),
             wstream_b2=_p(st['wb2']), **geo, _meta=dict(flops=2.0 * rf, bytes=2.0 * B * S * C * 6 + 4.0 * C * C))
        wb.queue_colsum(p2, nwg, C, _grads_of(wb, t + '.norm2.weight'), _grads_of(wb, t + '.norm2.bias'))
        wgrad(sv['n2'], dq2, t + '.attn2.to_q.weight', None)
        wgrad(sv['a1'], dx1, t + '.attn1.to_out.0.weight', t + '.attn1.to_out.0.bias')
        dqkv, _ = AttnFn.bwd_core(sv['qkv'], None, sv['a1'], sv['lse1'], da1, heads)
        # ---- phase A
        dtok, dhgn, p1 = e(B, S, C), e(B, S, C), part()
        call('sdmi_st_train_bwd', _st(), phase=3, dqkv=_p(dqkv), tok=_p(sv['tok']), st1=_p(sv['st1']),
             ln1_g=F_(t + '.norm1.weight'), dx1=_p(dx1), dtok=_p(dtok), dhgn=_p(dhgn), ln1_part=_p(p1),
             wstream_a=_p(st['wba']), **geo, _meta=dict(flops=4.0 * rf, bytes=2.0 * B * S * C * 8 + 8.0 * C * C))
        wb.queue_colsum(p1, nwg, C, _grads_of(wb, t + '.norm1.weight'), _grads_of(wb, t + '.norm1.bias'))
        wgrad(sv['n1'], dqkv, (t + '.attn1.to_q.weight', t + '.attn1.to_k.weight', t + '.attn1.to_v.weight'), None)
        wgrad(sv['hgn'], dtok, n + '.proj_in.weight', n + '.proj_in.bias')
        flush_group()
        dx = _gn_bwd_plain(wb, n + '.norm', x.view(B, S, C), sv['gn_stats'], dhgn, (do,))
        if StBlockFn.capture is not None:        # (tests: the intermediate gradients of this form)
            StBlockFn.capture.update(dx3=dx3, dh=dh, dx2=dx2, da2=da2, dq2=dq2, dx1=dx1, da1=da1, dqkv=dqkv, dtok=dtok,
                                     dhgn=dhgn)
        return dx.view_as(x), dkv

    @staticmethod
    def backward_layers(wb, n, heads, x, kv, sv, dout):
        """The block's backward pass as per-layer launches (pair launches of the linear layers, LayerNorm / attention /
        GEGLU / GroupNorm backward kernels) on the tensors the fused forward stored."""
        t = n + '.transformer_blocks.0'
        lin = (0, 0, 1, (0, 0, 0, 0), False)
        B, S, C = sv['tok'].shape
        do = dout.view(B, S, C)
        core = lambda a, dy, wn, bn, dal=None: GemmFn.core(wb, a, dy, wn, bn, lin, True, dal)[0]
        dx3 = core(sv['x3'], do, n + '.proj_out.weight', n + '.proj_out.bias')
        dg = core(sv['g'], dx3, t + '.ff.net.2.weight', t + '.ff.net.2.bias')
        h = sv['h']
        dh = torch.empty_like(h)
        call('sdmi_geglu_bwd', _st(), h=_p(h), dy=_p(dg), dh=_p(dh), dtype=_DT[h.dtype], rows=B * S, C=4 * C)
        dn3 = core(sv['n3'], dh, t + '.ff.net.0.proj.weight', t + '.ff.net.0.proj.bias')
        dx2 = LayerNormFn.bwd_core(wb, t + '.norm3', sv['x2'], sv['st3'], dn3, dx3)
        da2 = core(sv['a2'], dx2, t + '.attn2.to_out.0.weight', t + '.attn2.to_out.0.bias')
        dq2, dkv = AttnFn.bwd_core(sv['q2'], kv, sv['a2'], sv['lse2'], da2, heads)
        dn2 = core(sv['n2'], dq2, t + '.attn2.to_q.weight', None)
        dx1 = LayerNormFn.bwd_core(wb, t + '.norm2', sv['x1'], sv['st2'], dn2, dx2)
        da1 = core(sv['a1'], dx1, t + '.attn1.to_out.0.weight', t + '.attn1.to_out.0.bias')
        dqkv, _ = AttnFn.bwd_core(sv['qkv'], None, sv['a1'], sv['lse1'], da1, heads)
        dn1 = core(sv['n1'], dqkv, (t + '.attn1.to_q.weight', t + '.attn1.to_k.weight', t + '.attn1.to_v.weight'), None)
        dtok = LayerNormFn.bwd_core(wb, t + '.norm1', sv['tok'], sv['st1'], dn1, dx1)
        dhgn = core(sv['hgn'], dtok, n + '.proj_in.weight', n + '.proj_in.bias')
        dx = _gn_bwd_plain(wb, n + '.norm', x.view(B, S, C), sv['gn_stats'], dhgn, (do,))
        if StBlockFn.capture is not None:
            StBlockFn.capture.update(dx3=dx3, dh=dh, dx2=dx2, da2=da2, dq2=dq2, dx1=dx1, da1=da1, dqkv=dqkv, dtok=dtok,
                                     dhgn=dhgn)
        return dx.view_as(x), dkv


class ActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, kind):
        ctx.save_for_backward(x)
        ctx.kind = kind
        return ops.act(x, kind)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        call('sdmi_act_bwd', _st(), x=_p(x), dy=_p(dy), dx=_p(dx), dtype=_DT[x.dtype],
             act=_lib.ACT[ctx.kind], n=x.numel())
        return dx, None


class CastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return ops.act(x, None, dtype)

    @staticmethod
    def backward(ctx, dy):
        return ops.act(dy.contiguous(), None, ctx.src), None


class CastPadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype, cols, ldd):
        ctx.src, ctx.ld, ctx.cols = x.dtype, x.shape[-1], cols
        return ops.cast2d(x, dtype, cols=cols, ldd=ldd)

    @staticmethod
    def backward(ctx, dy):
        return ops.cast2d(dy.contiguous(), ctx.src, cols=ctx.cols, ldd=ctx.ld), None, None, None


class AddPosFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pos):
        ctx.pshape = pos.shape
        return ops.add_pos(x, pos)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dpos = None
        if ctx.needs_input_grad[1]:
            B = dy.shape[0]
            per = dy.numel() // B
            dpos = torch.empty(ctx.pshape, dtype=torch.float32, device=dy.device)
            call('sdmi_rowgroup_sum', _st(), x=_p(dy), out=_p(dpos), dtype=_DT[dy.dtype], groups=1,
                 rows_per=B, N=per, ldx=per)
        return dy, dpos


class ConcatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.ca, ctx.cb = a.shape[-1], b.shape[-1]
        return ops.concat_channels(a, b)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        da = torch.empty(dy.shape[:-1] + (ctx.ca,), dtype=dy.dtype, device=dy.device)
        db = torch.empty(dy.shape[:-1] + (ctx.cb,), dtype=dy.dtype, device=dy.device)
        call('sdmi_split_channels', _st(), y=_p(dy), a=_p(da), b=_p(db), dtype=_DT[dy.dtype],
             rows=dy.numel() // (ctx.ca + ctx.cb), Ca=ctx.ca, Cb=ctx.cb)
        return da, db


class SaAttendFn(torch.autograd.Function):
    """One Slot Attention iteration's streaming pass: (kv, q) -> (updates, attn)."""

    @staticmethod
    def forward(ctx, kv, q, eps, chain=False):
        """chain=True: also returns an alias of kv for the NEXT iteration; the gradient that comes
        back through it is the buffer this iteration's dk / dv are accumulated into."""
        B, M, D2 = kv.shape
        D = D2 // 2
        N = q.shape[1]
        attn = torch.empty((B, M, N), dtype=torch.float32, device=kv.device)
        upd = torch.empty((B, N, D), dtype=torch.float32, device=kv.device)
        den = torch.empty((B, N), dtype=torch.float32, device=kv.device)
        q = q.contiguous()
        ws = torch.empty((B * ((M + 63) // 64) * N * (D + 1),), dtype=torch.float32,
                         device=kv.device)
        call('sdmi_sa_attend_fwd', _st(), k=_p(kv), v=_p(kv[..., D:]), q=_p(q), attn=_p(attn),
             upd=_p(upd), den=_p(den), dtype=_DT[kv.dtype], B=B, M=M, N=N, D=D, ldkv=D2, eps=eps,
             scale=D ** -0.5, workspace=_p(ws))
        ctx.save_for_backward(kv, q, attn, upd, den)
        ctx.eps = eps
        ctx.mark_non_differentiable(attn)
        ctx.set_materialize_grads(False)
        if chain:
            return upd, attn, kv.view_as(kv)
        return upd, attn

    @staticmethod
    def backward(ctx, dupd, _dattn, dkv_next=None):
        kv, q, attn, upd, den = ctx.saved_tensors
        B, M, D2 = kv.shape
        D = D2 // 2
        N = q.shape[1]
        dupd = dupd.contiguous()
        dq = torch.empty_like(q)
        acc = dkv_next is not None and dkv_next.is_contiguous()
        dkv = dkv_next if acc else torch.empty_like(kv)
        ws = torch.empty((B * ((M + 63) // 64) * N * D,), dtype=torch.float32, device=kv.device)
        call('sdmi_sa_attend_bwd', _st(), k=_p(kv), v=_p(kv[..., D:]), q=_p(q), attn=_p(attn),
             upd=_p(upd), den=_p(den), dupd=_p(dupd), dq=_p(dq), dk=_p(dkv), dv=_p(dkv[..., D:]),
             dtype=_DT[kv.dtype], B=B, M=M, N=N, D=D, ldkv=D2, eps=ctx.eps, scale=D ** -0.5,
             workspace=_p(ws), accumulate=int(acc))
        if dkv_next is not None and not acc:
            dkv = AddFn.apply(dkv, dkv_next)
        _dbg('sa_attend', dupd=dupd, dkv=dkv, dq=dq)
        return dkv, dq, None, None


class GruGatesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gi, gh, h):
        R, D = h.shape
        out = torch.empty_like(h)
        call('sdmi_gru_gates', _st(), gi=_p(gi), gh=_p(gh), h=_p(h), hout=_p(out), R=R, D=D)
        ctx.save_for_backward(gi, gh, h)
        return out

    @staticmethod
    def backward(ctx, dout):
        gi, gh, h = ctx.saved_tensors
        R, D = h.shape
        dout = dout.contiguous()
        dgi, dgh, dh = torch.empty_like(gi), torch.empty_like(gh), torch.empty_like(h)
        call('sdmi_gru_gates_bwd', _st(), gi=_p(gi), gh=_p(gh), h=_p(h), dhout=_p(dout),
             dgi=_p(dgi), dgh=_p(dgh), dh=_p(dh), R=R, D=D)
        return dgi, dgh, dh


class LstmCellFn(torch.autograd.Function):
    """One LSTM step on gate pre-activations (sdmi_lstm_cell): (z [R, 4H], c_prev [R, H] | None) -> (h, c).  The
    backward is ONE sdmi_lstm_cell_bwd on the stored activated gates; a frame's dc_prev is the previous frame's dc."""

    @staticmethod
    def forward(ctx, z, c_prev):
        h, c, gates = ops.lstm_cell(z, c_prev, want_gates=True)
        ctx.has_prev = c_prev is not None
        ctx.save_for_backward(*((gates, c, c_prev) if ctx.has_prev else (gates, c)))
        ctx.set_materialize_grads(False)
        return h, c

    @staticmethod
    def backward(ctx, dh, dc):
        if dh is None and dc is None:
            return None, None
        gates, c = ctx.saved_tensors[:2]
        c_prev = ctx.saved_tensors[2] if ctx.has_prev else None
        dh = ops.zeros(c.shape, torch.float32, c.device) if dh is None else dh.contiguous()
        dz, dcp = ops.lstm_cell_bwd(dh, None if dc is None else dc.contiguous(), gates, c_prev, c)
        return dz, (dcp if ctx.has_prev else None)


class AddFn(torch.autograd.Function):
    """y = a + b on our add kernel (both grads are dy)."""

    @staticmethod
    def forward(ctx, a, b):
        y = torch.empty_like(a)
        call('sdmi_add', _st(), x=_p(a), z=_p(b.contiguous()), y=_p(y), dtype=_DT[a.dtype], n=a.numel())
        return y

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


class StackTimeFn(torch.autograd.Function):
    """out[:, t] = xs[t] -- torch.stack(xs, 1) of the per-frame slots / masks on the strided copy kernel (no framework
    kernel on the clip encode); backward hands every frame its slice of the gradient."""

    @staticmethod
    def forward(ctx, *xs):
        T, B = len(xs), xs[0].shape[0]
        n = xs[0].numel() // B
        out = torch.empty((B, T) + tuple(xs[0].shape[1:]), dtype=xs[0].dtype, device=xs[0].device)
        es, dt = out.element_size(), _DT[out.dtype]
        for t, x in enumerate(xs):
            x = x.contiguous()
            call('sdmi_cast2d', _st(), src=_p(x), dst=out.data_ptr() + t * n * es, src_dtype=dt, dst_dtype=dt, rows=B, cols=n,
                 lds=n, ldd=T * n, zpad=0)
        ctx.geo = (T, B, n, tuple(xs[0].shape))
        return out

    @staticmethod
    def backward(ctx, dout):
        T, B, n, shape = ctx.geo
        dout = dout.contiguous()
        es, dt = dout.element_size(), _DT[dout.dtype]
        outs = []
        for t in range(T):
            g = torch.empty(shape, dtype=dout.dtype, device=dout.device)
            call('sdmi_cast2d', _st(), src=dout.data_ptr() + t * n * es, dst=_p(g), src_dtype=dt, dst_dtype=dt, rows=B,
                 cols=n, lds=T * n, ldd=n, zpad=0)
            outs.append(g)
        return tuple(outs)


def _copy_rows(src, src_off, lds, dst, dst_off, ldd, B, cols):
    """dst[b][dst_off .. + cols] = src[b][src_off .. + cols] for b < B (element offsets / pitches; same dtype)."""
    es, dt = src.element_size(), _DT[src.dtype]
    call('sdmi_cast2d', _st(), src=src.data_ptr() + src_off * es, dst=dst.data_ptr() + dst_off * es, src_dtype=dt,
         dst_dtype=dt, rows=B, cols=cols, lds=lds, ldd=ldd, zpad=0)


def shift_window(win, new, L):
    """Sliding window of the SlotFormer rollout (slotformer.py:124): win [B, Lp, D] holds L real token rows, new
    [B, N, D] -> out rows [0, L - N) = win rows [N, L), rows [L - N, L) = new.  Rows >= L are left unwritten (pad rows
    of the fused layer's operand may hold anything)."""
    B, Lp, D = win.shape
    N = new.shape[1]
    out = torch.empty_like(win)
    if L > N:
        _copy_rows(win, N * D, Lp * D, out, 0, Lp * D, B, (L - N) * D)
    _copy_rows(new.contiguous(), 0, N * D, out, (L - N) * D, Lp * D, B, N * D)
    return out


def tail_tokens(x, n, L):
    """x [B, Lp, D] -> contiguous [B, n, D] = rows [L - n, L) (slotformer.py:120: the last N output tokens)."""
    B, Lp, D = x.shape
    out = torch.empty((B, n, D), dtype=x.dtype, device=x.device)
    _copy_rows(x, (L - n) * D, Lp * D, out, 0, n * D, B, n * D)
    return out


class ShiftWindowFn(torch.autograd.Function):
    """shift_window with its gradient: d win rows [N, L) = d out rows [0, L - N) (the dropped rows get zero),
    d new = d out rows [L - N, L)."""

    @staticmethod
    def forward(ctx, win, new, L):
        ctx.geo = (L, new.shape[1])
        return shift_window(win, new, L)

    @staticmethod
    def backward(ctx, dout):
        L, N = ctx.geo
        dout = dout.contiguous()
        B, Lp, D = dout.shape
        dwin = ops.zeros(dout.shape, dout.dtype, dout.device)
        if L > N:
            _copy_rows(dout, 0, Lp * D, dwin, N * D, Lp * D, B, (L - N) * D)
        return dwin, tail_tokens(dout, N, L), None


class TailTokensFn(torch.autograd.Function):
    """tail_tokens with its gradient (zero outside the rows taken)."""

    @staticmethod
    def forward(ctx, x, n, L):
        ctx.geo = (tuple(x.shape), n, L)
        return tail_tokens(x, n, L)

    @staticmethod
    def backward(ctx, dy):
        (B, Lp, D), n, L = ctx.geo
        dy = dy.contiguous()
        dx = ops.zeros((B, Lp, D), dy.dtype, dy.device)
        _copy_rows(dy, 0, n * D, dx, (L - n) * D, Lp * D, B, n * D)
        return dx, None, None


READOUT_NAMES = ('linear1.weight', 'linear1.bias', 'linear2.weight', 'linear2.bias')


def readout_fwd(wb, slots, agg, label=None, loss_weight=1.0, names=READOUT_NAMES):
    """sdmi_readout_fwd on the bank's weights: slots [B, T, N, C] fp32 / bf16 -> dict(frame_logits [B, T], logits [B],
    t_star [B] int32, loss [1] | None, dlogit [B] | None).  Operands in the bank's dtype."""
    w1p = wb.readout_weights(wb.dtype, names[0])
    f = lambda n: wb.t[n].detach()
    return ops.readout_fwd(slots, w1p, f(names[1]), f(names[2]).reshape(-1), f(names[3]), agg, wb.dtype, label=label,
                           loss_weight=loss_weight)


class ReadoutFn(torch.autograd.Function):
    """PhysionReadout.forward (+ the BCE loss when `label` is given) as sdmi_readout_fwd, its backward as ONE
    sdmi_readout_bwd that adds the four parameter gradients into the gradient arena.  -> (logits [B], frame_logits
    [B, T], loss scalar | None).  Gradient may arrive through the loss (the fused dlogit, scaled on the device by
    d loss) and / or through logits.  Slots are data (readout.py:56-79): no gradient reaches them."""

    @staticmethod
    def forward(ctx, slots, label, anchor, wb, agg, loss_weight=1.0, names=READOUT_NAMES):
        assert not slots.requires_grad, 'PhysionReadout takes slots as data: no gradient flows to them'
        r = readout_fwd(wb, slots, agg, label, loss_weight, names)
        ctx.save_for_backward(slots, r['t_star'], r['dlogit'])
        ctx.cfg = (wb, agg, names)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(r['frame_logits'])
        return r['logits'], r['frame_logits'], (None if r['loss'] is None else r['loss'].reshape(()))

    @staticmethod
    def backward(ctx, dlogits, _dframes, dloss):
        slots, t_star, dlogit = ctx.saved_tensors
        wb, agg, names = ctx.cfg
        gscale = None
        if dloss is not None and dlogits is None:
            d, gscale = dlogit, dloss.reshape(1).float().contiguous()
        elif dloss is not None:
            d = (dlogit * dloss.float() + dlogits.float()).contiguous()
        elif dlogits is not None:
            d = dlogits.float().contiguous()
        else:
            return (None,) * 7
        dst = [_grads_of(wb, n) for n in names]
        w1p = wb.readout_weights(wb.dtype, names[0])
        ops.readout_bwd(slots, w1p, wb.t[names[1]].detach(), wb.t[names[2]].detach().reshape(-1), t_star, d, agg,
                        wb.dtype, gscale=gscale, out=dst, accumulate=True)
        return (None,) * 7


class BceLogitsFn(torch.autograd.Function):
    """loss_weight * binary_cross_entropy_with_logits(logits [B], label [B]) through the finisher launch of
    sdmi_readout_fwd alone (phase 2 on the logits as a one-frame table): for logits that did not come with a loss."""

    @staticmethod
    def forward(ctx, logits, label, loss_weight=1.0):
        r = ops.readout_finish(logits.detach().float().reshape(-1, 1).contiguous(), label, loss_weight)
        ctx.save_for_backward(r['dlogit'])
        return r['loss'].reshape(())

    @staticmethod
    def backward(ctx, g):
        (dlogit,) = ctx.saved_tensors
        out = torch.empty_like(dlogit)
        call('sdmi_scale_dev', _st(), x=_p(dlogit), y=_p(out), s=_p(g.reshape(1).float().contiguous()),
             dtype=_DT[dlogit.dtype], n=dlogit.numel())
        return out, None, None


class MatmulNtFn(torch.autograd.Function):
    """y = x @ w^T in fp32 out of the implicit-GEMM kernel for an explicit weight TENSOR (engine.readout_composed);
    gradient to w only (dw = dy^T x, the same kernel on transposed operands)."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x)
        return ops.linear(x, w.contiguous(), out_dtype=torch.float32)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        M = x.shape[0]
        Mp = (M + 7) // 8 * 8                          # the reduction length must be whole 16-byte vectors
        dyt = torch.zeros((dy.shape[1], Mp), dtype=x.dtype, device=x.device)
        dyt[:, :M] = dy.t()
        xt = torch.zeros((x.shape[1], Mp), dtype=x.dtype, device=x.device)
        xt[:, :M] = x.t()
        return None, ops.linear(dyt, xt, out_dtype=torch.float32)


class VaeAttnFn(torch.autograd.Function):
    """Core of the VQ-VAE AttnBlock (vqvae/modules.py:130-150): one head of width C over S tokens,
    qkv [B,S,3C] -> o [B,S,C], as batched GEMMs (S = q k^T, P = softmax(S / sqrt(C)), o = P v) with
    batched transposes where a product contracts over a leading dimension."""

    @staticmethod
    def forward(ctx, qkv):
        B, S, C3 = qkv.shape
        C = C3 // 3
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        sc = torch.empty((B, S, S), dtype=qkv.dtype, device=qkv.device)
        ops.bmm_nt(q, k, sc)
        ops.softmax_rows_(sc, scale=float(C) ** -0.5)
        o = torch.empty((B, S, C), dtype=qkv.dtype, device=qkv.device)
        ops.bmm_nt(sc, ops.transpose2d(v), o)
        ctx.save_for_backward(qkv, sc)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, p = ctx.saved_tensors
        B, S, C3 = qkv.shape
        C = C3 // 3
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
        do = do.contiguous()
        dqkv = torch.empty_like(qkv)
        dp = torch.empty_like(p)
        ops.bmm_nt(do, v, dp)                                   # dP = dO v^T
        ops.bmm_nt(ops.transpose2d(p), ops.transpose2d(do), dqkv[..., 2 * C:])     # dv = P^T dO
        ops.softmax_rows_bwd_(p, dp, scale=float(C) ** -0.5)    # dp <- dS
        ops.bmm_nt(dp, ops.transpose2d(k), dqkv[..., :C])       # dq = dS k
        ops.bmm_nt(ops.transpose2d(dp), ops.transpose2d(q), dqkv[..., C:2 * C])    # dk = dS^T q
        return dqkv


class VqFn(torch.autograd.Function):
    """VectorQuantizer2.forward (quantize.py:80-123): nearest code with the straight-through
    estimator and the legacy commitment loss.  z [..,4] fp32 NHWC (3 channels used) ->
    (zq, quant_loss, idx); the codebook gradient is accumulated straight into `dcode`."""

    @staticmethod
    def forward(ctx, z, anchor, codebook, dcode, beta):
        idx, zq = ops.vq_nearest(z, codebook)
        dim = codebook.shape[1]
        ql = (ops.mse(zq, z) * (z.shape[-1] / float(dim)) * (1.0 + beta)).reshape(())
        ctx.save_for_backward(z, zq, idx)
        ctx.dcode, ctx.beta, ctx.dim = dcode, beta, dim
        ctx.mark_non_differentiable(idx)
        return zq, ql, idx

    @staticmethod
    def backward(ctx, dzq, dql, _didx):
        z, zq, idx = ctx.saved_tensors
        dz = torch.empty_like(z)
        g = dql.reshape(1).float().contiguous() if dql is not None else \
            torch.zeros(1, dtype=torch.float32, device=z.device)
        dzq = dzq.contiguous() if dzq is not None else None
        call('sdmi_vq_bwd', _st(), z=_p(z), zq=_p(zq), dzq=_p(dzq), dz=_p(dz), dcode=_p(ctx.dcode),
             idx=_p(idx), g=_p(g), R=z.numel() // z.shape[-1], dim=ctx.dim, ldz=z.shape[-1],
             beta=ctx.beta)
        return dz, None, None, None, None


class MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, scale, l1=False):
        val, dpred = ops.mse(pred, target, want_grad=True, gscale=scale, l1=l1, oscale=scale)
        ctx.save_for_backward(dpred)
        return val.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        out = torch.empty_like(dpred)                  # dpred * g, g a device scalar
        call('sdmi_scale_dev', _st(), x=_p(dpred), y=_p(out), s=_p(g.reshape(1).float().contiguous()),
             dtype=_DT[dpred.dtype], n=dpred.numel())
        return out, None, None, None


class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed, seed_dev):
        ctx.p, ctx.seed, ctx.seed_dev = p, seed, seed_dev
        y = torch.empty_like(x)
        call('sdmi_dropout', _st(), x=_p(x), y=_p(y), dtype=_DT[x.dtype], n=x.numel(), p=p, seed=seed,
             seed_dev=_p(seed_dev))
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call('sdmi_dropout', _st(), x=_p(dy), y=_p(dx), dtype=_DT[dy.dtype], n=dy.numel(), p=ctx.p,
             seed=ctx.seed, seed_dev=_p(ctx.seed_dev))
        return dx, None, None, None



# ------------------------------------------------------------------------------------------
# plain-SA decoder pieces (img_based/models/slot_attention.py:343-364)
# ------------------------------------------------------------------------------------------
def _deconv_problem(wb, x, wname, k, stride, pad):
    """The parameter [Cin, Cout, k, k] lies in the arena as [Cin][k][k][Cout] = the weight of the stride-`stride`
    convolution this layer is the data gradient of: that convolution's backward problem (bwd.LayerProblem.transposed)."""
    Cout = wb.w(wname, x.dtype).shape[1] // (k * k)
    return bwd.LayerProblem.transposed(x, Cout, k, stride, pad)


def deconv_forward(wb, x, wname, bname, k, stride, pad, act):
    """ConvTranspose2d(k, stride, padding=pad, output_padding=stride-1) on NHWC: sdmi_igemm on the flipped/transposed
    operand with virtual zero insertion (exactly GemmFn's dgrad launch, plus bias and activation; no residual)."""
    dt = x.dtype
    P = _deconv_problem(wb, x, wname, k, stride, pad)
    wd = wb.wd(wname, dt, k, k, P.Cin)            # [Cout][k'][k'][Cin]
    y = torch.empty((P.B, P.H, P.W, P.Cin), dtype=dt, device=x.device)
    call('sdmi_igemm', _st(), a=_p(x), w=_p(wd), out=_p(y), bias=_p(wb.b(bname)), split_k=1,
         **dict(P.dgrad_fields(), act=_lib.ACT[act], ldr=0))
    return y


class DeconvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, wb, wname, bname, k, stride, pad, act):
        y = deconv_forward(wb, x, wname, bname, k, stride, pad, act)
        ctx.save_for_backward(x, y)
        ctx.cfg = (wb, wname, bname, k, stride, pad, act)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        wb, wname, bname, k, stride, pad, act = ctx.cfg
        dt = x.dtype
        dy = dy.contiguous()
        w = wb.w(wname, dt)
        P = _deconv_problem(wb, x, wname, k, stride, pad)
        Cout = P.Cin
        if act:                                   # relu: act'(z) from the output
            dz = torch.empty_like(dy)
            call('sdmi_act_bwd', _st(), x=_p(y), dy=_p(dy), dx=_p(dz), dtype=_DT[dt],
                 act=_lib.ACT[act], n=dy.numel())
        else:
            dz = dy
        # data gradient = the strided convolution itself
        dx = ops.conv2d(dz, w, None, kh=k, kw=k, stride=stride, pad=(pad, pad, pad, pad)) \
            if ctx.needs_input_grad[0] else None
        # weight gradient: roles swapped (A = dz gathered with the stride, "dY" = x)
        splits = bwd.standalone_splits(P)
        ws = torch.empty((splits * (P.N * P.K + P.N),), dtype=torch.float32, device=x.device)
        call('sdmi_wgrad', _st(), a=_p(dz), dy=_p(x), dw=_p(_grads_of(wb, wname)), dbias=0, workspace=_p(ws),
             splits=splits, accumulate=1, **P.wgrad_fields())
        # bias gradient: column sums of dz in 1024-row chunks, folded into the arena
        rows = P.B * P.H * P.W
        chunk = 1024 if rows % 1024 == 0 else rows
        part = torch.empty((rows // chunk, Cout), dtype=torch.float32, device=x.device)
        call('sdmi_rowgroup_sum', _st(), x=_p(dz), out=_p(part), dtype=_DT[dt], groups=rows // chunk,
             rows_per=chunk, N=Cout, ldx=Cout)
        gb = _grads_of(wb, bname)
        tot = torch.empty((1, Cout), dtype=torch.float32, device=x.device)
        call('sdmi_rowgroup_sum', _st(), x=_p(part), out=_p(tot), dtype=_lib.F32, groups=1,
             rows_per=rows // chunk, N=Cout, ldx=Cout)
        call('sdmi_add', _st(), x=_p(gb), z=_p(tot), y=_p(gb), dtype=_lib.F32, n=Cout)
        return dx, None, None, None, None, None, None, None, None


class BroadcastPosFn(torch.autograd.Function):
    """[G, C] slot vectors -> [G, R, C] (+ position embedding [R, C])."""

    @staticmethod
    def forward(ctx, x, pos, dtype):
        G, C = x.shape
        R = pos.shape[0]
        y = torch.empty((G, R, C), dtype=dtype, device=x.device)
        call('sdmi_broadcast_pos', _st(), x=_p(x.contiguous()), pos=_p(pos.contiguous()), y=_p(y),
             dtype=_DT[dtype], G=G, R=R, C=C)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        G, R, C = dy.shape
        dx = torch.empty((G, C), dtype=torch.float32, device=dy.device)
        call('sdmi_rowgroup_sum', _st(), x=_p(dy), out=_p(dx), dtype=_DT[dy.dtype], groups=G,
             rows_per=R, N=C, ldx=C)
        dpos = torch.empty((R, C), dtype=torch.float32, device=dy.device)
        call('sdmi_rowgroup_sum', _st(), x=_p(dy), out=_p(dpos), dtype=_DT[dy.dtype], groups=1,
             rows_per=G, N=R * C, ldx=R * C)
        return dx, dpos, None


class SaCombineFn(torch.autograd.Function):
    """o [B*N, H, W, ld] (rgb + alpha logit) -> recon [B, H, W, 4] fp32, masks [B, N, H*W] fp32."""

    @staticmethod
    def forward(ctx, o, B, N):
        BN, H, W_, ld = o.shape
        recon = torch.empty((B, H, W_, 4), dtype=torch.float32, device=o.device)
        masks = torch.empty((B, N, H * W_), dtype=torch.float32, device=o.device)
        call('sdmi_sa_combine', _st(), o=_p(o), recon=_p(recon), masks=_p(masks), dtype=_DT[o.dtype],
             B=B, N=N, HW=H * W_, ldo=ld)
        ctx.save_for_backward(o, masks)
        ctx.mark_non_differentiable(masks)
        ctx.set_materialize_grads(False)
        return recon, masks

    @staticmethod
    def backward(ctx, drecon, _dm):
        o, masks = ctx.saved_tensors
        B, N = masks.shape[0], masks.shape[1]
        dout = torch.empty_like(o)
        call('sdmi_sa_combine_bwd', _st(), o=_p(o), masks=_p(masks), drecon=_p(drecon.contiguous()),
             dout=_p(dout), dtype=_DT[o.dtype], B=B, N=N, HW=masks.shape[2], ldo=o.shape[-1])
        return dout, None, None


class NhwcToNchwFn(torch.autograd.Function):
    """fp32 [B, H, W, Cpad] -> [B, C, H, W] with gradient (user-facing recon_img)."""

    @staticmethod
    def forward(ctx, x, C):
        ctx.cpad = x.shape[-1]
        return ops.nhwc_to_nchw(x, C)

    @staticmethod
    def backward(ctx, dy):
        return ops.nchw_to_nhwc(dy.contiguous(), torch.float32, ctx.cpad), None


class KernGrad(Kern):
    """Training provider (autograd)."""
    training = True
    dropout_p = 0.0
    _drop_ctr = 0

    def __init__(self, wb):
        super().__init__(wb)
        # run seed and data-parallel rank: ranks must not share dropout masks
        rank = int(os.environ.get('RANK', 0))
        self.seed = ((int(getattr(wb.model, 'seed', 0)) * 1000003 + rank * 7919 + 1) & 0xffffffff)

    def _p_drop(self, site):
        attr = 'train_dropout' if site == 'unet' else 'pred_dropout'
        return float(getattr(self.wb.model, attr, 0.0))

    def linear_drop_res(self, x, wname, bname, res):
        if self._p_drop('pred') <= 0.0:
            return self.linear(x, wname, bname, residual=res)
        return AddFn.apply(res, self.dropout(self.linear(x, wname, bname), site='pred'))

    def dropout(self, x, site='unet'):
        p = self._p_drop(site)
        if p <= 0.0:
            return x
        # site counter restarts every step (`begin_step`), the per-step variation comes from the
        # device word `model.step_seed` so that a captured HIP graph draws new masks on replay
        self._drop_ctr += 1
        return DropoutFn.apply(x, p, (self.seed << 20) + self._drop_ctr,
                               getattr(self.wb.model, 'step_seed', None))

    def begin_step(self):
        """Start of a training step (eager or under graph capture): advance the device-side seed word
        (a captured add, so replays draw new masks too) and restart the per-step site counter."""
        m = self.wb.model
        dev = m.arena().device
        if getattr(m, 'step_seed', None) is None or m.step_seed.device != dev:
            m.step_seed = torch.zeros(1, dtype=torch.int64, device=dev)
        call('sdmi_counters_inc', _st(), seed=_p(m.step_seed))
        self._drop_ctr = 0

    def conv(self, x, wname, bname=None, *, kh=3, kw=3, stride=1, pad=(1, 1, 1, 1), ups=False,
             rowvec=None, residual=None, out_dtype=None, ldc=None):
        return GemmFn.apply(x, rowvec, residual, self.wb.anchor_for(wname), self.wb, wname, bname,
                            (kh, kw, stride, pad, ups), out_dtype, ldc)

    def linear(self, x, wnames, bnames=None, *, act=None, residual=None, out_dtype=None):
        y = GemmFn.apply(x, None, residual, self.wb.anchor_for(wnames), self.wb, wnames, bnames,
                         (0, 0, 1, (0, 0, 0, 0), False), out_dtype, None)
        return ActFn.apply(y, act) if act else y

    def gn(self, x, name, *, eps, act=None, residual=None, dropout=None, for_conv=None, rowsum_of=None):
        drop = None
        if dropout is not None:
            p = self._p_drop(dropout)
            if p > 0.0:          # fused behind the activation: same seed scheme as DropoutFn
                self._drop_ctr += 1
                drop = (p, (self.seed << 20) + self._drop_ctr, getattr(self.wb.model, 'step_seed', None))
        f8 = self._f8_for(x, for_conv)
        y = GroupNormFn.apply(x, residual, self.wb.anchor_for(name), self.wb, name, eps, act, 0, drop,
                              getattr(rowsum_of, '_sdmi_sink', None), f8)
        if f8 is not None and len(f8) > 1:
            y._sdmi_fp8 = f8[1]
        return y

    def _f8_for(self, x, for_conv):
        """[scale] when the norm's only reader is a convolution that multiplies e4m3fn operands (fp8 configuration):
        the norm writes that operand next to its bf16 output -- no quantisation launch in front of the GEMM."""
        return [FP8_ACT_SCALE] if (for_conv and self.fp8_ok(x, for_conv, 9, False)) else None

    def st_train(self, x, n, heads, kv):
        """The SpatialTransformer block `n` through the fused training kernels (StBlockFn), or None when the block
        does not qualify (the caller runs the per-layer launches): bf16, C = 256 / 384, 32 | tokens per image <= 256,
        <= 16 slots, a grid that fills a good part of the chip."""
        B, H, W, C = x.shape
        S = H * W
        if not (_ST_TRAIN and torch.is_tensor(kv) and x.dtype == torch.bfloat16 and kv.dtype == torch.bfloat16 and
                C in (256, 384) and heads * 32 == C and S % 32 == 0 and S <= 256 and kv.shape[1] <= 16 and
                kv.shape[-1] == 2 * C and kv.stride(-1) == 1 and x.is_contiguous()):
            return None
        rows = _ST_ROWS or (64 if (S % 64 == 0 and B * S // 64 >= 192) else 32)
        if S % rows or B * S // rows < _ST_TRAIN_MIN_WGS:
            return None
        return StBlockFn.apply(x, kv, self.wb.anchor_for(n), self.wb, n, heads, rows)

    def ff_out_proj(self, g, tres, xres, t, n):
        tok = self.linear(g, t + '.ff.net.2.weight', t + '.ff.net.2.bias', residual=tres)
        return self.linear(tok, n + '.proj_out.weight', n + '.proj_out.bias', residual=xres)

    def res_tail(self, h, n, skip):
        if (n + '.skip_connection.weight') in self.wb.t:
            skip = self.conv(skip, n + '.skip_connection.weight', n + '.skip_connection.bias', kh=1, kw=1,
                             pad=(0, 0, 0, 0))
        return self.conv(h, n + '.out_layers.3.weight', n + '.out_layers.3.bias', residual=skip)

    def rowvec_slices(self, rowvecs, bounds):
        if not rowvecs.requires_grad:
            return [rowvecs[:, off:off + c] for off, c in bounds]
        outs = RowvecSplitFn.apply(rowvecs, tuple(bounds))
        sink = outs[0].grad_fn.sink if hasattr(outs[0].grad_fn, 'sink') else None
        for v, (off, c) in zip(outs, bounds):
            v._sdmi_sink = (sink, off)
        return list(outs)

    def gn_fan(self, x, name, *, eps, act=None, residual=None, n_alias=1, for_conv=None):
        f8 = self._f8_for(x, for_conv)
        outs = GroupNormFn.apply(x, residual, self.wb.anchor_for(name), self.wb, name, eps, act, n_alias, None, None, f8)
        if f8 is not None and len(f8) > 1:
            outs[0]._sdmi_fp8 = f8[1]
        return outs

    def linear_fan(self, x, wnames, bnames=None):
        return GemmFn.apply(x, None, None, self.wb.anchor_for(wnames), self.wb, wnames, bnames,
                            (0, 0, 1, (0, 0, 0, 0), False), None, None, 1)

    def linear_multi(self, x, wname_list):
        wname_list = tuple(wname_list)
        return MultiLinearFn.apply(x, self.wb.anchor_for(wname_list[0]), self.wb, wname_list)

    def ln_fan(self, x, name):
        return LayerNormFn.apply(x, self.wb.anchor_for(name), self.wb, name, 1)

    def ln_linear_fan(self, x, ln_name, wnames, bnames=None, *, act=None, geglu=False, eps=1e-5):
        n, xres = self.ln_fan(x, ln_name)          # (training keeps the normalised rows for wgrad)
        if geglu and _GEGLU_FUSE and act is None and isinstance(wnames, str) and n.dtype == torch.bfloat16 \
                and n.shape[-1] % 64 == 0:
            return GegluLinearFn.apply(n, self.wb.anchor_for(wnames), self.wb, wnames, bnames), xres
        h = self.linear(n, wnames, bnames, act=act)
        return (self.geglu(h) if geglu else h), xres

    def conv_fan(self, x, wname, bname=None, *, kh=3, kw=3, stride=1, pad=(1, 1, 1, 1), ups=False,
                 rowvec=None, residual=None, out_dtype=None, ldc=None):
        return GemmFn.apply(x, rowvec, residual, self.wb.anchor_for(wname), self.wb, wname, bname,
                            (kh, kw, stride, pad, ups), out_dtype, ldc, 1)

    def deconv(self, x, wname, bname, *, k, stride, pad, act='relu'):
        return DeconvFn.apply(x, self.wb.anchor_for(wname), self.wb, wname, bname, k, stride, pad, act)

    def broadcast_pos(self, x, pos, dtype):
        return BroadcastPosFn.apply(x, pos, dtype)

    def sa_combine(self, o, B, N):
        return SaCombineFn.apply(o, B, N)

    def ln(self, x, name):
        return LayerNormFn.apply(x, self.wb.anchor_for(name), self.wb, name)

    def attn_self(self, qkv, heads, head_dim=32):
        fits = ops.ATTN_MFMA_MAX_KV if (qkv.dtype == torch.bfloat16 and head_dim == 32) else ops.ATTN_LDS_MAX_KV
        if qkv.shape[1] > fits:
            return LongAttnFn.apply(qkv, heads, head_dim)
        return AttnFn.apply(qkv, None, heads, head_dim)

    def attn_cross(self, q, kv, heads):
        return AttnFn.apply(q, kv, heads)

    def vae_attn_core(self, qkv):
        return VaeAttnFn.apply(qkv)

    def geglu(self, h):
        return GegluFn.apply(h)

    def add_pos(self, x, pos):
        return AddPosFn.apply(x, pos)

    def shift_window(self, win, new, L):
        return ShiftWindowFn.apply(win, new, L)

    def tail_tokens(self, x, n, L):
        return TailTokensFn.apply(x, n, L)

    def concat(self, a, b):
        return ConcatFn.apply(a, b)

    def cast(self, x, dtype):
        return x if x.dtype == dtype else CastFn.apply(x, dtype)

    def lstm_cell(self, z, c_prev):
        return LstmCellFn.apply(z, c_prev)

    def pred_step(self, x, base, wrap, norm_first, state):
        return None                         # (recording gradients: the composed chain is the training path)

    def pred_tf(self, x, base, layers, heads):
        return None                         # (as pred_step)

    def cast_pad(self, x, dtype, cols, ldd):
        return CastPadFn.apply(x, dtype, cols, ldd)

    def slot_attention(self, kv, init, name, iters, eps):
        """Unfused training form of SlotAttentionWMask.forward (sa_diffusion.py:40-68)."""
        B, M, D2 = kv.shape
        D = D2 // 2
        if init.dim() == 2:
            init = init.unsqueeze(0).expand(B, -1, -1)
        slots = init.contiguous()
        N = slots.shape[1]
        seg = None
        # every tensor with several consumers hands out aliases (ln_fan / linear_fan / the kv chain):
        # the consumers' gradients meet inside a backward kernel, not in accumulation kernels
        for it in range(iters):
            nq, s_alias = self.ln_fan(slots, f'{name}.project_q.0')
            q = self.linear(nq, f'{name}.project_q.1.weight')
            if it + 1 < iters:
                upd, attn, kv = SaAttendFn.apply(kv, q, eps, True)
            else:
                upd, attn = SaAttendFn.apply(kv, q, eps)
            seg = attn
            gi = self.linear(upd.reshape(B * N, D), f'{name}.gru.weight_ih', f'{name}.gru.bias_ih')
            gh, prev = self.linear_fan(s_alias.reshape(B * N, D), f'{name}.gru.weight_hh',
                                       f'{name}.gru.bias_hh')
            h = GruGatesFn.apply(gi, gh, prev)
            nh, h_alias = self.ln_fan(h, f'{name}.mlp.0')
            hid = self.linear(nh, f'{name}.mlp.1.weight', f'{name}.mlp.1.bias', act='relu')
            slots = self.linear(hid, f'{name}.mlp.3.weight', f'{name}.mlp.3.bias',
                                residual=h_alias).view(B, N, D)
        return slots, seg
