"""Training backward of a convolution / linear layer: its geometry, its launch plan and the ordering of its launches.

`LayerProblem`  -- the geometry of one layer's backward, built once; the scalar fields of every SdmiWgradArgs /
                   SdmiGemmArgs of that backward come from its two methods.
`plan_layer`, `plan_group`, `standalone_splits` -- pure functions (no tensors, no device query): which launch a layer
                   takes, with which M-split, and which weight-gradient kernel the library is expected to dispatch
                   (tests/test_bwd_plan_cpu.py holds them against `sdmi_wgrad_kernel`).
`GradSchedule`  -- main-stream and side-stream writers of the gradient arena and the rules that order them.
"""
import ctypes
from typing import NamedTuple, Optional

import torch

from . import _lib

_DT = {torch.float32: _lib.F32, torch.bfloat16: _lib.BF16}


def _p(t):
    return 0 if t is None else t.data_ptr()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cdiv(a, b):
    return (a + b - 1) // b


class LayerProblem(NamedTuple):
    """Backward geometry of out[B, Ho, Wo, N] = conv(x[B, H, W, Cin]) (a linear layer: H = W = Ho = Wo = 1, B rows).
    M = B * Ho * Wo rows of dY (pitch ldy >= N), K = kh * kw * Cin; pad = (top, bottom, left, right); lda = pixel pitch
    of x.  A transposed convolution is the problem of the strided convolution it is the data gradient of."""
    is_conv: bool
    B: int
    H: int
    W: int
    Ho: int
    Wo: int
    Cin: int
    N: int
    K: int
    M: int
    kh: int
    kw: int
    stride: int
    pad: tuple
    ups: bool
    lda: int
    ldy: int
    dt: torch.dtype

    @classmethod
    def of(cls, x, dy, geom, dt, N):
        """x: the forward input, dy: the output gradient in the compute dtype `dt` (vector-multiple pitch), geom =
        (kh, kw, stride, pad, ups) as the forward took it."""
        kh, kw, stride, pad, ups = geom
        Cin = x.shape[-1]
        if x.dim() == 4 and (kh, kw) != (0, 0):
            return cls.conv(x.shape[0], x.shape[1], x.shape[2], dy.shape[1], dy.shape[2], Cin, N, dy.shape[-1], kh, kw,
                            stride, pad, dt, ups)
        rows = x.numel() // Cin
        return cls(False, rows, 1, 1, 1, 1, Cin, N, Cin, rows, 1, 1, 1, (0, 0, 0, 0), False, x.stride(-2), dy.shape[-1], dt)

    @classmethod
    def conv(cls, B, H, W, Ho, Wo, Cin, N, ldy, kh, kw, stride, pad, dt, ups=False):
        return cls(True, B, H, W, Ho, Wo, Cin, N, kh * kw * Cin, B * Ho * Wo, kh, kw, stride, tuple(pad), bool(ups), Cin,
                   ldy, dt)

    @classmethod
    def transposed(cls, x, Cout, k, stride, pad):
        """ConvTranspose2d(k, stride, padding = pad, output_padding = stride - 1) on x [B, H, W, Cin] -> [B, Ho, Wo, Cout]:
        the stride-`stride` convolution [B, Ho, Wo, Cout] -> [B, H, W, Cin] with the roles swapped -- x is that
        convolution's dY, the layer's output (gradient) its input image."""
        B, H, W, Cin = x.shape
        Ho = (H - 1) * stride - 2 * pad + k + (stride - 1)
        Wo = (W - 1) * stride - 2 * pad + k + (stride - 1)
        return cls.conv(B, Ho, Wo, H, W, Cout, Cin, Cin, k, k, stride, (pad,) * 4, x.dtype)

    @classmethod
    def upsampled(cls, x, Cout):
        """'Nearest 2x, then a 3x3 convolution, pad 1' on x [B, H, W, Cin] -> [B, 2H, 2W, Cout] is ConvTranspose2d(4,
        stride 2, padding 1) with the composite filter W4 (sdmi.h: SDMI_PACK_UPS_*): the 4x4 stride-2 pad-1 convolution
        [B, 2H, 2W, Cout] -> [B, H, W, Cin] with the roles swapped, as in `transposed` -- its forward IS the layer's data
        gradient, its weight gradient (image dY, "output gradient" x, M = B H W low-resolution rows, K = 16 Cout) is
        dW4 [Cin][4][4][Cout]."""
        B, H, W, Cin = x.shape
        return cls.conv(B, 2 * H, 2 * W, H, W, Cout, Cin, Cin, 4, 4, 2, (1, 1, 1, 1), x.dtype)

    # ---- argument-struct fields (pointers, splits / workspace and epilogue switches are the caller's) ----
    def wgrad_fields(self):
        """Scalar SdmiWgradArgs fields of dW[N][K] = dY^T im2col(x)."""
        return dict(dtype=_DT[self.dt], M=self.M, N=self.N, K=self.K, lda=self.lda, ldy=self.ldy, B=self.B, H=self.H,
                    W=self.W, Cin=self.Cin, Ho=self.Ho, Wo=self.Wo, KH=self.kh, KW=self.kw, stride=self.stride,
                    pad_t=self.pad[0], pad_l=self.pad[2], ups=int(self.ups))

    def dgrad_fields(self):
        """Scalar SdmiGemmArgs fields of the data gradient as ONE launch: the stride-1 convolution of dY with the flipped
        operand [Cin][kh][kw][ldy] -- over virtually zero-inserted dY when stride > 1, at twice the resolution for the
        up-sampling form (the caller pools 2 x 2 behind it)."""
        Hs, Ws = (2 * self.H, 2 * self.W) if self.ups else (self.H, self.W)
        kd = self.kh * self.kw * self.ldy
        return dict(dtype=_DT[self.dt], out_dtype=_DT[self.dt], M=self.B * Hs * Ws, N=self.Cin, K=kd, lda=self.ldy, ldw=kd,
                    ldc=self.Cin, B=self.B, H=self.Ho, W=self.Wo, Cin=self.ldy, Ho=Hs, Wo=Ws, KH=self.kh, KW=self.kw,
                    stride=1, pad_t=self.kh - 1 - self.pad[0], pad_l=self.kw - 1 - self.pad[2], ups=0, act=0, alpha=1.0,
                    batch=1, zins=(self.stride if self.stride > 1 else 0), ldr=self.Cin)

    def parity_dgrads(self):
        """Data gradient of a stride-s convolution as plain stride-1 convolutions over dY, one per input-pixel parity
        (py, px): only the filter taps kh = (py + pad_t) mod s (+ s, ...) reach that parity, so each launch uses its
        sub-filter (a strided slice of the flipped operand, from tap (a0, b0)) and writes its pixels interleaved into dx
        (igemm's sub-sampled output placement).  No multiply-adds on inserted zeros: 1/s^2 of the work of the
        zero-insertion form.  -> (every pixel of dx is written, [(a0, b0, SdmiGemmArgs fields)])."""
        s, kh, kw, pad = self.stride, self.kh, self.kw, self.pad
        full = all(len(range((p + pd) % s, k, s)) > 0 for k, pd in ((kh, pad[0]), (kw, pad[2])) for p in range(s))
        subs = []
        for py in range(s):
            ay = (py + pad[0]) % s
            nky, hs = len(range(ay, kh, s)), len(range(py, self.H, s))
            for px in range(s):
                ax = (px + pad[2]) % s
                nkx, ws = len(range(ax, kw, s)), len(range(px, self.W, s))
                if nky == 0 or nkx == 0 or hs == 0 or ws == 0:
                    continue
                K = nky * nkx * self.ldy
                subs.append(((kh - 1 - ay) % s, (kw - 1 - ax) % s, dict(
                    dtype=_DT[self.dt], out_dtype=_DT[self.dt], M=self.B * hs * ws, N=self.Cin, K=K, lda=self.ldy, ldw=K,
                    ldc=self.Cin, B=self.B, H=self.Ho, W=self.Wo, Cin=self.ldy, Ho=hs, Wo=ws, KH=nky, KW=nkx, stride=1,
                    pad_t=(nky - 1) - (py + pad[0] - ay) // s, pad_l=(nkx - 1) - (px + pad[2] - ax) // s, ups=0, act=0,
                    alpha=1.0, batch=1, oH=self.H, oW=self.W, osy=s, osx=s, ooy=py, oox=px, ldr=self.Cin)))
        return full, subs


# ---- launch planning ----------------------------------------------------------------------------------------------
# Stand-alone weight gradient: M is split so that ~0.75 workgroups per CU exist (the launches share the chip with the
# dgrad chain and three more weight-gradient streams; sweep 128 ... 768 on one box: 192-256 best, 512 is +0.7 ... +1.8 ms
# per step) while each still walks >= 8 m-steps (64 rows per step in the bf16 kernel, 32 in the fp32 one).
WG_TARGET, MIN_STEPS, MAX_SPLITS = 192, 8, 512
# Pair launch (round-3 sweeps, profiles/r03_pair_sweep.txt): resident workgroups (2 per CU), of which walk dX tiles, 64-row
# steps per weight-gradient workgroup, 64 x 64 dW tiles below this many 128 x 128 workgroups.
PAIR_SLOTS, PAIR_DGRAD, PAIR_MIN_STEPS, PAIR_WT64 = 512, 256, 8, 96
# Grouped launch: workgroups shared by the problems in proportion to their work (round 6, the fused SpatialTransformer
# block's eight linear layers as two launches: DESIGN section 4, `wgrad_group_kernel`), most splits of one problem.
WQ_TARGET, WQ_MAX_SPLITS = 512.0, 64


class PairPlan(NamedTuple):
    wgrad_tile: int
    dgrad_cap: int
    splits: int


class LayerPlan(NamedTuple):
    path: str                       # 'pair': sdmi_bwd_pair on the main stream; 'side': sdmi_wgrad + its own data gradient
    splits: int                     # of the stand-alone sdmi_wgrad
    kernel: str                     # ... and the kernel sdmi_wgrad is expected to dispatch: 'gemm' | 'c64' | 'halo'
    pair: Optional[PairPlan]


def _mstep(P):
    return 64 if P.dt == torch.bfloat16 else 32


def standalone_splits(P):
    tiles = _cdiv(P.N, 128) * _cdiv(P.K, 128)
    return max(1, min(_cdiv(WG_TARGET, tiles), P.M // (MIN_STEPS * _mstep(P)), MAX_SPLITS))


def _standalone(P, n_cus, wgrad_halo):
    """-> (splits, kernel).  The two direct kernels are taken by wgrad.hip's select_wgrad_bf16 on conditions the sizes
    chosen here must meet; both write M-split partials, so neither exists with one split."""
    splits = 1 if P.M <= 16 * _mstep(P) else standalone_splits(P)      # short contractions: straight into the arena
    same3x3 = (P.dt == torch.bfloat16 and P.is_conv and P.kh == 3 and P.kw == 3 and P.stride == 1 and not P.ups
               and P.pad == (1, 1, 1, 1))
    if (same3x3 and P.Cin == 64 and P.N == 64 and P.W % 64 == 0 and P.H % 4 == 0
            and P.B * (P.H // 4) * (P.W // 64) >= 2 * n_cus):
        return n_cus, 'c64'             # wgrad3x3_c64_kernel: one persistent workgroup per CU and slot
    hw = P.H * P.W
    if (same3x3 and wgrad_halo and P.W in (16, 32, 64) and P.Cin % 64 == 0 and P.N % 64 == 0 and P.Ho == P.H
            and P.Wo == P.W and hw % 256 == 0 and (hw & (hw - 1)) == 0):
        # wgrad3x3_halo_kernel on (64 output x 64 input channel) pairs, one persistent workgroup per CU: slots x pairs
        # fills the chip
        pairs = (P.N // 64) * (P.Cin // 64)
        halo = min(n_cus // pairs, P.M // 256)
        if halo >= 2 and pairs * halo >= 128:
            return halo, 'halo'
    return splits, 'gemm'


def _pairable(P, direct, has_bias, bias_dst, dalias_cols):
    """Data and weight gradient are of the same loader class (1x1 / linear, or a stride-1 same-size convolution) and
    within sdmi_bwd_pair's contract (sdmi.h)."""
    kh, kw, pad = P.kh, P.kw, P.pad
    same = P.is_conv and P.stride == 1 and not P.ups and P.Ho == P.H and P.Wo == P.W
    one = kh == 1 and kw == 1 and P.stride == 1 and not P.ups and pad[0] == 0 and pad[2] == 0
    kd = kh * kw * P.ldy                                # contraction depth of the data gradient
    bk = 64 if kd * 2 >= 512 else 32
    return (P.dt == torch.bfloat16 and direct and P.N > 64 and P.K > 64 and P.Cin > 64
            and (not has_bias or bias_dst) and P.Cin % 8 == 0 and P.ldy % 8 == 0
            and (one or (same and kh * kw <= 32 and P.ldy % bk == 0
                         and pad[0] == pad[1] == (kh - 1) // 2 and pad[2] == pad[3] == (kw - 1) // 2))
            and (dalias_cols is None or dalias_cols == P.Cin)
            and (P.M + (kh + 1) * P.W + 128) * max(P.lda, P.ldy, P.Cin) * 2 < (1 << 31) and P.N * kd * 2 < (1 << 31))


def _pair_plan(P, has_bias):
    """The weight-gradient workgroups take what the data gradient leaves of PAIR_SLOTS resident workgroups, >=
    PAIR_MIN_STEPS 64-row steps each."""
    Md, Nd, Kd = P.B * P.H * P.W, P.Cin, P.kh * P.kw * P.ldy
    t128 = _cdiv(Md, 128) * _cdiv(Nd, 128)
    shallow = P.kh == 1 and P.kw == 1 and Kd * 2 <= 512
    big = t128 >= 192 and not shallow
    tiles_d = t128 if big else _cdiv(Md, 64) * _cdiv(Nd, 64)
    steps = _cdiv(P.M, 64)

    def plan(wt, slots, min_steps):
        tn = _cdiv(P.N, wt)
        tiles_w = tn * _cdiv(P.K, wt) + (tn if has_bias else 0)
        n_d = min(tiles_d, PAIR_DGRAD)
        return tiles_w, n_d, max(1, min((slots - n_d) // tiles_w, steps // min_steps, 256))
    wt = 128
    tiles_w, n_d, splits = plan(128, PAIR_SLOTS, PAIR_MIN_STEPS)
    if not big and PAIR_WT64 and tiles_w * splits < PAIR_WT64:
        # a small layer: 64 x 64 weight-gradient tiles -- four times the workgroups, three per CU
        wt = 64
        tiles_w, n_d, splits = plan(64, PAIR_SLOTS * 3 // 2, max(2, PAIR_MIN_STEPS // 2))
    return PairPlan(wt, _cdiv(n_d, 8) * 8, splits)


def plan_layer(P, *, need_dx, direct, has_bias, bias_dst, dalias_cols, n_cus, pair_bwd=True, wgrad_halo=True):
    """direct: dW goes straight into the gradient arena (one destination of the kernel's [N][K] layout); has_bias /
    bias_dst: the layer has a bias / its gradient has one destination; dalias_cols: columns of the gradient of x's other
    consumer that rides in the data gradient's epilogue (None: there is none)."""
    splits, kernel = _standalone(P, n_cus, wgrad_halo)
    if pair_bwd and need_dx and _pairable(P, direct, has_bias, bias_dst, dalias_cols):
        return LayerPlan('pair', splits, kernel, _pair_plan(P, has_bias))
    return LayerPlan('side', splits, kernel, None)


def plan_group(problems):
    """problems: [(LayerProblem of a bf16 linear layer, has_bias)] of ONE sdmi_wgrad_group launch -> M-splits of each: ~
    WQ_TARGET workgroups over the group, shared in proportion to each problem's work (128 x 128 tiles x 64-row steps),
    every split keeping >= MIN_STEPS steps."""
    tiles = [_cdiv(P.N, 128) * (_cdiv(P.K, 128) + (1 if bias else 0)) for P, bias in problems]
    steps = [_cdiv(P.M, 64) for P, _ in problems]
    total = float(sum(t * st for t, st in zip(tiles, steps)))
    return [max(1, min(max(1, int(round(WQ_TARGET * (t * st) / total / t))), st // MIN_STEPS, WQ_MAX_SPLITS))
            for t, st in zip(tiles, steps)]


# ---- launch ordering ----------------------------------------------------------------------------------------------
class GradSchedule:
    """Who writes a gradient destination, on which stream, in which order.  Weight-gradient launches are off the
    backward critical path (nothing reads them before the optimiser), so they run either inside the layer's
    data-gradient launch on the main stream (`launch_pair`; M-split partials folded by extra workgroups of the NEXT pair
    launch -- the pending fold) or on one of N_SIDE side streams (`side_wgrad`, `launch_group`), joined when the autograd
    pass ends (`join`).  Four rules keep a destination's read-modify-writes in one order:

    1. a pending fold into a parameter runs before any new writer of that parameter;
    2. a main-stream writer waits for the side streams that have launches into the same destination in flight;
    3. a parameter always uses the same side stream (its uses accumulate in stream order), different parameters are
       spread round-robin;
    4. operands of side-stream launches are kept alive until the join (HBM is plentiful), so no allocator stream
       bookkeeping is needed.

    Every operation below enforces them itself; callers hold no scheduling state."""
    N_SIDE = 4       # most weight-gradient launches are small (<= 128 workgroups + their fold): several fit next to the
    #                  dgrad chain

    def __init__(self, overlap):
        self.overlap = overlap            # side streams on (off: every launch on the main stream)
        self._sides, self._side_of = [], {}
        self._keep = []                   # rule 4
        self._pfold = None                # (SdmiWgradArgs fields, workspace) of the pending fold
        self._side_dst = {}               # destination pointer -> side stream with a launch into it in flight
        self._cq, self._cq_after = [], []
        self._groups = 0
        self._join_queued = False

    # -- the rules
    def _side_stream(self, key):
        if not self.overlap:
            return None
        if not self._sides:
            self._sides = [torch.cuda.Stream() for _ in range(self.N_SIDE)]
        i = self._side_of.get(key)
        if i is None:
            i = self._side_of[key] = len(self._side_of) % self.N_SIDE
        return self._sides[i]

    def _fold_first(self, dst_ptrs=None):
        """Rule 1 (own launch).  dst_ptrs given: only when the pending fold targets one of these destinations."""
        pf = self._pfold
        if pf is None:
            return
        if dst_ptrs is not None and pf[0]['dw'] not in dst_ptrs and (not pf[0]['dbias'] or pf[0]['dbias'] not in dst_ptrs):
            return
        self._pfold = None
        self._after_side_writers(pf[0]['dw'], pf[0]['dbias'])
        arr = _lib.struct_array('SdmiWgradArgs', [pf[0]])
        _lib.call('sdmi_wgrad_fold_group', _st(), problems=ctypes.addressof(arr), n=1)

    def _after_side_writers(self, *ptrs):
        """Rule 2."""
        for p_ in ptrs:
            side = self._side_dst.pop(p_, None) if p_ else None
            if side is not None:
                torch.cuda.current_stream().wait_stream(side)

    def _on_side(self, side, launch, dst_ptrs):
        """Run `launch` on `side` behind everything queued on the main stream so far; record its destinations."""
        if side is None:
            launch()
            return
        ev = torch.cuda.Event()
        ev.record()
        side.wait_event(ev)
        with torch.cuda.stream(side):
            launch()
        for p_ in dst_ptrs:
            if p_:
                self._side_dst[p_] = side

    def _ensure_join(self):
        if not self._join_queued:
            self._join_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self.join)

    def join_by_hand(self):
        """Outside an autograd pass: the caller calls join() itself."""
        self._join_queued = True

    # -- the operations
    def launch_pair(self, P, plan, dgrad, wgrad, device):
        """One sdmi_bwd_pair launch on the main stream: dgrad / wgrad are the layer's SdmiGemmArgs / SdmiWgradArgs fields
        (pointers included), plan its PairPlan; the previous launch's pending fold rides along."""
        N, K, splits = P.N, P.K, plan.splits
        self._fold_first((wgrad['dw'], wgrad['dbias']))
        self._after_side_writers(wgrad['dw'], wgrad['dbias'])
        ws = torch.empty((splits * (N * K + N),), dtype=torch.float32, device=device) if splits > 1 else None
        pf, self._pfold = self._pfold, None
        if pf is not None:
            self._after_side_writers(pf[0]['dw'], pf[0]['dbias'])
        d = _lib.struct_array('SdmiGemmArgs', [dgrad])
        w = _lib.struct_array('SdmiWgradArgs', [dict(wgrad, splits=splits, workspace=_p(ws), defer_fold=1)])
        f = _lib.struct_array('SdmiWgradArgs', [pf[0]]) if pf is not None else None
        fl_d = 2.0 * dgrad['M'] * dgrad['N'] * dgrad['K']
        _lib.call('sdmi_bwd_pair', _st(), dgrad=ctypes.addressof(d), wgrad=ctypes.addressof(w),
                  fold=(ctypes.addressof(f) if pf is not None else 0), dgrad_cap=plan.dgrad_cap, wgrad_tile=plan.wgrad_tile,
                  _meta=dict(flops=fl_d + 2.0 * P.M * N * K, flops_dgrad=fl_d,
                             bytes=float(2 * (dgrad['M'] * dgrad['K'] // (P.kh * P.kw) + dgrad['N'] * dgrad['K']
                                              + dgrad['M'] * dgrad['N'] * (2 if dgrad.get('residual', 0) else 1)
                                              + P.M * P.Cin) + 4 * N * K)))
        if splits > 1:            # folded by the next pair launch (or at the join)
            self._pfold = (dict(dw=wgrad['dw'], dbias=wgrad['dbias'], workspace=_p(ws), N=N, K=K, splits=splits,
                                accumulate=wgrad['accumulate']), ws)
            self._ensure_join()

    def side_wgrad(self, key, dst_ptrs, launch, keep):
        """Run `launch` (a parameter's weight / bias gradient launches into dst_ptrs) on the side stream of `key`."""
        self._fold_first(dst_ptrs)
        side = self._side_stream(key)
        self._on_side(side, launch, dst_ptrs)
        if side is not None:
            self._keep.append(keep)
            self._ensure_join()

    def launch_group(self, rows, splits, keep, device):
        """ONE sdmi_wgrad_group launch of `rows` (SdmiWgradArgs fields with pointers) with these M-splits."""
        for kw in rows:
            self._fold_first((kw['dw'], kw['dbias']))
            self._after_side_writers(kw['dw'], kw['dbias'])
        size = lambda kw, sp: sp * (kw['N'] * kw['K'] + kw['N']) if sp > 1 else 0
        ws = torch.empty((max(sum(size(kw, sp) for kw, sp in zip(rows, splits)), 1),), dtype=torch.float32, device=device)
        off, full = 0, []
        for kw, sp in zip(rows, splits):
            full.append(dict(kw, splits=sp))
            if sp > 1:
                full[-1]['workspace'] = ws.data_ptr() + 4 * off
                off += size(kw, sp)
        arr = _lib.struct_array('SdmiWgradArgs', full)
        flops = sum(2.0 * kw['M'] * kw['N'] * kw['K'] for kw in rows)
        self._groups += 1
        self._on_side(self._side_stream(f'wgrad-group-{self._groups % self.N_SIDE}'),
                      lambda: _lib.call('sdmi_wgrad_group', _st(), problems=ctypes.addressof(arr), n=len(rows),
                                        _meta=dict(flops=flops)),
                      [d for kw in rows for d in (kw['dw'], kw['dbias'])])
        self._keep.append(tuple(keep) + (ws,))
        self._ensure_join()

    def queue_colsum(self, partial, nblk, C, out0, out1, after=None):
        """Deferred dgamma / dbeta fold of a normalisation backward: launched, grouped, at the join.  out1 = None: one
        column sum, partial [nblk][C] (a bias gradient).  after: the event behind the side-stream launch that writes
        `partial` (the flush runs on the main stream before the side streams are joined)."""
        self._cq.append((partial, nblk, C, out0, out1))
        if after is not None:
            self._cq_after.append(after)
        self._ensure_join()

    def _flush_colsum(self):
        q, self._cq = self._cq, []
        for ev in self._cq_after:
            torch.cuda.current_stream().wait_event(ev)
        del self._cq_after[:]
        # a parameter used several times per step (Slot Attention iterations, per-frame modules)
        # has several items with the same destination: they go to successive launches (the
        # workgroups of one launch read-modify-write their destinations concurrently)
        chunks = []
        for it in q:
            for ch in chunks:
                if len(ch[0]) < 64 and _p(it[3]) not in ch[1]:
                    break
            else:
                ch = ([], set())
                chunks.append(ch)
            ch[0].append(it)
            ch[1].add(_p(it[3]))
        for chunk, _ in chunks:
            arr = _lib.struct_array('SdmiColsumItem', (dict(partial=_p(partial), out0=_p(o0), out1=_p(o1), nblk=nblk, C=C)
                                                       for partial, nblk, C, o0, o1 in chunk))
            _lib.call('sdmi_colsum_group', _st(), items=ctypes.addressof(arr), n=len(chunk))
        # (the partial buffers die with q: the launches above are ordered before their reuse)

    def join(self):
        self._fold_first()
        self._flush_colsum()
        for side in self._sides:
            torch.cuda.current_stream().wait_stream(side)
        self._keep.clear()
        self._side_dst.clear()
        self._join_queued = False
