"""The fused transformer slot transition and whole-video slot extraction on the GPU: sdmi_pred_tf through the C ABI,
pinned element by element to float64 references (tests/pred_tf_ref.py) computed from the tensors the kernel reads;
engine.encode_stream against model.encode; extract_video_slots end to end.

Kernel pin (U = 2^-24, BF = 2^-8; no norms, no element excused).  Two references, both float64:
  rounding    rounds to bf16 at exactly the feed points sdmi.h lists for sdmi_pred_tf       feed term 2 BF |v|
  unrounded   oracle.transformer_predictor (pred_tf_ref with rnd = ident is that function)  feed term 1.01 BF |v|
and the bound tests/pred_tf_ref.py's header builds stage by stage: (K + 3) U A per product, the feed term per feed point,
the fp32 LayerNorm rows, the scores' error carried through p (1 - p), and the expf row EXPF['exp'].  That row is the
(r, a) test_gpu_predictor.py measured for 1 / (1 + __expf(-x)) against float64 (the same intrinsic; the arguments here
are <= 0, so the values are <= 1), under the cap that file asserts; the kernel stores no probability, so the row cannot
be measured on this kernel directly -- only through the share of the bound below.

What that bound can and cannot see.  Worst-case propagation (`d_a |W|^T`) grows an error by a row's sum of magnitudes at
every product, eight stages deep per layer: with weights at the scale of a trained layer (entries N(0, 1 / K), family
'unit') the bound is far above the values for one layer already and astronomically so for two.  It is asserted on every
case as built, and it is not what gives this file its teeth.  Those are:
  * family 'amp1' (entries N(0, (1 / (0.8 K))^2): a row's magnitudes sum to ~1, an error is not grown by a product):
    one layer's bound against the rounding reference stays at 0.04 - 0.07 where the layer moves x by up to 0.2 - 0.3;
  * TIGHT: against the unrounded float64 reference, per element, 4 x the largest error measured on an MI355X over every
    case of that family in this file -- for family unit over the cases of the same (layers, D, F) -- (a measured term
    where no tight one can be derived; measured against float64, never against the composed GPU chain).  Inputs and kernel
    are deterministic, so the margin of 4 is for other seeds, not for noise;
  * bits: a two-layer launch equals two one-layer launches with layer 0's and layer 1's operands, bit for bit (the layer
    loop, the operand offsets and the LDS reuse across layers); a second launch gives the same bits; the memory behind the
    last sample's row N - 1 changes no output bit.

Measured on an MI355X (every case of this file).  Largest |kernel - unrounded float64| per family (MEASURED below): unit
1.13e-2 - 1.27e-2 for one layer and 1.88e-2 - 1.97e-2 for two (|y| up to 6), amp1 1.92e-4, one-hot 3.703e-2.  Against the ROUNDING reference the
kernel's error is 2e-7 - 6e-7 wherever no bf16 rounding flips (all of amp1 but one case at 4.5e-6, the one-hot case
4.0e-7) and up to 1.4e-2 over two layers of family unit where one does.  Largest share of the derived bound any element
used: 1.25e-4 against the rounding reference and 8.45e-3 against the unrounded one, both in family amp1; in family unit
the shares are below 1e-4 for one layer and below 1e-30 for two (the bound is not informative there, as said above).

Poison and edges as in test_gpu_predictor.py: x lives between guard rows of 8192.0, y between guard rows of -3.0 that
must be unchanged; inputs are unchanged after the launch.

Stream against clip: fp32 engine.encode_stream in chunks of 2 against model.encode on the whole clip, within the bars the
video-model parity tests hold slots to (SAVi 5e-5, SAViDiffusion 1e-4, largest absolute error; measured: the same bits).
bf16, one transition on the model path (frame 0 -> frame 1, with and without pred_rnn), per element, each within 4 x the
figure measured on an MI355X (MEASURED_MODEL): the fused transition's output against the float64 restatement on the
model's own weights, matrices rounded to bf16 as the kernels read them (1.283e-2 of values up to 5.6; with pred_rnn
3.727e-3 of 0.83) -- what a wrong weight key, a stale packed operand, a wrong base name, head count or layer count would
break by O(1) --; against the composed transition (2.035e-2 / 4.600e-3); the frame-1 slots of the bf16 fused stream against
the fp32 model's (3.789e-2 / 2.171e-2 of 5.0, the bf16 encoder included).  The derived bound is asserted there too and is
as uninformative as for family unit.  And the two paths' frame-1 slots against each other: Slot Attention's response to
a perturbation of its initial slots of the size of the two transitions' difference delta is measured on the same launch
(8 random sign patterns of magnitude max |delta|, largest output change L), and the slots must agree within 4 L (delta
itself is bounded by the constant above, so this cannot grow with a wrong transition)."""
import functools

import pytest
import torch

from slotdiffusion_amd import engine, extract, kern
from tests import pred_tf_ref as R
from tests import predictor_ref as PR
from tests.detfill import det_fill_, is_buffer_name
from tests.test_gpu_bwd_helpers import (BF, DEV, U, _call, _end_the_session_on_a_gpu_fault,  # noqa: F401
                                        _gen, _same_bits, _worst)

pytestmark = pytest.mark.gpu

EXPF = {'exp': (4e-7, 2e-7)}     # __expf(v), v <= 0
assert all(r <= 4e-6 and a <= 1e-6 for r, a in EXPF.values())
assert U == R.U and BF == R.BF
# largest |kernel - unrounded float64| over every case of the family (family unit: of the geometry), measured on an
# MI355X; TIGHT = 4 x that
MEASURED = {'amp1': 1.92e-4, 'onehot': 3.703e-2,
            # family unit per (layers, D, F), over N in {1, 7, 16} and B in {1, 3}
            ('unit', 1, 64, 64): 1.132e-2, ('unit', 1, 64, 768): 1.227e-2, ('unit', 1, 192, 64): 1.270e-2,
            ('unit', 1, 192, 768): 1.217e-2, ('unit', 2, 64, 64): 1.887e-2, ('unit', 2, 64, 768): 1.949e-2,
            ('unit', 2, 192, 64): 1.881e-2, ('unit', 2, 192, 768): 1.974e-2}
MARGIN = 4.0
SHARE = {}
POISON_IN, POISON_OUT = 8192.0, -3.0
F32 = torch.float32
OPERANDS = ('wqkv', 'wo', 'w1', 'w2', 'ln1_g', 'ln1_b', 'bqkv', 'bo', 'ln2_g', 'ln2_b', 'b1', 'b2')


def _check(what, out, exact, bound):
    out = out.detach().double().cpu()
    assert out.shape == exact.shape, (what, out.shape, exact.shape)
    assert bool(torch.isfinite(out).all()), what
    err = (out - exact).abs()
    share = float((err / bound.clamp_min(1e-300)).max())
    SHARE[what] = share
    print(f'{what}: max err {float(err.max()):.3e}, largest share of the bound {share:.3g}')
    assert bool((err <= bound).all()), f'{what}: {_worst(err, bound)}'
    return float(err.max())


def _launch(P, xv, y, B, N, D, heads):
    _call('sdmi_pred_tf', x=xv.data_ptr(), y=y.data_ptr(), B=B, N=N, D=D, heads=heads, F=P['F'], layers=P['layers'],
          eps=1e-5, **{k: P[k].data_ptr() for k in OPERANDS})


def _guarded(rows, D, value):
    buf = torch.full((rows + 2, D), value, dtype=F32, device=DEV)
    return buf, buf[1:rows + 1]


def _layer(W, l):
    """Layer l's tensors under layer 0's names."""
    tag = f'.layers.{l}.'
    return {k.replace(tag, '.layers.0.'): v for k, v in W.items() if tag in k}


def _pin(tag, family, N, D, heads, F, L, B, amp=None, qk_gain=1.0, equal_keys=False, x_gain=1.0):
    W = R.weights(D, F, L, seed=D * 7 + F + L, qk_gain=qk_gain, amp=amp)
    P = kern.pred_tf_pack(W, R.NAME, L, device=DEV)
    x = torch.randn(B, N, D, generator=_gen(N * 131 + D + B)) * x_gain
    if equal_keys:
        x[:, N - 1] = x[:, 0]
    xb, xv = _guarded(B * N, D, POISON_IN)
    xv.copy_(x.view(B * N, D))
    before = xb.clone()
    yb, y = _guarded(B * N, D, POISON_OUT)
    runs = []
    for _ in range(2):
        _launch(P, xv, y, B, N, D, heads)
        runs.append(yb.clone())
    assert _same_bits(*runs), 'a second launch gives the same bits'
    assert bool((yb[0] == POISON_OUT).all()) and bool((yb[-1] == POISON_OUT).all()), 'rows the launch does not own'
    assert _same_bits(before, xb), 'inputs are unchanged'
    xb[-1].fill_(float('nan'))                      # the memory behind row N - 1 of the last sample
    _launch(P, xv, y, B, N, D, heads)
    assert _same_bits(runs[0], yb), 'nothing behind the last row is read'
    if L == 2:
        (mb, mid), (zb, z) = _guarded(B * N, D, POISON_OUT), _guarded(B * N, D, POISON_OUT)
        _launch(kern.pred_tf_pack(_layer(W, 0), R.NAME, 1, device=DEV), xv, mid, B, N, D, heads)
        _launch(kern.pred_tf_pack(_layer(W, 1), R.NAME, 1, device=DEV), mid, z, B, N, D, heads)
        assert _same_bits(zb, yb), 'two layers in one launch = two one-layer launches'
    x64 = x.double()
    y_r, d_r, ext = R.ref_and_bound(W, x64, heads, L, rnd=R.bf16, feed=2 * BF, expf=EXPF['exp'])
    y_u, d_u, _ = R.ref_and_bound(W, x64, heads, L, feed=1.01 * BF, expf=EXPF['exp'])
    got = y.view(B, N, D)
    _check(f'{tag} vs rounding fp64', got, y_r, d_r)
    err = _check(f'{tag} vs unrounded fp64', got, y_u, d_u)
    print(f'{tag}: family {family}, |y| max {float(y_u.abs().max()):.3g}, |y - x| max {float((y_u - x64).abs().max()):.3g}, '
          f'pmax {ext["pmax"]:.6f}, smax {ext["smax"]:.3g}')
    measured = MEASURED[(family, L, D, F) if family == 'unit' else family]
    assert err <= MARGIN * measured, (tag, err, measured)
    return ext, got


GEOMS = [(64, 4), (192, 4)]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('L', [1, 2])
@pytest.mark.parametrize('F', [64, 768])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: f'D{g[0]}h{g[1]}')
@pytest.mark.parametrize('N', [1, 7, 16])
def test_pred_tf_against_fp64(N, geom, F, L, B):
    """Weights at a trained layer's scale: head dims 16 and 48, one k step and 24 of the feed-forward, one and two
    layers, one and three workgroups, a full tile / a ragged one / a single row (a softmax over one key)."""
    D, heads = geom
    _pin(f'pred_tf N{N} D{D}h{heads} F{F} L{L} B{B}', 'unit', N, D, heads, F, L, B)


@pytest.mark.parametrize('F', [64, 768])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: f'D{g[0]}h{g[1]}')
@pytest.mark.parametrize('N', [7, 16])
def test_pred_tf_one_layer_inside_a_bound_that_bites(N, geom, F):
    """Family 'amp1': the derived bound against the rounding reference stays below the layer's own effect on x."""
    D, heads = geom
    _pin(f'pred_tf amp1 N{N} D{D}h{heads} F{F}', 'amp1', N, D, heads, F, 1, 3, amp=1.0)
    assert SHARE[f'pred_tf amp1 N{N} D{D}h{heads} F{F} vs rounding fp64'] <= 1.0


def test_pred_tf_nearly_one_hot_softmax():
    """q and k rows of in_proj scaled by 3: scores of tens, a softmax row within 1e-6 of one-hot."""
    ext, _ = _pin('pred_tf one-hot', 'onehot', 7, 64, 4, 64, 1, 3, qk_gain=3.0)
    assert ext['pmax'] >= 1 - 1e-6 and ext['smax'] >= 20, ext


def test_pred_tf_two_equal_keys():
    """Slot N - 1 is a copy of slot 0: their keys, scores and probabilities are equal, and so are their output rows."""
    _, y = _pin('pred_tf equal keys', 'unit', 7, 192, 4, 768, 2, 3, equal_keys=True)
    assert _same_bits(y[:, 0], y[:, 6])


def test_pred_tf_rejects_what_it_does_not_cover():
    W = R.weights(64, 64, 1, seed=3)
    P = kern.pred_tf_pack(W, R.NAME, 1, device=DEV)
    x = torch.zeros(2, 7, 96, device=DEV)
    y = torch.empty_like(x)
    kw = {k: P[k].data_ptr() for k in OPERANDS}
    with pytest.raises(Exception, match='multiple of 16'):
        _call('sdmi_pred_tf', x=x.data_ptr(), y=y.data_ptr(), B=2, N=7, D=96, heads=4, F=64, layers=1, eps=1e-5, **kw)
    with pytest.raises(Exception, match='N <= 16'):
        _call('sdmi_pred_tf', x=x.data_ptr(), y=y.data_ptr(), B=2, N=17, D=64, heads=4, F=64, layers=1, eps=1e-5, **kw)
    with pytest.raises(Exception, match='overlap'):
        _call('sdmi_pred_tf', x=x.data_ptr(), y=x.data_ptr() + 64, B=2, N=7, D=64, heads=4, F=64, layers=1, eps=1e-5, **kw)
    assert kern.KernGrad.pred_tf(None, x, R.NAME, 1, 4) is None


# ------------------------------------------------------------------------------------------
# the stream
# ------------------------------------------------------------------------------------------
SLOTS, DS, T, BV = 5, 64, 5, 2
HEADS = {64: 2, 192: 4}
BARS = {'SAVi': 5e-5, 'SAViDiffusion': 1e-4}


@functools.lru_cache(None)
def _model(name, rnn=False, dtype=F32, slots=SLOTS, D=DS, ffn=128):
    """res 32, 5 slots of 64, a 2-layer 2-head transformer transition (head dim 32: the composed chain's attention
    kernel takes head dims 32 / 48 / 64 only; ffn 128), optionally LSTM-wrapped (hidden 2 D); the end-to-end test asks
    for the shipped transition instead (8 slots of 192, 4 heads of 48, ffn 768)."""
    from slotdiffusion_amd import models
    cfg = PR.tiny_cfg(name, 'transformer_rnn')
    cfg['slot_dict'] = dict(num_slots=slots, slot_size=D, slot_mlp_size=2 * D, num_iterations=2)
    cfg['enc_dict']['enc_out_channels'] = D
    if name == 'SAVi':
        cfg['dec_dict']['dec_channels'] = (D, 16, 16, 16, 16)
    else:
        cfg['dec_dict']['unet_dict']['context_dim'] = D
    cfg['pred_dict'] = dict(pred_type='transformer', pred_rnn=rnn, pred_norm_first=True, pred_num_layers=2,
                            pred_num_heads=HEADS[D], pred_ffn_dim=ffn, pred_sg_every=None)
    cls = getattr(models, cfg.pop('model'))
    cfg.pop('input_frames')
    m = cls(clip_len=T, **cfg, compute_dtype=dtype)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    return m.cuda().eval()


def _clip(seed=4, frames=T):
    return (torch.randn(BV, frames, 3, 32, 32, generator=_gen(seed)) * 0.5).clamp(-1, 1)


def _encode(m, img):
    out = m.encode(img)
    return out[0] if isinstance(out, tuple) else out


def _stream(m, img, chunk):
    prev, parts = None, []
    for t0 in range(0, img.shape[1], chunk):
        s = m.encode_stream(img[:, t0:t0 + chunk].contiguous(), prev)
        prev = s[:, -1]
        parts.append(s)
    return torch.cat(parts, 1)


@pytest.mark.parametrize('name,rnn', [('SAVi', False), ('SAViDiffusion', False), ('SAVi', True)])
def test_stream_in_chunks_matches_the_clip_fp32(name, rnn):
    """Chunks of 2, 2, 1 frames against the whole clip of 5; with pred_rnn the (h, c) state crosses both boundaries."""
    m = _model(name, rnn)
    img = _clip().cuda()
    with torch.no_grad():
        want = _encode(m, img).clone()
        got = _stream(m, img, 2)
        if rnn:
            assert m.pred_state.step == T - 1
    err = float((got - want).abs().max())
    print(f'{name} rnn={rnn}: stream vs clip max err {err:.2e} of {float(want.abs().max()):.2f}')
    assert got.shape == want.shape == (BV, T, SLOTS, DS) and err <= BARS[name]


def _spy(fn):
    seen, orig = [], kern.call
    from slotdiffusion_amd import ops

    def spy(fname, *a, **k):
        seen.append(fname)
        return orig(fname, *a, **k)
    kern.call = ops.call = spy
    try:
        out = fn()
    finally:
        kern.call = ops.call = orig
    return out, seen


@pytest.mark.parametrize('rnn', [False, True])
def test_recurrence_is_two_calls_per_frame(rnn):
    """bf16: after the first frame's sdmi_slot_attention the recurrence is [sdmi_pred_tf, (sdmi_pred_step,)
    sdmi_slot_attention] per frame; what follows is the T strided copies that stack the frames."""
    m = _model('SAVi', rnn, torch.bfloat16)
    img = _clip().cuda()
    m.encode_stream(img)                                    # (weight preparation stays out of the count)
    _, seen = _spy(lambda: m.encode_stream(img))
    i0 = seen.index('sdmi_slot_attention')
    per = ['sdmi_pred_tf'] + (['sdmi_pred_step'] if rnn else []) + ['sdmi_slot_attention']
    assert seen[i0 + 1:i0 + 1 + len(per) * (T - 1)] == per * (T - 1), seen[i0:]
    assert seen[i0 + 1 + len(per) * (T - 1):] == ['sdmi_cast2d'] * T, seen[i0:]
    assert len(per) == (3 if rnn else 2) and 'sdmi_pred_tf' not in seen[:i0]
    kern._PRED_TF = False
    try:
        _, seen = _spy(lambda: m.encode_stream(img))
    finally:
        kern._PRED_TF = True
    assert 'sdmi_pred_tf' not in seen and seen.count('sdmi_igemm') > 8 * (T - 1)


# largest errors of ONE transition on the model path (frame 0 -> frame 1 of _clip(frames=2), bf16 SAVi of _model),
# measured on an MI355X, per pred_rnn: the fused transition's output against the float64 restatement on the operands
# the kernels read (`lat`), the fused against the composed transition output (`delta`), and the frame-1 slots of the
# bf16 fused stream against the fp32 model's (`slots`; this one includes the bf16 encoder).  Asserted with MARGIN = 4.
MEASURED_MODEL = {False: dict(lat=1.283e-2, delta=2.035e-2, slots=3.789e-2),     # |lat| up to 5.6, |slots| up to 5.0
                  True: dict(lat=3.727e-3, delta=4.600e-3, slots=2.171e-2)}       # |lat| up to 0.83


def _transition_fp64(m, s0, rnn):
    """The model's first transition after a reset in float64, matrices rounded to bf16 as the fused kernels read them."""
    W = {k: v.detach().float().cpu() for k, v in m.state_dict().items() if k.startswith('predictor.')}
    Wq = {k: (R.bf16(v) if v.dim() == 2 else v).double() for k, v in W.items()}
    base = 'predictor.base_predictor' if rnn else 'predictor'
    y, d, _ = R.ref_and_bound(Wq, s0.double().cpu(), HEADS[DS], 2, feed=1.01 * BF, expf=EXPF['exp'], name=base)
    if rnn:
        y = PR.lstm_step(Wq, y.reshape(-1, DS), None, 'predictor')[0].view(y.shape)
    return y, d


@pytest.mark.parametrize('rnn', [False, True])
def test_bf16_model_transition_fused_against_fp64_composed_and_fp32(rnn):
    """One transition on the model path (K.pred_tf, the weight bank's packed operands, base name, heads, layers; with
    pred_rnn the sdmi_pred_step launch behind it), per element: the fused output against float64 and against the
    composed chain, the frame-1 slots against the fp32 model -- each within 4 x its MEASURED_MODEL figure; and
    |slots_fused - slots_composed| on frame 1 within 4 L, L = Slot Attention's measured response to perturbations of
    its initial slots of the size of the two transitions' difference."""
    m = _model('SAVi', rnn, torch.bfloat16)
    img = _clip(frames=2).cuda()
    K = m.K()
    want = MEASURED_MODEL[rnn]
    with torch.no_grad():
        s0 = m.encode_stream(img[:, :1].contiguous())[:, 0].contiguous()
        lat_f = engine.stream_transition(K, s0, m.pred_dict, m.pred_state)
        m.pred_state.reset()
        kern._PRED_TF = False
        try:
            lat_c = engine.stream_transition(K, s0, m.pred_dict, m.pred_state)
            both_c = m.encode_stream(img)
        finally:
            kern._PRED_TF = True
        both_f = m.encode_stream(img)
        slots32 = _model('SAVi', rnn).encode_stream(img)
        assert _same_bits(both_f[:, 0], both_c[:, 0])
        y64, d_u = _transition_fp64(m, s0, rnn)
        e_lat = float((lat_f.double().cpu() - y64).abs().max())
        if not rnn:
            _check('model transition fused vs unrounded fp64', lat_f, y64, d_u)
        delta = float((lat_f - lat_c).abs().max())
        e_slots = float((both_f[:, 1] - slots32[:, 1]).abs().max())
        # Slot Attention on frame 1's tokens from lat_c and from lat_c +- delta
        tok = engine.encoder_out(K, m._to_nhwc(img[:, 1].contiguous()), m.rplan)
        x = K.ln(tok, 'slot_attention.norm_inputs')
        kv = K.linear(x, ('slot_attention.project_k.weight', 'slot_attention.project_v.weight'))
        sa = lambda lat: K.slot_attention(kv, lat.contiguous(), 'slot_attention', m.num_iterations, m.eps)[0]
        base = sa(lat_c)
        g = _gen(21)
        L = 0.0
        for _ in range(8):
            sign = (torch.randint(0, 2, lat_c.shape, generator=g).float() * 2 - 1).cuda()
            L = max(L, float((sa(lat_c + delta * sign) - base).abs().max()))
    err = float((both_f[:, 1] - both_c[:, 1]).abs().max())
    print(f'rnn={rnn} frame 1: fused transition vs fp64 {e_lat:.3e} (|lat| max {float(y64.abs().max()):.3g}), vs composed '
          f'{delta:.3e}; slots vs the fp32 model {e_slots:.3e} (|slots| max {float(slots32.abs().max()):.3g}), fused vs '
          f'composed slots {err:.3e}, measured response L {L:.3e}')
    assert e_lat <= MARGIN * want['lat'], (e_lat, want)
    assert 0 < delta <= MARGIN * want['delta'], (delta, want)
    assert e_slots <= MARGIN * want['slots'], (e_slots, want)
    assert err <= 4 * L


def test_extract_end_to_end(tmp_path):
    """3 synthetic videos of 7 frames, batches of 2, chunks of 3 -> [3, 7, N, C] finite; video 2 alone gives the same
    bits; the dumped file feeds one LDMSlotFormer forward (the shipped geometry: 8 slots of 192; 5 frames of history, 2
    rolled out, 2 layers) through SlotsFileDataModule."""
    import types
    import numpy as np
    from slotdiffusion_amd.method import SlotsFileDataModule
    from tests import slotformer_ref as SF
    SLOTS, DS = 8, 192
    m = _model('SAVi', True, torch.bfloat16, SLOTS, DS, 768)
    ds = extract.SyntheticVideoDataset(types.SimpleNamespace(resolution=(32, 32)), num_videos=3, video_len=7, seed=3)
    slots = extract.extract_video_slots(m, ds, batch_size=2, chunk_len=3)
    assert slots.shape == (3, 7, SLOTS, DS) and slots.dtype == np.float32 and bool(np.isfinite(slots).all())
    assert float(np.abs(slots[:, 1:] - slots[:, :-1]).max()) > 0

    class _Only:
        num_videos = 1

        def get_video(self, i):
            return ds.get_video(2)
    alone = extract.extract_video_slots(m, _Only(), batch_size=2, chunk_len=3)
    assert np.array_equal(alone[0].view(np.uint32), slots[2].view(np.uint32)), 'video 2 alone gives the same bits'
    path = str(tmp_path / 'slots.pkl')
    extract.dump_slots(path, {'train': (ds.files, slots), 'val': (ds.files[:1], slots[:1])})
    sf = SF.build(history_len=5, num_slots=SLOTS, num_layers=2, rollout_len=2).cuda().eval()
    params = SF.shipped_params(num_layers=2, rollout_len=2, history_len=5)
    dm = SlotsFileDataModule(params, path, steps_per_epoch=1)
    batch = next(iter(dm.train_loader(0)))
    assert dm.T == 7 and batch['slots'].shape == (params.train_batch_size, 7, SLOTS, DS)
    with torch.no_grad():
        out = sf(batch)
    assert bool(torch.isfinite(out['pred_slots']).all())
