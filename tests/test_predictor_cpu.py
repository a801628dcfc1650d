"""The residual-MLP and LSTM-wrapped slot transitions of SAVi / SAViDiffusion, host side: parameter layout against the
reference's recorded state_dict keys (tests/golden/savi_pred_family.npz, tools/gen_golden_pred.py), the torch
restatement tests/predictor_ref.py against the reference's recorded outputs, and the reset / carry / detach
bookkeeping of engine.PredictorState.  No GPU."""
import numpy as np
import pytest
import torch

from slotdiffusion_amd import compat, engine, models, spec
from tests import predictor_ref as R

NEW = ('mlp', 'mlp_rnn', 'transformer_rnn')           # the three variants the constructors used to refuse
G = R.load_fixture()

# predictor_ref against the recorded outputs: both sides are fp32 torch on the CPU, so the bound is the fp32 error of the
# restatement itself, measured against its own fp64 evaluation on the same inputs and weights (restatement_error), with
# a factor 4 for the reference's different (fused LSTM / linear kernel) summation order; never below 16 fp32 ulps of the
# output's magnitude.
ULP = 2.0 ** -24


def restatement_error(case, x):
    W32, W64 = R.fixture_weights(G, case), R.fixture_weights(G, case, torch.float64)
    p32, p64 = R.Predictor(W32, R.pred_dict(case)), R.Predictor(W64, R.pred_dict(case))
    err = 0.0
    for t in range(x.shape[0]):
        err = max(err, float((p32(x[t]).double() - p64(x[t].double())).abs().max()))
    return err


@pytest.mark.parametrize('model', ['SAVi', 'SAViDiffusion'])
@pytest.mark.parametrize('case', NEW)
def test_spec_keys_shapes_order_match_reference(model, case):
    cfg = R.tiny_cfg(model, case)
    fn = spec.savi_model if model == 'SAVi' else spec.savi_diffusion
    sp = fn(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'])
    pred = [p for p in sp if p.name.startswith('predictor.')]
    assert sp[-len(pred):] == pred, 'the predictor comes last in state_dict order (savi.py:154-170)'
    assert [p.name for p in pred] == ['predictor.' + str(k) for k in G[f'{case}/keys']]
    assert [p.shape for p in pred] == [tuple(int(v) for v in s if v >= 0) for s in G[f'{case}/shapes']]
    assert all(p.trainable for p in pred)


def test_lstm_init_bound_is_one_over_sqrt_hidden():
    sp = spec.rnn_wrapper('predictor', R.D, R.H)
    rnn = [p for p in sp if '.rnn.' in p.name]
    assert len(rnn) == 4 and all(p.init == 'gru' and p.fan_in == R.H for p in rnn)
    m = R.build_tiny('SAVi', 'mlp_rnn')
    fresh = models.SAVi(**{k: v for k, v in R.tiny_cfg('SAVi', 'mlp_rnn').items() if k not in ('model', 'input_frames')},
                        clip_len=4)
    for p in rnn:
        v = fresh.state_dict()[p.name]
        assert float(v.abs().max()) <= R.H ** -0.5 and float(v.abs().max()) > 0.5 * R.H ** -0.5
    assert m.state_dict()[rnn[0].name].shape == (4 * R.H, R.D)


@pytest.mark.parametrize('model', ['SAVi', 'SAViDiffusion'])
@pytest.mark.parametrize('case', NEW)
def test_build_model_constructs_and_state_dict_round_trips(model, case):
    cfg = R.tiny_cfg(model, case)
    m = models.build_model(compat.Params(**cfg))
    assert type(m).__name__ == model
    keys = [k for k in m.state_dict() if k.startswith('predictor.')]
    assert keys == ['predictor.' + str(k) for k in G[f'{case}/keys']]
    W = R.fixture_weights(G, case)
    sd = {k: (W[k] if k in W else v.clone()) for k, v in m.state_dict().items()}
    missing, unexpected = m.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    for k, v in W.items():
        assert torch.equal(m.state_dict()[k].cpu(), v), k


@pytest.mark.parametrize('case', list(R.VARIANTS))
def test_restatement_reproduces_reference_outputs(case):
    x = torch.from_numpy(G[f'{case}/x'])
    W = R.fixture_weights(G, case)
    p = R.Predictor(W, R.pred_dict(case))
    y = torch.stack([p(x[t]) for t in range(4)])
    p.reset()
    yr = p(x[1])
    want, want_r = torch.from_numpy(G[f'{case}/y']), torch.from_numpy(G[f'{case}/y_reset'])
    bound = max(4 * restatement_error(case, x), 16 * ULP * float(want.abs().max()))
    e, er = float((y - want).abs().max()), float((yr - want_r).abs().max())
    print(f'{case}: four calls {e:.2e}, after reset {er:.2e}, bound {bound:.2e}')
    assert e <= bound and er <= bound
    if R.VARIANTS[case]['pred_rnn']:                   # the state matters: call 1 differs from a fresh call on x[1]
        assert float((want[1] - want_r).abs().max()) > 100 * bound


class _Tok:
    """Stands in for a tensor: remembers whether it was detached."""

    def __init__(self, name, cut=False):
        self.name, self.cut = name, cut

    def detach(self):
        return _Tok(self.name, True)


def test_state_resets_on_new_video_and_carries_on_continuation():
    s = engine.PredictorState()
    s.begin_forward(None)
    x, hid = s.enter(_Tok('x0'))
    assert hid is None and s.step == 0 and not x.cut
    s.leave((_Tok('h0'), _Tok('c0')))
    s.begin_forward(prev_slots=object())              # continuation of a long video: carried
    x, hid = s.enter(_Tok('x1'))
    assert [h.name for h in hid] == ['h0', 'c0'] and s.step == 1 and not any(h.cut for h in hid)
    s.leave((_Tok('h1'), _Tok('c1')))
    s.begin_forward(None)                             # a new video: zero state, the count restarts
    assert s.hidden is None and s.step == 0


def test_state_detaches_exactly_every_k_calls():
    s = engine.PredictorState(sg_every=2)
    s.begin_forward(None)
    cuts = []
    for step in range(7):
        assert s.cuts() == (step in (2, 4, 6))
        x, hid = s.enter(_Tok(f'x{step}'))
        cuts.append(x.cut)
        if step == 0:
            assert hid is None
        else:
            assert all(h.cut == x.cut for h in hid) and [h.name for h in hid] == [f'h{step - 1}', f'c{step - 1}']
        s.leave((_Tok(f'h{step}'), _Tok(f'c{step}')))
    assert cuts == [False, False, True, False, True, False, True]
    never = engine.PredictorState(sg_every=None)
    for step in range(5):
        assert not never.cuts()
        never.leave(None)


def test_state_detach_works_on_tensors():
    s = engine.PredictorState(sg_every=1)
    a = torch.ones(2, requires_grad=True)
    s.leave((a * 2, a * 3))
    x, (h, c) = s.enter(a * 5)
    assert not x.requires_grad and not h.requires_grad and not c.requires_grad


def test_pack_index_is_a_permutation_in_fragment_order():
    from slotdiffusion_amd import kern
    for N, K, gates in ((64, 32, 1), (32, 64, 1), (4 * 64, 96, 4)):
        idx = kern.pred_pack_index(N, K, gates)
        assert sorted(idx.tolist()) == list(range(N * K))
        w = torch.arange(N * K).reshape(N, K)
        p = w.reshape(-1)[idx].reshape(N // gates // 16, K // 32, gates, 64, 8)
        # chunk 1 (0 where there is one chunk), k step 1 (0 ...), last gate, lane 37, element 5
        c, s = min(1, p.shape[0] - 1), min(1, p.shape[1] - 1)
        row, col = (gates - 1) * (N // gates) + 16 * c + 37 % 16, 32 * s + 8 * (37 // 16) + 5
        assert int(p[c, s, gates - 1, 37, 5]) == row * K + col
    assert all(kern.pred_step_covers(d, h) for d, h in ((128, 256), (192, 384), (256, 512), (32, 64), (32, 0)))
    assert not kern.pred_step_covers(40, 24) and not kern.pred_step_covers(288, 512) and not kern.pred_step_covers(128, 544)
