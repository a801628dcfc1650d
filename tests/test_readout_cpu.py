"""PhysionReadout (vp_vqa) without a GPU: registry, checkpoint keys, the CPU restatement against the reference's
fixture in both of its forms, the fixture's gap condition, calc_eval_loss, the labelled synthetic data, and the C ABI's
argument checks of sdmi_readout_fwd / sdmi_readout_bwd.  No kernel is launched here."""
import importlib

import pytest
import torch

from slotdiffusion_amd import _lib
from tests import common as C
from tests import readout_ref as R


@pytest.fixture(scope='module')
def shipped_model():
    return importlib.import_module('slotdiffusion.vp_vqa').build_model(R.shipped_params())


@pytest.fixture(scope='module')
def golden():
    return C.load_golden('physion_readout_b3.npz')


def test_shipped_config_builds_with_reference_keys(shipped_model):
    m = shipped_model
    assert type(m).__name__ == 'PhysionReadout'
    want = R.key_fixture()
    assert sum(p.numel() for p in m.parameters()) == want['num_params'] == 74113
    assert [[k, list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()] == want['state']   # names, shapes, order
    assert [k for k, _ in m.named_buffers()] == want['buffers'] == ['comb_idx']
    assert m.comb_idx.dtype == torch.int64 and m.comb_idx.tolist() == want['comb_idx']
    assert all(p.requires_grad for p in m.parameters())
    assert m.loss_names == ['vqa_loss'] and m.agg_func == 'max'
    assert m.dtype == torch.float32 and m.device.type == 'cpu'
    m.set_compute_dtype('bf16')
    assert m.compute_dtype == torch.bfloat16 and m.dtype == torch.float32
    m.set_compute_dtype('fp32')


def test_reference_format_state_dict_loads_strictly(shipped_model):
    want = R.key_fixture()
    W = R.det_weights(8, 192, 192)
    sd = {'comb_idx': torch.tensor(want['comb_idx'], dtype=torch.int64)}
    sd.update(W)
    assert list(sd) == [k for k, _, _ in want['state']]
    m = importlib.import_module('slotdiffusion.vp_vqa').build_model(R.shipped_params())
    m.load_state_dict(sd, strict=True)
    for k, v in W.items():
        assert torch.equal(m.state_dict()[k], v)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if k != 'comb_idx'}, strict=True)


@pytest.mark.parametrize('agg', R.AGGS)
def test_cpu_restatement_reproduces_the_reference_fixture(golden, agg):
    """Same torch CPU arithmetic as the reference: 1e-6 in both forms; gradients against the stored ones."""
    G = golden
    W = R.det_weights(8, 192, 192)
    slots, label = G['slots'], G['label']
    assert tuple(slots.shape) == (3, 5, 8, 192)
    with torch.no_grad():
        for fwd in (R.forward_pairs, R.forward_uv):
            logits = fwd(W, slots, agg)
            assert float((logits - G[f'{agg}:logits']).abs().max()) <= 1e-6 * max(1.0, float(G[f'{agg}:logits'].abs().max()))
            assert abs(float(R.vqa_loss(logits, label)) - float(G[f'{agg}:vqa_loss'])) <= 1e-6
    g = R.grads(W, slots, label, agg)
    for k in R.KEYS[1:]:
        ref = G[f'{agg}:grad:{k}']
        assert float((g[k] - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max())), k
    ref = G[f'{agg}:grad_rows4:linear1.weight']
    assert float((g['linear1.weight'][::4] - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max()))


def test_fixture_gap_condition(golden):
    W = R.det_weights(8, 192, 192)
    for agg in R.AGGS:
        tgap, pgap = R.gaps(W, golden['slots'], agg)
        assert tgap >= 1e-3 and pgap >= 1e-4, (agg, tgap, pgap)


def test_calc_eval_loss_keys_and_values(shipped_model, golden):
    for agg in R.AGGS:
        logits, label = golden[f'{agg}:logits'], golden['label']
        want = R.eval_metrics(logits, label)
        assert list(want) == ['vqa_loss', 'acc_0.10', 'acc_0.30', 'acc_0.50', 'acc_0.70', 'acc_0.90']
        for k, v in want.items():
            assert abs(float(v) - float(golden[f'{agg}:{k}'])) <= 1e-6, (agg, k)
    # the model's own calc_eval_loss on logits that came with their loss (as its forward hands them over)
    logits, label = golden['max:logits'], golden['label']
    out = {'logits': logits, 'vqa_loss': golden['max:vqa_loss']}
    got = shipped_model.calc_eval_loss({'label': label.double()}, out)           # the label is cast type_as the logits
    assert list(got) == ['vqa_loss', 'acc_0.10', 'acc_0.30', 'acc_0.50', 'acc_0.70', 'acc_0.90']
    for k, v in got.items():
        assert float(v) == float(golden[f'max:{k}']), k


def test_labelled_synthetic_data_follows_the_planted_rule():
    task = importlib.import_module('slotdiffusion.vp_vqa')
    P = R.shipped_params(train_batch_size=16, video_len=6)
    assert len(task.build_dataset(P)) > 0 and callable(task.build_method)
    dm = type(task.build_dataset(P))(P, device='cpu')
    assert type(dm).__name__ == 'SyntheticSlotsLabelDataModule'
    batches = list(dm.train_loader(0))
    assert len(batches) == len(dm)
    seen = []
    for b in batches:
        assert tuple(b['slots'].shape) == (16, 6, 8, 192) and tuple(b['label'].shape) == (16,)
        i, j = R.pairs(8)
        u, v = b['slots'].double() @ dm.a.double(), b['slots'].double() @ dm.c.double()
        score = (u[:, :, i] + v[:, :, j]).flatten(1).max(1)[0]
        near = (score - dm.thr).abs() < 1e-5
        assert torch.equal((score > dm.thr).float()[~near], b['label'][~near])
        seen.append(b['label'])
    frac = float(torch.cat(seen).mean())
    assert 0.2 < frac < 0.8                      # thr is the median of the score: both classes occur
    again = next(iter(type(dm)(P, device='cpu').train_loader(0)))
    assert torch.equal(again['slots'], batches[0]['slots']) and torch.equal(again['label'], batches[0]['label'])
    other = next(iter(dm.train_loader(1)))
    assert not torch.equal(other['slots'], batches[0]['slots'])


def test_registry_refuses_params_without_readout_dict():
    task = importlib.import_module('slotdiffusion.vp_vqa')
    d = R.shipped_values()
    del d['readout_dict']
    from slotdiffusion_amd import compat
    with pytest.raises(NotImplementedError, match='PhysionReadout is not on the MI355X hot path yet'):
        task.build_model(compat.Params(**d))
    from slotdiffusion_amd import kern, policy
    assert kern._READOUT_FUSED is True and not any('READOUT' in k for k in policy.SWITCHES)
    assert kern.readout_covers(8, 192, 192) and kern.readout_covers(16, 256, 256) and kern.readout_covers(2, 32, 32)
    assert not any(kern.readout_covers(*g) for g in [(1, 192, 192), (17, 192, 192), (8, 200, 192), (8, 288, 192),
                                                     (8, 192, 0), (8, 192, 288), (20, 192, 192)])


def test_pack_index_is_a_permutation_of_linear1():
    from slotdiffusion_amd import kern
    for dt in (torch.float32, torch.bfloat16):
        for Cc, Ff in ((32, 32), (192, 192), (96, 64), (256, 256)):
            idx = kern.readout_pack_index(Cc, Ff, dt)
            assert idx.dtype == torch.int64 and torch.equal(idx.sort()[0], torch.arange(Ff * 2 * Cc))
    # bf16, first k step of chunk 0: lane l holds W_a[l % 32][8 (l // 32) .. + 8], then the same of W_b
    idx = kern.readout_pack_index(192, 192, torch.bfloat16).view(6, 12, 2, 64, 8)
    assert idx[0, 0, 0, 33].tolist() == [1 * 384 + 8 + e for e in range(8)]
    assert idx[2, 3, 1, 5].tolist() == [(64 + 5) * 384 + 192 + 48 + e for e in range(8)]
    idx = kern.readout_pack_index(192, 192, torch.float32).view(6, 24, 2, 64, 4)
    assert idx[1, 2, 1, 40].tolist() == [(32 + 8) * 384 + 192 + 16 + 4 + j for j in range(4)]


FWD_OK = dict(slots=16, w1p=32, b1=48, w2=64, b2=80, label=96, frame_logits=112, logits=128, t_star=144, loss=160,
              dlogit=176, B=2, T=3, N=8, C=192, F=192, agg=2, x_dtype=0, op_dtype=0, phase=0, loss_weight=1.0)
BWD_OK = dict(slots=16, w1p=32, b1=48, w2=64, t_star=80, dlogit=96, gscale=0, dw1=112, db1=128, dw2=144, db2=160,
              B=2, T=3, N=8, C=192, F=192, agg=2, x_dtype=0, op_dtype=1, accumulate=0)
GEOMETRY = [dict(N=1), dict(N=17), dict(C=200), dict(C=288), dict(C=0), dict(F=0), dict(F=200), dict(F=288), dict(T=0),
            dict(B=0), dict(agg=3), dict(agg=-1), dict(x_dtype=2), dict(x_dtype=7), dict(op_dtype=2), dict(op_dtype=-1),
            dict(slots=8), dict(w1p=36)]


@pytest.mark.parametrize('entry, ok, extra', [
    ('sdmi_readout_fwd', FWD_OK, [dict(slots=0), dict(w1p=0), dict(b1=0), dict(w2=0), dict(b2=0), dict(frame_logits=0),
                                  dict(logits=0), dict(t_star=0), dict(loss=0), dict(dlogit=0), dict(phase=3),
                                  dict(phase=-1)]),
    ('sdmi_readout_bwd', BWD_OK, [dict(slots=0), dict(w1p=0), dict(b1=0), dict(w2=0), dict(t_star=0), dict(dlogit=0),
                                  dict(dw1=0), dict(db1=0), dict(dw2=0), dict(db2=0)])])
def test_readout_entry_points_reject_bad_arguments_without_launch(entry, ok, extra):
    for over in extra + GEOMETRY:
        kw = dict(ok, **over)
        with pytest.raises(_lib.SdmiError, match=entry):
            _lib.call(entry, None, **kw)
        assert len(_lib.lib().sdmi_last_error()) > 0, over
