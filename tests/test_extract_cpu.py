"""Whole-video slot extraction, host side: the packed operands and the geometry gate of sdmi_pred_tf, the extractor's
chunk / state bookkeeping on a stub model, the slots file and the data module that reads it.  No GPU."""
import types

import numpy as np
import pytest
import torch

from slotdiffusion_amd import engine, extract, kern, vp_vqa
from slotdiffusion_amd.method import SlotsFileDataModule, SyntheticSlotsDataModule
from tests import pred_tf_ref as R


def _fragment_order(w):
    """Independent statement of the MFMA B-fragment order of a weight [N, K] (sdmi.h: sdmi_pred_step / sdmi_pred_tf):
    per chunk of 16 output rows and k step of 32 columns, lane l holds row l % 16, columns 8 (l // 16) .. + 7."""
    N, K = w.shape
    out = np.empty(N * K, dtype=w.dtype)
    i = 0
    for c in range(N // 16):
        for s in range(K // 32):
            for l in range(64):
                for e in range(8):
                    out[i] = w[16 * c + l % 16, 32 * s + 8 * (l // 16) + e]
                    i += 1
    return out


@pytest.mark.parametrize('D', [32, 64])
def test_in_proj_operand_is_in_fragment_order(D):
    F, layers = 64, 2
    W = R.weights(D, F, layers, seed=D)
    P = kern.pred_tf_pack(W, R.NAME, layers)
    idx = kern.pred_pack_index(3 * D, D).numpy()
    for i in range(layers):
        w = W[f'{R.NAME}.transformer_encoder.layers.{i}.self_attn.in_proj_weight'].numpy()
        want = _fragment_order(w)
        assert np.array_equal(w.reshape(-1)[idx], want)
        got = P['wqkv'][i * 3 * D * D:(i + 1) * 3 * D * D].float().numpy()
        assert np.array_equal(got, want)            # (the test weights are on the bf16 grid)
    assert P['wqkv'].dtype == torch.bfloat16 and P['wqkv'].numel() == layers * 3 * D * D
    assert P['w1'].numel() == layers * F * D and P['w2'].numel() == layers * D * F and P['wo'].numel() == layers * D * D
    w2 = W[f'{R.NAME}.transformer_encoder.layers.1.linear2.weight'].numpy()
    assert np.array_equal(P['w2'][D * F:].float().numpy(), _fragment_order(w2))
    assert P['bqkv'].shape == (layers, 3 * D) and P['b1'].shape == (layers, F) and P['ln2_g'].shape == (layers, D)
    assert P['F'] == F and P['layers'] == layers
    assert torch.equal(P['b1'][1], W[f'{R.NAME}.transformer_encoder.layers.1.linear1.bias'])


@pytest.mark.parametrize('args,want', [
    ((0, 192, 4, 768, 2), False), ((1, 192, 4, 768, 2), True), ((16, 192, 4, 768, 2), True), ((17, 192, 4, 768, 2), False),
    ((15, 192, 4, 768, 2), True),           # head_dim 48: the shipped configurations
    ((8, 96, 4, 768, 2), False),            # head_dim 24
    ((8, 192, 4, 1056, 2), False), ((8, 192, 4, 1024, 4), True), ((8, 192, 4, 1024, 5), False), ((8, 192, 4, 768, 0), False),
    ((8, 288, 6, 768, 2), False), ((8, 256, 4, 768, 2), True), ((8, 256, 2, 768, 2), False),      # D <= 256; head_dim <= 64
    ((8, 192, 5, 768, 2), False), ((8, 192, 4, 784, 2), False), ((8, 64, 4, 64, 1), True), ((8, 48, 3, 64, 1), False),
])
def test_pred_tf_covers_row_by_row(args, want):
    assert kern.pred_tf_covers(*args) is want


class _StubModel:
    """Records what the extractor asks of a video model."""
    clip_len = 4
    N, C = 3, 5

    def __init__(self):
        self.pred_state = engine.PredictorState()
        self.resets, self.calls, self.evals = 0, [], 0
        reset = self.pred_state.reset

        def counting_reset():
            self.resets += 1
            reset()
        self.pred_state.reset = counting_reset
        self.gen = torch.Generator().manual_seed(5)

    def eval(self):
        self.evals += 1
        return self

    def encode_stream(self, img, prev_slots=None):
        self.pred_state.begin_forward(prev_slots)
        B, Tc = img.shape[:2]
        out = torch.randn(B, Tc, self.N, self.C, generator=self.gen)
        self.calls.append((B, Tc, None if prev_slots is None else prev_slots.clone(), out.clone(), img[:, :, 0, 0, 0].clone()))
        return out


def test_extractor_chunks_carry_slots_and_reset_once_per_batch():
    ds = extract.SyntheticVideoDataset(types.SimpleNamespace(resolution=(8, 8)), num_videos=3, video_len=7, seed=2)
    m = _StubModel()
    out = extract.extract_video_slots(m, ds, batch_size=2, chunk_len=3)
    assert m.evals == 1 and isinstance(out, np.ndarray) and out.shape == (3, 7, m.N, m.C)
    assert [(B, Tc) for B, Tc, *_ in m.calls] == [(2, 3), (2, 3), (2, 1), (1, 3), (1, 3), (1, 1)]
    assert m.resets == 2, 'PredictorState is reset at the first chunk of a batch of videos only'
    for i, (B, Tc, prev, ret, _) in enumerate(m.calls):
        if i % 3 == 0:
            assert prev is None
        else:
            assert torch.equal(prev, m.calls[i - 1][3][:, -1])
    got = torch.cat([torch.cat([c[3] for c in m.calls[:3]], 1), torch.cat([c[3] for c in m.calls[3:]], 1)])
    assert np.array_equal(out, got.numpy())
    # the frames arrive in order: video 2's chunks are its frames 0-2, 3-5, 6
    v2 = ds.get_video(2)['video']
    assert torch.equal(torch.cat([c[4] for c in m.calls[3:]], 1)[0], v2[:, 0, 0, 0])
    # default chunk: model.clip_len
    m2 = _StubModel()
    extract.extract_video_slots(m2, ds, batch_size=3)
    assert [(B, Tc) for B, Tc, *_ in m2.calls] == [(3, 4), (3, 3)] and m2.resets == 1


def test_synthetic_videos_depend_on_seed_and_index_alone():
    p = types.SimpleNamespace(resolution=16)
    a, b = extract.SyntheticVideoDataset(p, 3, 4, seed=1), extract.SyntheticVideoDataset(p, 5, 4, seed=1)
    assert a.num_videos == 3 and a.get_video(2)['video'].shape == (4, 3, 16, 16)
    assert torch.equal(a.get_video(2)['video'], b.get_video(2)['video'])
    assert not torch.equal(a.get_video(1)['video'], a.get_video(2)['video'])
    assert float(a.get_video(0)['video'].abs().max()) <= 1.0 and len(set(a.files)) == 3


def _slots_file(tmp_path, T=9):
    g = np.random.default_rng(0)
    tr = g.standard_normal((4, T, 3, 8)).astype(np.float32)
    va = g.standard_normal((2, T, 3, 8)).astype(np.float32)
    path = str(tmp_path / 'sub' / 'slots.pkl')
    extract.dump_slots(path, {'train': ([f'/data/train/v{i}.mp4' for i in range(4)], tr),
                              'val': ([f'/data/val/w{i}.mp4' for i in range(2)], va)})
    return path, tr, va


def test_slots_file_round_trip(tmp_path):
    path, tr, va = _slots_file(tmp_path)
    d = extract.load_slots(path)
    assert set(d) == {'train', 'val'} and sorted(d['train']) == [f'v{i}.mp4' for i in range(4)]
    assert sorted(d['val']) == ['w0.mp4', 'w1.mp4']
    for i in range(4):
        a = d['train'][f'v{i}.mp4']
        assert isinstance(a, np.ndarray) and a.shape == (9, 3, 8) and np.array_equal(a, tr[i])
    assert np.array_equal(d['val']['w1.mp4'], va[1])
    import pickle
    assert isinstance(pickle.load(open(path, 'rb')), dict)              # the reference's reader is a plain unpickle
    with pytest.raises(AssertionError):
        extract.dump_slots(path, {'train': (['a/x.mp4', 'b/x.mp4'], tr[:2])})


def _params(**kw):
    return types.SimpleNamespace(model='LDMSlotFormer', train_batch_size=4, rollout_dict={'history_len': 3},
                                 loss_dict={'rollout_len': 2}, slot_dict={'num_slots': 3, 'slot_size': 8}, **kw)


def test_slots_file_data_module_cuts_seeded_contiguous_windows(tmp_path, monkeypatch):
    path, tr, _ = _slots_file(tmp_path)
    dm = SlotsFileDataModule(_params(), path, steps_per_epoch=3, device='cpu', seed=7)
    batches = [b['slots'] for b in dm.train_loader(epoch=1)]
    assert len(dm) == 3 and len(batches) == 3 and all(b.shape == (4, 5, 3, 8) and b.dtype == torch.float32 for b in batches)
    again = [b['slots'] for b in SlotsFileDataModule(_params(), path, steps_per_epoch=3, device='cpu', seed=7).train_loader(1)]
    assert all(torch.equal(a, b) for a, b in zip(batches, again))
    other = [b['slots'] for b in dm.train_loader(epoch=2)]
    assert not all(torch.equal(a, b) for a, b in zip(batches, other))
    monkeypatch.setenv('RANK', '1')
    rank1 = [b['slots'] for b in SlotsFileDataModule(_params(), path, steps_per_epoch=3, device='cpu', seed=7).train_loader(1)]
    assert not all(torch.equal(a, b) for a, b in zip(batches, rank1))
    for b in batches + other + rank1:
        for w in b.numpy():
            hits = [(v, t0) for v in range(4) for t0 in range(9 - 5 + 1) if np.array_equal(tr[v, t0:t0 + 5], w)]
            assert len(hits) == 1, 'a window is a contiguous slice of one stored video'
    starts = {t0 for step in dm.windows(1) + dm.windows(2) for _, t0 in step}
    assert len(starts) > 1
    val = SlotsFileDataModule(_params(), path, split='val', device='cpu')
    assert len(val.videos) == 2
    with pytest.raises(AssertionError):
        SlotsFileDataModule(types.SimpleNamespace(train_batch_size=1, rollout_dict={'history_len': 8},
                                                  loss_dict={'rollout_len': 2}), path)


def test_build_dataset_selects_the_file_module_only_for_an_existing_slots_root(tmp_path):
    assert type(vp_vqa.build_dataset(_params())) is SyntheticSlotsDataModule
    assert type(vp_vqa.build_dataset(_params(slots_root=str(tmp_path / 'absent.pkl')))) is SyntheticSlotsDataModule
    path, _, _ = _slots_file(tmp_path)
    dm = vp_vqa.build_dataset(_params(slots_root=path))
    assert type(dm) is SlotsFileDataModule and len(dm.videos) == 4
    assert len(vp_vqa.build_dataset(_params(slots_root=path), val_only=True).videos) == 2


def test_public_surface():
    from slotdiffusion_amd import video_based
    assert video_based.extract_video_slots is extract.extract_video_slots
    assert kern.KernGrad.pred_tf(None, None, None, 2, 4) is None
    assert kern._PRED_TF is True


def test_reference_restatement_matches_the_oracle():
    """tests/pred_tf_ref.py with no rounding is oracle.transformer_predictor; on the small-amplitude weight family its
    fp32-only bound for one layer is finite and small, and rounding at the feed points stays inside the bound that
    allows for it."""
    from oracle import slotdiff_oracle as O
    x = torch.randn(2, 7, 64, generator=torch.Generator().manual_seed(3)).double()
    for amp, layers in ((None, 2), (1.0, 1)):
        W = R.weights(64, 64, layers, seed=1, amp=amp)
        y, d, _ = R.ref_and_bound(W, x, 4, layers, expf=(4e-7, 2e-7))
        want = O.transformer_predictor({k: v.double() for k, v in W.items()}, x, layers, 4, name=R.NAME)
        assert float((y - want).abs().max()) <= 1e-12
        assert bool(torch.isfinite(d).all()) and float(d.min()) > 0
    assert float(d.max()) < 1e-3
    yr, dr, _ = R.ref_and_bound(W, x, 4, 1, rnd=R.bf16, feed=2 * R.BF, expf=(4e-7, 2e-7))
    assert bool(((yr - y).abs() <= dr).all()) and float(dr.max()) < 0.1
