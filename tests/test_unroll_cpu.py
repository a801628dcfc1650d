"""The rollout stage (slotdiffusion_amd/unroll.py), its data modules and the host side of sdmi_rollout_feed, without a GPU:
the stage's indexing on a stub model, the file round trip into the readout's data module, build_dataset's choice, the
strided windows of SlotsFileDataModule, the packed operands and the geometry predicate."""
import os
import types

import numpy as np
import pytest
import torch

from slotdiffusion_amd import extract, kern, unroll, vp_vqa
from slotdiffusion_amd.method import (SlotsFileDataModule, SlotsLabelFileDataModule, SyntheticSlotsLabelDataModule,
                                      physion_label_key)

N, C = 2, 3


class _Stub:
    """unroll(past, P)[b, k] = sum_j (j + 1) past[b, j] + 1000 (k + 1): step k as a known function of the burn-in
    frames (their order included) and k."""

    def __init__(self, h):
        self.history_len, self.calls = h, []

    def unroll(self, past, pred_len):
        self.calls.append((tuple(past.shape), pred_len))
        assert past.shape[1] == self.history_len
        w = torch.arange(1, self.history_len + 1, dtype=past.dtype).view(1, -1, 1, 1)
        base = (past * w).sum(1, keepdim=True)
        return base + 1000.0 * torch.arange(1, pred_len + 1, dtype=past.dtype).view(1, -1, 1, 1)


def _videos(n, T):
    """Slot values encode (video, frame): 100 v + f + 0.01 (slot, channel index)."""
    fine = 0.01 * np.arange(N * C, dtype=np.float32).reshape(N, C)
    return {f'v{v}.mp4': (100.0 * v + np.arange(T, dtype=np.float32)[:, None, None] + fine).astype(np.float32)
            for v in range(n)}


def _expect(video, f, obs, h, o):
    if f < obs:
        return video[f]
    off, k = (f - obs) % o, (f - obs) // o
    burn = [obs - h * o + off + j * o for j in range(h)]
    return sum((j + 1) * video[t] for j, t in enumerate(burn)) + 1000.0 * (k + 1)


@pytest.mark.parametrize('n,video_len,obs,h,o,bs,calls', [
    (3, 14, 6, 2, 3, 2, [((6, 2, N, C), 3), ((3, 2, N, C), 3)]),      # ragged batch; streams of 3 / 3 / 2 steps
    (2, 9, 4, 3, 1, 1, [((1, 3, N, C), 5)] * 2),                      # offset 1
    (2, 11, 6, 2, 3, 2, [((6, 2, N, C), 2)]),                         # obs = h * offset exactly
])
def test_stage_indexing_on_a_stub_model(n, video_len, obs, h, o, bs, calls):
    vids = _videos(n, video_len + 2)                                   # stored videos are longer than video_len
    files = [f'some/dir/v{v}.mp4' for v in range(n)]
    m = _Stub(h)
    out = unroll.rollout_video_slots(m, vids, files, video_len, obs_frames=obs, frame_offset=o, batch_size=bs)
    assert out.shape == (n, video_len, N, C) and out.dtype == np.float32
    assert m.calls == calls, 'one unroll call per batch, B * offset sequences, the longest stream\'s pred_len'
    for v in range(n):
        vid = vids[f'v{v}.mp4']
        assert np.array_equal(out[v, :obs].view(np.uint32), vid[:obs].view(np.uint32)), 'observed frames are copied'
        for f in range(obs, video_len):
            assert np.allclose(out[v, f], _expect(vid, f, obs, h, o), rtol=0, atol=1e-3), (v, f)


def test_stage_refusals_raise_by_name():
    vids = _videos(2, 10)
    files = ['v0.mp4', 'v1.mp4']
    run = lambda **kw: unroll.rollout_video_slots(_Stub(2), vids, files, **{**dict(video_len=10, obs_frames=6,
                                                                                   frame_offset=3), **kw})
    assert run().shape == (2, 10, N, C)
    with pytest.raises(ValueError, match='obs_frames'):
        run(obs_frames=5)
    with pytest.raises(ValueError, match='video_len'):
        run(video_len=6)
    with pytest.raises(ValueError, match='video_len'):
        run(video_len=11)                                              # the stored videos have 10 frames
    with pytest.raises(KeyError, match='absent'):
        unroll.rollout_video_slots(_Stub(2), vids, ['absent.mp4'], 10, obs_frames=6, frame_offset=3)
    with pytest.raises(ValueError, match='frame_offset'):
        run(frame_offset=0)
    with pytest.raises(ValueError, match='batch_size'):
        run(batch_size=0)


def _readout_params(**kw):
    return types.SimpleNamespace(model='PhysionReadout', train_batch_size=4, video_len=10,
                                 readout_dict=dict(num_slots=N, slot_size=C, agg_func='max', feats_dim=32), **kw)


def _write_csv(path, rows):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        f.write(',stimulus,ground truth outcome,other\n')
        for k, v in rows:
            f.write(f'{k},"a, quoted, field",{v},7\n')


def test_file_round_trip_into_the_readout_data_module(tmp_path):
    src, dst = str(tmp_path / 'slots.pkl'), str(tmp_path / 'out' / 'rollout_readout_slots.pkl')
    names = ['pilot_dominoes_0_img.mp4', 'pilot_roll_3_img.mp4', 'pilot_drop_1_img.mp4']
    vids = _videos(3, 12)
    tr = {n: vids[f'v{i}.mp4'] for i, n in enumerate(names)}
    te = {'pilot_towers_5-redyellow_img.mp4': vids['v1.mp4']}
    extract.dump_slots(src, {'train': (list(tr), list(tr.values())), 'test': (list(te), list(te.values()))})
    wrote = unroll.rollout_slots_file(_Stub(2), src, dst, ('train', 'test'), video_len=10, obs_frames=6, frame_offset=3,
                                      batch_size=2)
    got = extract.load_slots(dst)
    assert sorted(got) == ['test', 'train'] and sorted(got['train']) == sorted(names) and sorted(wrote['train']) == sorted(names)
    for n in names:
        assert got['train'][n].shape == (10, N, C) and got['train'][n].dtype == np.float32
        assert np.array_equal(got['train'][n][:6], tr[n][:6])
        assert np.allclose(got['train'][n][9], _expect(tr[n], 9, 6, 2, 3), atol=1e-3)
    with pytest.raises(KeyError, match='val'):
        unroll.rollout_slots_file(_Stub(2), src, dst, ('val',), video_len=10, obs_frames=6, frame_offset=3)

    csv_tr, csv_te = str(tmp_path / 'readout_labels.csv'), str(tmp_path / 'labels.csv')
    _write_csv(csv_tr, [('pilot_dominoes_0', 'True'), ('pilot_roll_3', 'False'), ('pilot_drop_1', 'True'), ('unused', 'False')])
    _write_csv(csv_te, [('pilot_towers_5_img', 'False')])
    dm = SlotsLabelFileDataModule(_readout_params(), dst, csv_tr, 'train', steps_per_epoch=3, device='cpu', seed=5)
    want = {'pilot_dominoes_0_img.mp4': 1.0, 'pilot_roll_3_img.mp4': 0.0, 'pilot_drop_1_img.mp4': 1.0}
    assert dm.files == sorted(names) and dm.labels == [want[f] for f in dm.files]
    batches = list(dm.train_loader(epoch=1))
    assert len(dm) == 3 and len(batches) == 3
    seen = set()
    for b, vi in zip(batches, dm.batches(1)):
        assert b['slots'].shape == (4, 10, N, C) and b['slots'].dtype == torch.float32 and b['label'].shape == (4,)
        for s, l, v in zip(b['slots'], b['label'], vi):
            assert np.array_equal(s.numpy(), got['train'][dm.files[v]]) and float(l) == want[dm.files[v]]
            seen.add(v)
    assert len(seen) > 1
    again = list(SlotsLabelFileDataModule(_readout_params(), dst, csv_tr, 'train', steps_per_epoch=3, device='cpu',
                                          seed=5).train_loader(1))
    assert all(torch.equal(a['slots'], b['slots']) and torch.equal(a['label'], b['label']) for a, b in zip(batches, again))
    test = SlotsLabelFileDataModule(_readout_params(), dst, csv_te, 'test', device='cpu')
    assert test.labels == [0.0] and physion_label_key('x/pilot_towers_5-redyellow_img.mp4', 'test') == 'pilot_towers_5_img'
    assert physion_label_key('pilot_a_img.mp4', 'train') == 'pilot_a' and physion_label_key('pilot_a_img', 'val') == 'pilot_a'
    _write_csv(csv_tr, [('pilot_dominoes_0', 'True'), ('pilot_roll_3', 'False')])
    with pytest.raises(KeyError, match='pilot_drop_1'):
        SlotsLabelFileDataModule(_readout_params(), dst, csv_tr, 'train', device='cpu')
    with pytest.raises(ValueError, match='video_len'):
        SlotsLabelFileDataModule(types.SimpleNamespace(train_batch_size=1, video_len=13), src, csv_te, 'test', device='cpu')


def test_build_dataset_takes_the_file_module_only_with_both_files(tmp_path):
    root = str(tmp_path / 'data')
    slots = str(tmp_path / 'rollout_readout_slots.pkl')
    csv_path = os.path.join(root, 'PhysionTrainMP4s', 'readout_labels.csv')
    syn = lambda **kw: type(vp_vqa.build_dataset(_readout_params(**kw))) is SyntheticSlotsLabelDataModule
    assert syn() and syn(slots_root=slots, data_root=root)
    vids = _videos(2, 10)
    extract.dump_slots(slots, {'train': (['a_img.mp4', 'b_img.mp4'], list(vids.values())), 'val': (['a_img.mp4'], [vids['v0.mp4']]),
                               'test': (['c-redyellow_img.mp4'], [vids['v1.mp4']])})
    assert syn(slots_root=slots, data_root=root), 'the CSV is absent'
    assert syn(slots_root=slots), 'no data_root'
    _write_csv(csv_path, [('a', 'True'), ('b', 'False')])
    assert syn(slots_root=str(tmp_path / 'absent.pkl'), data_root=root), 'the slots file is absent'
    dm = vp_vqa.build_dataset(_readout_params(slots_root=slots, data_root=root))
    assert type(dm) is SlotsLabelFileDataModule and dm.labels == [1.0, 0.0]
    assert len(vp_vqa.build_dataset(_readout_params(slots_root=slots, data_root=root), val_only=True).videos) == 1
    assert syn(slots_root=slots, data_root=root, dataset='physion_slots_label_test'), 'the test subset has its own CSV'
    _write_csv(os.path.join(root, 'PhysionTestMP4s', 'labels.csv'), [('c_img', 'True')])
    dm = vp_vqa.build_dataset(_readout_params(slots_root=slots, data_root=root, dataset='physion_slots_label_test'))
    assert type(dm) is SlotsLabelFileDataModule and dm.labels == [1.0]


def _former_params():
    return types.SimpleNamespace(model='LDMSlotFormer', train_batch_size=4, rollout_dict={'history_len': 3},
                                 loss_dict={'rollout_len': 2}, slot_dict={'num_slots': N, 'slot_size': C})


def _draw(seed, epoch, steps, B, lens, span):
    """The documented generator sequence: per step one randint for the B video indices, then one per window start."""
    g = torch.Generator().manual_seed(seed + 1000 * epoch)
    out = []
    for _ in range(steps):
        vi = torch.randint(len(lens), (B,), generator=g).tolist()
        out.append([(v, int(torch.randint(lens[v] - span + 1, (1,), generator=g))) for v in vi])
    return out


def test_slots_file_data_module_windows_default_and_strided(tmp_path):
    path = str(tmp_path / 'slots.pkl')
    lens = [13, 16, 15, 9]
    vids = {f'v{i}.mp4': _videos(i + 1, T)[f'v{i}.mp4'] for i, T in enumerate(lens)}
    extract.dump_slots(path, {'train': (list(vids), list(vids.values()))})
    dm = SlotsFileDataModule(_former_params(), path, steps_per_epoch=5, device='cpu', seed=11)
    assert dm.frame_offset == 1 and dm.windows(2) == _draw(11, 2, 5, 4, lens, 5), 'the default draws the parent\'s windows'
    for b, step in zip(dm.train_loader(2), dm.windows(2)):
        for w, (v, t0) in zip(b['slots'].numpy(), step):
            assert np.array_equal(w, vids[f'v{v}.mp4'][t0:t0 + 5])
    ds = SlotsFileDataModule(_former_params(), path, steps_per_epoch=40, device='cpu', seed=11, frame_offset=3)
    assert ds.files == ['v0.mp4', 'v1.mp4', 'v2.mp4'], 'a stride-3 window of 5 frames reaches over 13'
    assert ds.windows(0) == _draw(11, 0, 40, 4, lens[:3], 13)
    starts = {}
    for b, step in zip(ds.train_loader(0), ds.windows(0)):
        assert b['slots'].shape == (4, 5, N, C)
        for w, (v, t0) in zip(b['slots'].numpy(), step):
            assert np.array_equal(w, vids[f'v{v}.mp4'][[t0, t0 + 3, t0 + 6, t0 + 9, t0 + 12]])
            starts.setdefault(v, set()).add(t0)
    assert starts[0] == {0} and starts[1] == {0, 1, 2, 3} and starts[2] == {0, 1, 2}


def _fragment_order(w):
    """Independent statement of the MFMA B-fragment order of a weight [N, K] (sdmi.h: sdmi_pred_step): per chunk of 16
    output rows and k step of 32 columns, lane l holds row l % 16, columns 8 (l // 16) .. + 7."""
    rows, K = w.shape
    out = []
    for c in range(rows // 16):
        for s in range(K // 32):
            for l in range(64):
                out.extend(w[16 * c + l % 16, 32 * s + 8 * (l // 16):32 * s + 8 * (l // 16) + 8])
    return np.asarray(out, dtype=w.dtype)


@pytest.mark.parametrize('Cm,Ds', [(256, 192), (64, 32)])
def test_feed_operands_are_in_fragment_order(Cm, Ds):
    g = torch.Generator().manual_seed(Cm + Ds)
    w_out = torch.randn(Ds, Cm, generator=g).bfloat16().float()          # on the bf16 grid
    w_in = torch.randn(Cm, Ds, generator=g).bfloat16().float()
    b_out, b_in = torch.randn(Ds, generator=g), torch.randn(Cm, generator=g)
    P = kern.rollout_feed_pack(w_out, b_out, w_in, b_in)
    assert P['wout'].dtype == P['win_w'].dtype == torch.bfloat16 and P['C'] == Cm and P['Ds'] == Ds
    assert np.array_equal(P['wout'].float().numpy(), _fragment_order(w_out.numpy()))
    assert np.array_equal(P['win_w'].float().numpy(), _fragment_order(w_in.numpy()))
    assert torch.equal(P['bout'], b_out) and torch.equal(P['bin'], b_in) and P['bout'].dtype == torch.float32
    off = torch.randn(32, 64, generator=g)                               # off the grid: rounded once, to nearest even
    assert torch.equal(kern.rollout_feed_pack(off, b_out[:32], off.t().contiguous(), b_in[:64])['wout'].float(),
                       torch.from_numpy(_fragment_order(off.bfloat16().float().numpy())))


@pytest.mark.parametrize('args,want', [
    # (N, L, Lp, C, Ds)
    ((8, 120, 128, 256, 192), True),                                   # the shipped shape
    ((0, 0, 64, 256, 192), False), ((1, 1, 64, 256, 192), True), ((16, 32, 64, 256, 192), True), ((17, 34, 64, 256, 192), False),
    ((8, 0, 64, 256, 192), False), ((8, 8, 64, 256, 192), True), ((8, 4, 64, 256, 192), False),       # N <= L
    ((8, 60, 64, 256, 192), False), ((8, 56, 64, 256, 192), True),                                     # L % N
    ((8, 64, 64, 256, 192), True), ((8, 72, 64, 256, 192), False),                                     # L <= Lp
    ((8, 16, 64, 32, 192), True), ((8, 16, 64, 0, 192), False), ((8, 16, 64, 16, 192), False), ((8, 16, 64, 48, 192), False),
    ((8, 16, 64, 256, 192), True), ((8, 16, 64, 288, 192), False),
    ((8, 16, 64, 256, 32), True), ((8, 16, 64, 256, 0), False), ((8, 16, 64, 256, 16), False), ((8, 16, 64, 256, 80), False),
    ((8, 16, 64, 256, 256), True), ((8, 16, 64, 256, 288), False),
])
def test_rollout_feed_covers_row_by_row(args, want):
    assert kern.rollout_feed_covers(*args) is want
    assert kern._ROLLOUT_FEED is True
