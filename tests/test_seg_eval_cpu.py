"""Segmentation evaluation, host side: the scores on contingency tables against the reference's own metric functions
(tests/golden/seg_eval_ref.npz, recorded by tools/gen_golden_seg.py), the overlap argument of the metric functions, the
drivers' chunk / average / NaN bookkeeping on a stub model, and the argument refusals of sdmi_seg_tables.  No GPU."""
import types

import numpy as np
import pytest
import torch

from slotdiffusion_amd import _lib, engine, evaluate, extract
from slotdiffusion_amd import metrics as MT
from tests import common as C

KEYS = ('ari', 'fari', 'miou', 'fmiou', 'mbo')
TOL = 1e-6              # tests/test_oracle_golden.py on metrics_b4.npz: per-image ARI equal, batch values within 1e-6


@pytest.fixture(scope='module')
def G():
    g = C.load_golden('seg_eval_ref.npz')
    return {k: (v.long() if k in ('gt', 'pred', 'overlap') else v) for k, v in g.items()}


def cpu_tables(gt, pred, overlap=None, num_true=None, num_pred=None):
    """[B, ...] ids -> int64 [B, Kg + 1, N] with torch.bincount: sdmi_seg_tables' layout (row Kg: overlapped pixels)."""
    B = gt.shape[0]
    Kg = int(num_true if num_true is not None else int(gt.max()) + 1)
    N = int(num_pred if num_pred is not None else int(pred.max()) + 1)
    rows = gt if overlap is None else torch.where(overlap != 0, torch.full_like(gt, Kg), gt)
    flat = (rows.reshape(B, -1) * N + pred.reshape(B, -1)).long()
    return torch.stack([torch.bincount(flat[b], minlength=(Kg + 1) * N).view(Kg + 1, N) for b in range(B)])


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all(np.abs(a - b)[~np.isnan(a)] <= TOL))


def test_fixture_holds_the_cases_it_is_for(G):
    gt, pred, ov = G['gt'], G['pred'], G['overlap']
    assert gt.shape == (4, 16, 16) and int(gt.max()) <= 5 and int(pred.max()) <= 5
    assert int(gt[1].max()) == 0                                                  # background only
    assert len(pred[2].unique()) < len(gt[2].unique())                            # M < N
    top = int(pred[3].max())
    assert bool((ov[3][pred[3] == top] == 1).all()) and int((pred[3] == top).sum()) > 0
    assert np.isnan(float(G['plain/fmiou_per_image'][1])) and np.isnan(float(G['overlap/mbo_per_image'][1]))


@pytest.mark.parametrize('tag', ['plain', 'overlap'])
def test_scores_from_tables_reproduce_the_reference(G, tag):
    gt, pred = G['gt'], G['pred']
    ov = G['overlap'] if tag == 'overlap' else None
    tabs = cpu_tables(gt, pred, ov)
    per = MT.scores_from_tables(tabs)
    assert np.array_equal(per['ari'], G[f'{tag}/ari_batch_per_image'].numpy())
    assert np.array_equal(per['fari'], G[f'{tag}/fari_batch_per_image'].numpy())
    for k in ('miou', 'fmiou', 'mbo'):
        assert _close(per[k], G[f'{tag}/{k}_per_image']), (k, per[k])
    vals = MT.batch_scores(tabs)
    for k in KEYS:
        assert abs(vals[k] - float(G[f'{tag}/{k}'])) <= TOL, (k, vals[k])
    # one sample at a time: its own one_hot widths, as a batch of one
    for i in range(4):
        one = MT.scores_from_tables(cpu_tables(gt[i:i + 1], pred[i:i + 1], None if ov is None else ov[i:i + 1]))
        for k in KEYS:
            assert _close(one[k], G[f'{tag}/{k}_per_image'][i:i + 1]), (k, i)
    # wider tables than the ids need (the kernel's N is the slot count) change nothing
    wide = MT.scores_from_tables(cpu_tables(gt, pred, ov, num_true=9, num_pred=11))
    assert all(np.array_equal(wide[k], per[k], equal_nan=True) for k in KEYS)


def test_overlap_rule_takes_the_maximum_before_the_overwrite(G):
    gt, pred, ov = G['gt'][3:4], G['pred'][3:4], G['overlap'][3:4]
    t = MT._resolve_overlap(cpu_tables(gt, pred, ov)[0])
    top = int(pred.max())
    assert t.shape == (int(gt.max()) + 1, top + 2)
    assert int(t[:, top].sum()) == 0, 'every pixel of the largest id is overlapped'
    assert int(t[0, top + 1]) == int(ov.sum()) and int(t[1:, top + 1].sum()) == 0
    assert int(t.sum()) == 256
    none = MT._resolve_overlap(cpu_tables(gt, pred)[0])
    assert int(none[:, -1].sum()) == 0 and torch.equal(none[:, :-1], cpu_tables(gt, pred)[0][:-1])


def test_video_tables_fold_time_into_the_pixel_axis(G):
    gv, pv = G['gt'].view(2, 2, 16, 16), G['pred'].view(2, 2, 16, 16)
    tabs = cpu_tables(gv, pv)
    per = MT.scores_from_tables(tabs)
    assert np.array_equal(per['ari'], G['video/ari_per_video'].numpy())
    assert np.array_equal(per['fari'], G['video/fari_per_video'].numpy())
    assert _close(per['miou'], G['video/miou_per_video']) and _close(per['mbo'], G['video/mbo_per_video'])
    vals = MT.batch_scores(tabs)
    for k in KEYS:
        assert abs(vals[k] - float(G[f'video/{k}'])) <= TOL, k
    # a video's table is the sum of its frames' tables
    frames = cpu_tables(G['gt'], G['pred'], num_true=6, num_pred=6).view(2, 2, 7, 6).sum(1)
    assert torch.equal(frames, cpu_tables(gv, pv, num_true=6, num_pred=6))


def test_metric_functions_take_the_overlap_argument(G, monkeypatch):
    """The five public functions with the reference's third argument, on the CPU through the table path: the device
    kernel behind metrics.contingency is replaced by a bincount (its device requirement itself is unchanged)."""
    gt, pred, ov = G['gt'], G['pred'], G['overlap']
    with pytest.raises(RuntimeError):
        MT.ARI_metric(gt, pred, ov)                                  # CPU tensors: still refused

    def bincount_contingency(true_ids, pred_ids, num_true=None, num_pred=None):
        return cpu_tables(true_ids, pred_ids, None, num_true, num_pred)[:, :-1]
    monkeypatch.setattr(MT, 'contingency', bincount_contingency)
    fns = dict(ari=MT.ARI_metric, fari=MT.fARI_metric, miou=MT.miou_metric, fmiou=MT.fmiou_metric, mbo=MT.mbo_metric)
    for k, fn in fns.items():
        assert abs(float(fn(gt, pred, ov)) - float(G[f'overlap/{k}'])) <= TOL, k
        assert abs(float(fn(gt, pred, inst_overlap_mask=ov)) - float(G[f'overlap/{k}'])) <= TOL, k
        assert abs(float(fn(gt, pred)) - float(G[f'plain/{k}'])) <= TOL, k
        assert abs(float(fn(gt, pred, None)) - float(G[f'plain/{k}'])) <= TOL, k
    # an all-zero overlap map is no overlap
    for k, fn in fns.items():
        assert abs(float(fn(gt, pred, torch.zeros_like(ov))) - float(G[f'plain/{k}'])) <= TOL, k


# ----------------------------------------------------------------------------------------------------------------------
# driver bookkeeping on a stub model
# ----------------------------------------------------------------------------------------------------------------------
class _StubVideoModel:
    clip_len = 4
    N = 5

    def __init__(self):
        self.pred_state = engine.PredictorState()
        self.resets, self.evals, self.calls = 0, 0, []
        reset = self.pred_state.reset

        def counting_reset():
            self.resets += 1
            reset()
        self.pred_state.reset = counting_reset

    def eval(self):
        self.evals += 1
        return self


def _stub_chunk_tables(pred_of):
    """A chunk_tables_fn that 'predicts' pred_of(frame) and counts on the CPU; slots carry the index of the last frame."""
    def fn(model, chunk, prev, gt, counts, num_true):
        model.pred_state.begin_forward(prev)
        B, Tc = chunk.shape[:2]
        first = 0 if prev is None else int(prev[0, 0, 0]) + 1
        model.calls.append((B, Tc, None if prev is None else prev.clone(), first, chunk[:, :, 0, 0, 0].clone()))
        pred = torch.stack([pred_of(gt[:, t].long(), first + t) for t in range(Tc)], 1)
        add = cpu_tables(gt.long(), pred, None, num_true, model.N).unsqueeze(1)
        counts = add if counts is None else counts + add
        return torch.full((B, model.N, 3), float(first + Tc - 1)), counts
    return fn


def _ds(num_videos=3, video_len=7, seed=2):
    return extract.SyntheticVideoSegDataset(types.SimpleNamespace(resolution=(8, 8)), num_videos=num_videos, video_len=video_len,
                                            seed=seed, num_objects=3)


def test_synthetic_video_masks():
    a, b = _ds(), _ds(num_videos=5)
    d = a.get_video(2)
    assert d['video'].shape == (7, 3, 8, 8) and d['masks'].shape == (7, 8, 8) and d['masks'].dtype == torch.int64
    assert torch.equal(d['masks'], b.get_video(2)['masks']) and not torch.equal(d['masks'], a.get_video(1)['masks'])
    assert int(d['masks'].min()) == 0 and 1 <= int(d['masks'].max()) <= 3
    base = extract.SyntheticVideoDataset(types.SimpleNamespace(resolution=(8, 8)), num_videos=3, video_len=7, seed=2)
    assert torch.equal(d['video'], base.get_video(2)['video']) and 'masks' not in base.get_video(2)


def test_video_driver_walks_every_frame_once_and_carries_state():
    ds = _ds()
    m = _StubVideoModel()
    pred_of = lambda g, t: (g + t) % 5
    res = evaluate.evaluate_video_segmentation(m, ds, batch_size=2, chunk_len=3, metrics=('ARI', 'fARI', 'miou', 'fmiou', 'mbo'),
                                               chunk_tables_fn=_stub_chunk_tables(pred_of))
    assert m.evals == 1
    assert [(B, Tc) for B, Tc, *_ in m.calls] == [(2, 3), (2, 3), (2, 1), (1, 3), (1, 3), (1, 1)]
    assert [c[3] for c in m.calls] == [0, 3, 6, 0, 3, 6], 'the last slots of a chunk start the next one'
    assert [c[2] is None for c in m.calls] == [True, False, False, True, False, False]
    assert m.resets == 2, 'PredictorState is reset at the first chunk of a batch of videos only'
    v2 = ds.get_video(2)['video']
    assert torch.equal(torch.cat([c[4] for c in m.calls[3:]], 1)[0], v2[:, 0, 0, 0])
    # one table per video over all frames, whatever the chunk length
    got = [t for tabs in res['tables'] for t in tabs[:, 0]]
    assert len(got) == 3 and all(int(t.sum()) == 7 * 64 for t in got)
    for i in range(3):
        g = ds.get_video(i)['masks']
        pred = torch.stack([pred_of(g[t], t) for t in range(7)])
        assert torch.equal(got[i], cpu_tables(g[None], pred[None], None, got[i].shape[0] - 1, 5)[0])     # (Kg is the batch's)
    for cl, bs in ((1, 2), (7, 2), (4, 2), (None, 2)):
        m2 = _StubVideoModel()
        r2 = evaluate.evaluate_video_segmentation(m2, ds, batch_size=bs, chunk_len=cl, metrics=('ARI', 'fARI', 'miou', 'fmiou', 'mbo'),
                                                  chunk_tables_fn=_stub_chunk_tables(pred_of))
        assert all(torch.equal(a, b) for a, b in zip(r2['tables'], res['tables'])), cl
        assert r2['metrics'] == res['metrics']
        if cl is None:
            assert [(B, Tc) for B, Tc, *_ in m2.calls] == [(2, 4), (2, 3), (1, 4), (1, 3)]          # default: model.clip_len
    # the numbers: per batch the reference's value, averaged with weight B
    b0, b1 = MT.batch_scores(res['tables'][0][:, 0]), MT.batch_scores(res['tables'][1][:, 0])
    for name, k in (('ARI', 'ari'), ('fARI', 'fari'), ('miou', 'miou'), ('fmiou', 'fmiou'), ('mbo', 'mbo')):
        assert abs(res['metrics'][name] - (2 * b0[k] + 1 * b1[k]) / 3) <= 1e-12
        assert res['per_sample'][name].shape == (3,) and res['nan_batches'][name] == 0


def test_video_driver_truncates_to_seq_len():
    ds = _ds()
    m = _StubVideoModel()
    res = evaluate.evaluate_video_segmentation(m, ds, batch_size=3, chunk_len=2, seq_len=5,
                                               chunk_tables_fn=_stub_chunk_tables(lambda g, t: g % 5))
    assert [(B, Tc) for B, Tc, *_ in m.calls] == [(3, 2), (3, 2), (3, 1)]
    assert all(int(t.sum()) == 5 * 64 for t in res['tables'][0][:, 0])
    assert set(res['metrics']) == {'fARI', 'miou', 'mbo'}                   # the three the reference reports
    assert abs(res['metrics']['fARI'] - 1.0) <= 1e-6 and abs(res['metrics']['mbo'] - 1.0) <= 1e-6     # pred == gt
    m = _StubVideoModel()
    evaluate.evaluate_video_segmentation(m, ds, batch_size=3, chunk_len=4, seq_len=-1,
                                         chunk_tables_fn=_stub_chunk_tables(lambda g, t: g % 5))
    assert [(B, Tc) for B, Tc, *_ in m.calls] == [(3, 4), (3, 3)]


class _StubImageModel:
    def eval(self):
        return self


def _image_tables_fn(model, batch, num_true):
    maps = [batch['masks']] + ([batch['sem_masks']] if 'sem_masks' in batch else [])
    return torch.stack([cpu_tables(m, batch['pred'], batch.get('inst_overlap_masks'), num_true, 6) for m in maps], 1)


def test_image_driver_average_is_weighted_and_leaves_nan_batches_out(G):
    gt, pred, ov = G['gt'], G['pred'], G['overlap']
    img = torch.zeros(4, 3, 16, 16)
    batches = [dict(img=img[:3], masks=gt[[0, 2, 3]], pred=pred[[0, 2, 3]]),
               dict(img=img[:1], masks=gt[1:2], pred=pred[1:2]),                   # background only: fmiou / mbo are NaN
               dict(img=img[:2], masks=gt[[3, 1]], pred=pred[[3, 1]])]
    names = ('ARI', 'fARI', 'miou', 'fmiou', 'mbo')
    res = evaluate.evaluate_image_segmentation(_StubImageModel(), batches, metrics=names, tables_fn=_image_tables_fn)
    assert set(res['metrics']) == set(names)
    vals = [MT.batch_scores(cpu_tables(b['masks'], b['pred'])) for b in batches]
    for name, k in zip(names, KEYS):
        if k in ('fmiou', 'mbo'):
            assert np.isnan(vals[1][k]) and res['nan_batches'][name] == 1
            want = (3 * vals[0][k] + 2 * vals[2][k]) / 5
        else:
            assert res['nan_batches'][name] == 0
            want = (3 * vals[0][k] + 1 * vals[1][k] + 2 * vals[2][k]) / 6
        assert abs(res['metrics'][name] - want) <= 1e-12, name
        assert res['per_sample'][name].shape == (6,)
    assert np.isnan(res['per_sample']['mbo'][3]) and np.isnan(res['per_sample']['mbo'][5])
    # the whole fixture as one batch is the reference's number
    one = evaluate.evaluate_image_segmentation(_StubImageModel(), [dict(img=img, masks=gt, pred=pred, inst_overlap_masks=ov)],
                                               metrics=names, tables_fn=_image_tables_fn)
    for name, k in zip(names, KEYS):
        assert abs(one['metrics'][name] - float(G[f'overlap/{k}'])) <= TOL
    # every batch NaN: the average is NaN and every batch is counted
    allnan = evaluate.evaluate_image_segmentation(_StubImageModel(), [batches[1], batches[1]], metrics=('mbo',),
                                                  tables_fn=_image_tables_fn)
    assert np.isnan(allnan['metrics']['mbo']) and allnan['nan_batches']['mbo'] == 2


def test_image_driver_scores_instance_and_semantic_masks(G):
    gt, pred, ov = G['gt'], G['pred'], G['overlap']
    sem = (gt + 1) // 2                                           # pairs of instances share a class; one more id range
    batch = dict(img=torch.zeros(4, 3, 16, 16), masks=gt, sem_masks=sem, inst_overlap_masks=ov, pred=pred)
    res = evaluate.evaluate_image_segmentation(_StubImageModel(), [batch], tables_fn=_image_tables_fn)
    assert set(res['metrics']) == {f'{p}/{m}' for p in ('inst', 'sem') for m in ('fARI', 'miou', 'mbo')}
    assert res['tables'][0].shape == (4, 2, int(gt.max()) + 2, 6)
    for k, name in (('fari', 'fARI'), ('miou', 'miou'), ('mbo', 'mbo')):
        assert abs(res['metrics'][f'inst/{name}'] - float(G[f'overlap/{k}'])) <= TOL
        assert abs(res['metrics'][f'sem/{name}'] - MT.batch_scores(cpu_tables(sem, pred, ov))[k]) <= 1e-12
    assert res['metrics']['sem/miou'] != res['metrics']['inst/miou']


# ----------------------------------------------------------------------------------------------------------------------
# the entry point refuses bad arguments before any launch
# ----------------------------------------------------------------------------------------------------------------------
def test_seg_tables_rejects_bad_arguments_without_launch():
    ok = dict(seg=64, gt=128, gt2=192, overlap=256, counts=320, ids=384, ids_u8=0, B=2, T=3, time_major=1, N=7, h=8, w=8, H=32,
              W=32, Kg=6, map_bstride=3 * 1024, map_tstride=1024)
    bad = [dict(seg=0), dict(gt=0), dict(counts=0),                                   # null pointers
           dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(B=0), dict(T=0), dict(time_major=2),
           dict(Kg=0), dict(Kg=1170, N=7), dict(Kg=8192, N=1), dict(N=8192, Kg=1),    # (Kg + 1) * N > 8192
           dict(ids_u8=2), dict(ids_u8=1, N=300, Kg=6), dict(map_bstride=-1), dict(seg=68)]
    for over in bad:
        with pytest.raises(_lib.SdmiError, match='sdmi_seg_tables'):
            _lib.call('sdmi_seg_tables', None, **dict(ok, **over))
        assert b'sdmi_seg_tables' in _lib.lib().sdmi_last_error(), over
    # a table inside the count gate whose LDS copy plus one source row band does not fit: refused as unsupported
    with pytest.raises(_lib.SdmiError, match=r'sdmi_seg_tables failed \(-3\)'):
        _lib.call('sdmi_seg_tables', None, **dict(ok, N=4000, Kg=1, w=64))


@pytest.mark.parametrize('args,want', [((15, 25, 32, 1), True), ((7, 100, 28, 2), True), ((1, 8191, 4, 1), True), ((1, 8192, 4, 1), False),
                                       ((0, 4, 4, 1), False), ((16, 511, 8, 2), True), ((16, 512, 8, 1), False),
                                       ((4000, 1, 64, 1), False), ((4000, 1, 2, 1), True)])
def test_seg_tables_covers_is_the_entry_points_gate(args, want):
    assert MT.seg_tables_covers(*args) is want
