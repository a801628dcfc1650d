"""The Physion VQA test stage on the GPU (slotdiffusion_amd/vqa.py): the fused stage (one sdmi_vqa_score call per batch
of videos for all checkpoints and thresholds) against the composed one (per checkpoint, the model's own forward) --
exactly, in table, accuracies, selection and report -- the call counts, the geometries and the switch that take the
composed stage, the model's weights left alone, and the documented end of the chain from a rollout file."""
import numpy as np
import pytest
import torch

from slotdiffusion_amd import extract, kern, ops, unroll
from slotdiffusion_amd.method import Method
from slotdiffusion_amd.vp_vqa import PhysionVQATestSet, evaluate_physion_vqa, format_report, logit_cuts
from tests import readout_ref as R
from tests import vqa_ref as V

pytestmark = pytest.mark.gpu

T = 6
SPLITS = {'Roll': [f'pilot_roll_{i}.mp4' for i in range(3)] + ['pilot_roll_bad_3.mp4'],
          'Dominoes': ['pilot_dominoes_0-redyellow.mp4'] + [f'pilot_dominoes_{i}.mp4' for i in range(1, 4)],
          'Contain': [f'pilot_contain_{i}.mp4' for i in range(4)]}
BAD = ['roll_bad']


def _model(dtype, **over):
    m = R.build(agg_func='max', **over).cuda()
    m.set_compute_dtype(dtype)
    return m.eval()


def _state_dicts(model, n):
    base = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return [{k: ((torch.roll(v, 7 * i, 0) if k.startswith('linear1') else v) * (1.0 + 0.25 * i) if k in R.KEYS else v)
             for k, v in base.items()} for i in range(n)]


def _testset(tmp_path, C=192, seed=3):
    names = [f[:-4] for fs in SPLITS.values() for f in fs]
    g = torch.Generator().manual_seed(seed)
    slots = {n: torch.randn((T + 1, 8, C), generator=g).numpy() for n in names}
    pkl, csv = str(tmp_path / 'test_slots.pkl'), str(tmp_path / 'labels.csv')
    extract.dump_slots(pkl, {'test': (list(slots), list(slots.values()))})
    with open(csv, 'w') as f:
        f.write(',stimulus,ground truth outcome\n')
        for i, n in enumerate(names):
            f.write(f"{n.replace('-redyellow', '')},x,{'True' if (i * 5) % 3 else 'False'}\n")
    return PhysionVQATestSet(pkl, csv, video_len=T, splits=SPLITS, bad_stimuli=BAD)


def _weights(tmp_path, model, over=None):
    """Three checkpoints written by Method.save into a directory, plus one raw state dict."""
    sds = _state_dicts(model, 4)
    d = tmp_path / 'models'
    d.mkdir()
    scratch = R.build(agg_func='max', **(over or {})).cuda()
    for i in range(3):
        scratch.load_state_dict(sds[i])
        Method(scratch, None, R.shipped_params()).save(str(d / f'model_{i}.pth'))
    return [str(d / f'model_{i}.pth') for i in range(3)] + [sds[3]]


def _spy(fn):
    seen = {'vqa_score': 0, 'readout_fwd': 0}
    orig = ops.vqa_score, ops.readout_fwd

    def wrap(name, f):
        def g(*a, **k):
            seen[name] += 1
            return f(*a, **k)
        return g
    ops.vqa_score, ops.readout_fwd = wrap('vqa_score', orig[0]), wrap('readout_fwd', orig[1])
    try:
        out = fn()
    finally:
        ops.vqa_score, ops.readout_fwd = orig
    return out, seen


def _same(a, b):
    assert np.array_equal(a['table'], b['table']) and np.array_equal(a['task_total'], b['task_total'])
    assert np.array_equal(a['acc'], b['acc']) and np.array_equal(a['task_acc'], b['task_acc'], equal_nan=True)
    assert np.array_equal(a['logits'], b['logits'])
    for k in ('k_index', 'w_index', 'thresh', 'weight', 'best_acc', 'weights', 'threshs', 'tasks'):
        assert a[k] == b[k], k
    assert format_report(a) == format_report(b)


def _matches_ref(res, ds):
    cuts = logit_cuts(res['threshs']).numpy()
    want = V.table(res['logits'], ds.labels, ds.task_idx, len(ds.all_tasks), cuts)
    assert np.array_equal(res['table'], want)
    ref = V.sweep(res['logits'], res['weights'], ds.labels, ds.task_idx, ds.all_tasks, res['threshs'])
    assert res['thresh'] == ref['thresh'] and res['weight'] == ref['weight'] and res['best_acc'] == ref['acc']
    assert format_report(res) == ref['lines']


@pytest.mark.parametrize('dtype', ['fp32', 'bf16'])
def test_fused_stage_equals_the_composed_stage(tmp_path, dtype):
    model = _model(dtype)
    ds = _testset(tmp_path)
    assert len(ds) == 11 and ds.num_removed == 1 and ds.all_tasks == ['Contain', 'Dominoes', 'Roll']
    weights = _weights(tmp_path, model)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    x = torch.stack(ds.videos[:2]).cuda()
    own = model({'slots': x})['logits'].clone()
    fused, seen = _spy(lambda: evaluate_physion_vqa(model, ds, weights, batch_size=4, return_logits=True))
    assert fused['fused'] is True and seen == {'vqa_score': 3, 'readout_fwd': 0}          # batches of 4, 4 and 3
    assert fused['table'].shape == (4, 6, 3) and fused['logits'].shape == (4, 11)
    assert fused['weights'] == weights[:3] + ['state_dict[3]']
    comp, seen = _spy(lambda: evaluate_physion_vqa(model, ds, weights, batch_size=4, fused=False, return_logits=True))
    assert comp['fused'] is False and seen == {'vqa_score': 0, 'readout_fwd': 12}
    _same(fused, comp)
    _matches_ref(fused, ds)
    assert len(np.unique(fused['logits'], axis=0)) == 4                                   # four different checkpoints
    kern._VQA_FUSED = False
    try:
        off, seen = _spy(lambda: evaluate_physion_vqa(model, ds, weights, batch_size=4, return_logits=True))
    finally:
        kern._VQA_FUSED = True
    assert off['fused'] is False and seen == {'vqa_score': 0, 'readout_fwd': 12}
    _same(fused, off)
    after = model.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)
    assert torch.equal(model({'slots': x})['logits'], own)                               # and it computes with them


def test_an_uncovered_geometry_runs_composed(tmp_path):
    over = dict(slot_size=48)
    model = _model('fp32', **over)
    ds = _testset(tmp_path, C=48)
    weights = _weights(tmp_path, model, over)
    res, seen = _spy(lambda: evaluate_physion_vqa(model, ds, weights, batch_size=4, fused=True, return_logits=True))
    assert res['fused'] is False and seen == {'vqa_score': 0, 'readout_fwd': 0}           # engine.readout_composed
    _matches_ref(res, ds)
    assert len(np.unique(res['logits'], axis=0)) == 4                                     # every checkpoint was loaded
    # more thresholds than the kernel takes: composed as well
    m192 = _model('fp32')
    ds192 = _testset(tmp_path)
    many = [float(t) for t in np.linspace(0.1, 0.9, 33)]
    res, seen = _spy(lambda: evaluate_physion_vqa(m192, ds192, _state_dicts(m192, 2), threshs=many, batch_size=4,
                                                  return_logits=True))
    assert res['fused'] is False and seen == {'vqa_score': 0, 'readout_fwd': 6} and res['table'].shape == (2, 33, 3)
    _matches_ref(res, ds192)


def test_from_a_rollout_file_to_the_vqa_table(tmp_path):
    """The documented end of the chain: unroll.rollout_slots_file -> PhysionVQATestSet -> evaluate_physion_vqa."""
    from tests import slotformer_ref as SF
    sf = SF.gpu_model(decoder=False)
    g = torch.Generator().manual_seed(21)
    names = ['pilot_towers_1-redyellow_img.mp4', 'pilot_towers_0_img.mp4', 'pilot_link_2_img.mp4']
    vids = [torch.randn(20, 8, 192, generator=g).numpy() for _ in names]
    src, dst = str(tmp_path / 'test_slots.pkl'), str(tmp_path / 'rollout_test_slots.pkl')
    extract.dump_slots(src, {'test': (names, vids)})
    unroll.rollout_slots_file(sf, src, dst, ('test',), video_len=19, obs_frames=15, frame_offset=1, batch_size=2)
    csv = str(tmp_path / 'labels.csv')
    with open(csv, 'w') as f:
        f.write(',stimulus,ground truth outcome\npilot_towers_1_img,x,True\npilot_towers_0_img,x,False\n'
                'pilot_link_2_img,x,True\n')
    ds = PhysionVQATestSet(dst, csv, video_len=19)
    assert ds.files == sorted(names) and ds.labels == [1.0, 0.0, 1.0] and ds.all_tasks == ['all']
    assert tuple(ds.videos[0].shape) == (19, 8, 192)
    assert np.array_equal(ds.videos[1][:15].numpy(), vids[1][:15]) and not np.array_equal(ds.videos[1][15:].numpy(), vids[1][15:19])
    model = _model('fp32')
    sds = _state_dicts(model, 2)
    res = evaluate_physion_vqa(model, ds, sds, batch_size=2, return_logits=True)
    assert res['fused'] is True and res['table'].shape == (2, 6, 1)
    _matches_ref(res, ds)
    _same(res, evaluate_physion_vqa(model, ds, sds, batch_size=2, fused=False, return_logits=True))
    x = torch.stack(ds.videos).double()
    for w, sd in enumerate(sds):
        want = R.forward_pairs({k: sd[k].double().cpu() for k in R.KEYS}, x, 'max')
        assert float((torch.from_numpy(res['logits'][w]).double() - want).abs().max()) <= 1e-5
    assert format_report(res)[0].startswith('Threshold ') and format_report(res)[-1].startswith('all: ')
