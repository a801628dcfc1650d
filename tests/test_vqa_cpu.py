"""The Physion VQA test stage on the CPU: logit_cuts, PhysionVQATestSet on a synthetic slots file + CSV + splits, and
evaluate_physion_vqa's composed stage (checkpoints as a file, a directory, state dicts) against the numpy restatement of
the reference's loops (tests/vqa_ref.py): table, fp32 accuracies, the selection rule with ties, the report, nan for an
empty task, and the model's own weights untouched."""
import json
import math
import warnings

import numpy as np
import pytest
import torch

from slotdiffusion_amd import extract, kern, policy
from slotdiffusion_amd.vp_vqa import (PhysionVQATestSet, ReadoutBank, evaluate_physion_vqa, format_report, logit_cuts)
from slotdiffusion_amd.vqa import DEFAULT_THRESHS
from tests import readout_ref as R
from tests import vqa_ref as V

N, C, F, T = 4, 32, 32, 5


# ------------------------------------------------------------------------------------------
# logit_cuts
# ------------------------------------------------------------------------------------------
def test_logit_cuts_values_and_refusals():
    ts = list(DEFAULT_THRESHS) + [0.05, 0.95, 1e-6, 0.999999]
    cuts = logit_cuts(ts)
    assert cuts.dtype == torch.float32 and tuple(cuts.shape) == (len(ts),)
    for t, c in zip(ts, cuts.tolist()):
        t32 = float(np.float32(t))
        want = math.log(t32 / (1.0 - t32))                       # float64 on the float32 threshold
        assert c == float(np.float32(want)), t
    assert float(logit_cuts([0.5])[0]) == 0.0
    for bad in (0.0, 1.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError, match='threshs'):
            logit_cuts([0.5, bad])
    with pytest.raises(ValueError, match='threshs'):
        logit_cuts([])


def test_logit_rule_equals_the_sigmoid_rule_away_from_the_cuts():
    """Over a grid that stays >= 1e-4 from every cut (>= 4.7e-6 in probability for thresholds in [0.05, 0.95], far above
    fp32 sigmoid error) the two rules agree exactly, whatever position a value has in the tensor."""
    cuts = logit_cuts(DEFAULT_THRESHS)
    grid = torch.linspace(-3, 3, 60001, dtype=torch.float64)
    near = torch.cat([c + torch.tensor([-1e-3, -1.0001e-4, 1.0001e-4, 1e-3], dtype=torch.float64) for c in cuts.double()])
    x = torch.cat([grid, near])
    x = x[((x[:, None] - cuts.double()[None, :]).abs() >= 1e-4).all(1)].float()
    assert ((x.double()[:, None] - cuts.double()[None, :]).abs() >= 0.99e-4).all() and x.numel() > 59000
    p = torch.sigmoid(x)
    for t, c in zip(DEFAULT_THRESHS, cuts):
        assert torch.equal(x > c, p > float(np.float32(t))), t
        assert np.array_equal(V.rule_logit(x.numpy(), t), V.rule_sigmoid(x.numpy(), t)), t


# ------------------------------------------------------------------------------------------
# PhysionVQATestSet
# ------------------------------------------------------------------------------------------
SPLITS = {'Roll': ['pilot_roll_0-redyellow.mp4', 'pilot_roll_1.mp4', 'pilot_roll_bad_2.mp4'],
          'Collide': ['pilot_collide_0.mp4', 'pilot_collide-redyellow_7.mp4', 'pilot_collide_1.mp4'],
          'Drop': ['pilot_drop_0.mp4', 'pilot_drop_1.mp4'],
          'Link': ['pilot_link_bad_0.mp4']}
BAD = ['roll_bad', 'pilot_collide_7', 'link_bad']         # the second one matches only with '-redyellow' removed
KEPT = ['pilot_roll_0-redyellow', 'pilot_roll_1', 'pilot_collide_0', 'pilot_collide_1', 'pilot_drop_0', 'pilot_drop_1']
ALL_TASKS = ['Collide', 'Drop', 'Link', 'Roll']


def _names(splits=SPLITS):
    return [f[:-4] for fs in splits.values() for f in fs]


def _slots(names, seed=0, frames=T):
    g = torch.Generator().manual_seed(seed)
    return {n: torch.randn((frames, N, C), generator=g).numpy() for n in names}


def _write(tmp_path, slots, labels, split='test'):
    pkl, csv = str(tmp_path / 'test_slots.pkl'), str(tmp_path / 'labels.csv')
    extract.dump_slots(pkl, {split: (list(slots), list(slots.values()))})
    with open(csv, 'w') as f:
        f.write(',stimulus,ground truth outcome\n')
        for k, v in labels.items():
            f.write(f'{k},x,{v}\n')
    return pkl, csv


def _labels(names, values=None):
    return {n.replace('-redyellow', ''): (values[i] if values else ('True' if i % 2 else 'False'))
            for i, n in enumerate(names)}


def test_testset_order_keys_filter_and_task_modes(tmp_path):
    names = _names()
    slots = _slots(names)
    pkl, csv = _write(tmp_path, slots, _labels(names))
    ds = PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS, bad_stimuli=BAD)
    assert ds.all_tasks == ALL_TASKS and ds.files == KEPT and len(ds) == 6 and ds.num_removed == 3
    assert ds.task_idx == [3, 3, 0, 0, 1, 1]                   # every kept file under its own task
    assert ds.labels == [float(names.index(n) % 2) for n in KEPT]
    for n, v in zip(KEPT, ds.videos):
        assert tuple(v.shape) == (4, N, C) and np.array_equal(v.numpy(), slots[n][:4])
    # the reference as written: position i of the filtered list reads the task of position i of the unfiltered list
    ref = PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS, bad_stimuli=BAD, task_index='reference')
    assert ref.files == KEPT and ref.task_idx == [3, 3, 3, 0, 0, 0] and ref.labels == ds.labels
    # the two files as paths
    sp, bp = tmp_path / 'test_test.json', tmp_path / 'bad_stimuli.txt'
    sp.write_text(json.dumps(SPLITS))
    bp.write_text('\n'.join(BAD) + '\n\n')
    again = PhysionVQATestSet(pkl, csv, video_len=4, splits=str(sp), bad_stimuli=str(bp))
    assert again.files == ds.files and again.task_idx == ds.task_idx and again.all_tasks == ds.all_tasks
    # no filter: the modes agree
    a = PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS)
    b = PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS, task_index='reference')
    assert a.files == names and a.task_idx == b.task_idx == [3, 3, 3, 0, 0, 0, 1, 1, 2]


def test_testset_without_splits_and_ragged_batches(tmp_path):
    names = ['b_vid-redyellow.mp4', 'a_vid.mp4', 'c_vid.mp4', 'd_bad.mp4', 'e_vid.mp4']
    slots = _slots(names, seed=1)
    pkl, csv = _write(tmp_path, slots, {'b_vid': 'True', 'a_vid': 'False', 'c_vid': '1', 'e_vid': '0', 'd_bad': 'True'})
    ds = PhysionVQATestSet(pkl, csv, video_len=T, bad_stimuli=['d_bad'])
    assert ds.all_tasks == ['all'] and ds.files == ['a_vid.mp4', 'b_vid-redyellow.mp4', 'c_vid.mp4', 'e_vid.mp4']
    assert ds.task_idx == [0, 0, 0, 0] and ds.labels == [0.0, 1.0, 1.0, 0.0]
    bs = list(ds.batches(3))
    assert [tuple(b['slots'].shape) for b in bs] == [(3, T, N, C), (1, T, N, C)]
    assert set(bs[0]) == {'slots', 'label', 'task_idx'}
    assert bs[0]['slots'].dtype == torch.float32 and bs[0]['label'].dtype == torch.float32
    assert bs[0]['task_idx'].dtype == torch.int64
    assert torch.equal(torch.cat([b['label'] for b in bs]), torch.tensor(ds.labels))
    assert np.array_equal(bs[1]['slots'][0].numpy(), slots['e_vid.mp4'])
    with pytest.raises(ValueError, match='batch_size'):
        list(ds.batches(0))


def test_testset_raises_by_name(tmp_path):
    names = _names()
    slots = _slots(names)
    labels = _labels(names)
    pkl, csv = _write(tmp_path, slots, labels)
    with pytest.raises(ValueError, match='task_index'):
        PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS, task_index='task')
    with pytest.raises(KeyError, match='val'):
        PhysionVQATestSet(pkl, csv, video_len=4, split='val', splits=SPLITS)
    with pytest.raises(ValueError, match=r'pilot_roll_0-redyellow.*5 frames'):
        PhysionVQATestSet(pkl, csv, video_len=6, splits=SPLITS)
    with pytest.raises(ValueError, match='no videos'):
        PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS, bad_stimuli=['pilot'])
    more = dict(SPLITS, Drop=SPLITS['Drop'] + ['pilot_drop_9.mp4'])
    with pytest.raises(KeyError, match='no slots for .*pilot_drop_9'):
        PhysionVQATestSet(pkl, csv, video_len=4, splits=more)
    pkl2, csv2 = _write(tmp_path, slots, {k: v for k, v in labels.items() if k != 'pilot_drop_1'})
    with pytest.raises(KeyError, match='no label for .*pilot_drop_1'):
        PhysionVQATestSet(pkl2, csv2, video_len=4, splits=SPLITS)


# ------------------------------------------------------------------------------------------
# evaluate_physion_vqa, composed stage
# ------------------------------------------------------------------------------------------
def _checkpoints(model, n):
    """n distinct state dicts of the model's geometry: linear1's feature axis rolled against linear2's (rolling both
    would permute the features and leave the function as it was) and everything scaled, per checkpoint."""
    base = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out = []
    for i in range(n):
        sd = dict(base)
        for k in R.KEYS:
            v = base[k]
            sd[k] = (torch.roll(v, 3 * i, 0) if k.startswith('linear1') else v) * (1.0 + 0.25 * i)
        out.append(sd)
    return out


def _case(tmp_path, agg='max', dup=True):
    """Test set + checkpoints with a planted winner: the labels are checkpoint 1's decisions at threshold 0.5, and
    checkpoint 2 is a copy of checkpoint 1."""
    model = R.build(num_slots=N, slot_size=C, feats_dim=F, agg_func=agg)
    names = _names()
    slots = _slots(names, seed=7)
    cks = _checkpoints(model, 2)
    if dup:
        cks.append({k: v.clone() for k, v in cks[1].items()})
    x = torch.stack([torch.from_numpy(slots[n][:4]) for n in names])
    W1 = {k: cks[1][k].double() for k in R.KEYS}
    plant = R.forward_pairs(W1, x.double(), agg)
    labels = _labels(names, ['True' if v > 0 else 'False' for v in plant.tolist()])
    pkl, csv = _write(tmp_path, slots, labels)
    ds = PhysionVQATestSet(pkl, csv, video_len=4, splits=SPLITS, bad_stimuli=BAD)
    return model, ds, cks


def _check_against_ref(res, ds, threshs):
    lg = res['logits']
    cuts = logit_cuts(threshs).numpy()
    assert np.abs(lg[:, :, None] - cuts[None, None, :]).min() >= 1e-4              # no decision hangs on an ulp
    J = len(ds.all_tasks)
    want = V.table(lg, ds.labels, ds.task_idx, J, cuts)
    assert res['table'].dtype == np.int64 and np.array_equal(res['table'], want)
    assert np.array_equal(res['task_total'], np.bincount(ds.task_idx, minlength=J))
    assert res['acc'].dtype == np.float32 and res['task_acc'].dtype == np.float32
    for w in range(lg.shape[0]):
        for k, t in enumerate(threshs):
            a, ta = V.score_one(lg[w], ds.labels, ds.task_idx, ds.all_tasks, t, V.rule_logit)
            assert res['acc'][w, k] == a
            for j, task in enumerate(ds.all_tasks):
                assert res['task_acc'][w, k, j] == ta[task] or (np.isnan(ta[task]) and np.isnan(res['task_acc'][w, k, j]))
    ref = V.sweep(lg, res['weights'], ds.labels, ds.task_idx, ds.all_tasks, list(threshs))
    assert res['thresh'] == ref['thresh'] and res['weight'] == ref['weight'] and res['best_acc'] == ref['acc']
    assert list(res['best_task_acc']) == list(ref['task_acc'])
    assert format_report(res) == ref['lines']
    return ref


@pytest.mark.parametrize('agg', R.AGGS)
def test_evaluate_composed_against_the_reference_loops(tmp_path, agg):
    model, ds, cks = _case(tmp_path, agg)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    threshs = (0.05, 0.5, 0.5, 0.95)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                           # the empty task 'Link' gives nan without a warning
        res = evaluate_physion_vqa(model, ds, cks, threshs=threshs, batch_size=4, return_logits=True)
    assert res['fused'] is False and res['logits'].shape == (3, 6) and res['table'].shape == (3, 4, 4)
    # the logits are the readout's (fp64 restatement of the reference)
    x = torch.stack(ds.videos).double()
    for w, sd in enumerate(cks):
        want = R.forward_pairs({k: sd[k].double() for k in R.KEYS}, x, agg)
        assert float((torch.from_numpy(res['logits'][w]).double() - want).abs().max()) <= 1e-5
    _check_against_ref(res, ds, threshs)
    # the planted winner: checkpoints 1 and 2 are perfect at thresholds 1 and 2 -- the first of each wins
    assert res['acc'][1, 1] == res['acc'][2, 1] == res['acc'][1, 2] == 1.0 and res['acc'][0].max() < 1.0
    assert res['acc'][:, 0].max() < 1.0
    assert (res['k_index'], res['w_index']) == (1, 1) and res['weight'] == 'state_dict[1]' and res['thresh'] == 0.5
    # an empty task ('Link': its only file is a bad stimulus)
    j = ds.all_tasks.index('Link')
    assert res['task_total'][j] == 0 and np.isnan(res['task_acc'][:, :, j]).all() and (res['table'][:, :, j] == 0).all()
    assert np.isnan(res['best_task_acc']['Link']) and 'Link: nan' in format_report(res)
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_evaluate_takes_a_file_a_directory_state_dicts_and_a_bank(tmp_path):
    model, ds, cks = _case(tmp_path, 'max', dup=False)
    d = tmp_path / 'models'
    d.mkdir()
    # sorted as strings, as the reference lists them: model_10 before model_2
    torch.save({'state_dict': cks[0], 'it': 3}, str(d / 'model_2.pth'))
    torch.save(cks[1], str(d / 'model_10.pth'))
    (d / 'notes.txt').write_text('not a checkpoint')
    by_dir = evaluate_physion_vqa(model, ds, str(d), batch_size=4, return_logits=True)
    assert by_dir['weights'] == [str(d / 'model_10.pth'), str(d / 'model_2.pth')]
    by_sd = evaluate_physion_vqa(model, ds, [cks[1], {'state_dict': cks[0]}], batch_size=5, return_logits=True)
    assert by_sd['weights'] == ['state_dict[0]', 'state_dict[1]']
    assert np.array_equal(by_dir['table'], by_sd['table'])
    assert float(np.abs(by_dir['logits'] - by_sd['logits']).max()) <= 1e-5       # (another batch size, another GEMM shape)
    one = evaluate_physion_vqa(model, ds, str(d / 'model_2.pth'), batch_size=4, return_logits=True)
    assert one['weights'] == [str(d / 'model_2.pth')] and np.array_equal(one['logits'][0], by_dir['logits'][1])
    assert np.array_equal(one['table'][0], by_dir['table'][1]) and one['weight'] == str(d / 'model_2.pth')
    _check_against_ref(by_dir, ds, DEFAULT_THRESHS)
    mixed = evaluate_physion_vqa(model, ds, [str(d / 'model_2.pth'), cks[1]], batch_size=4)
    assert mixed['weights'] == [str(d / 'model_2.pth'), 'state_dict[1]'] and 'logits' not in mixed
    bank = ReadoutBank.from_weights(model, str(d))
    assert len(bank) == 2 and bank.dtype == model.compute_dtype
    assert np.array_equal(evaluate_physion_vqa(model, ds, bank, batch_size=4)['table'], by_dir['table'])
    with pytest.raises(ValueError, match='no \\*.pth'):
        ReadoutBank.from_weights(model, str(tmp_path))
    with pytest.raises(FileNotFoundError, match='weights'):
        ReadoutBank.from_weights(model, str(d / 'missing.pth'))
    with pytest.raises(KeyError, match="linear1.bias"):
        ReadoutBank.from_weights(model, [{k: v for k, v in cks[0].items() if k != 'linear1.bias'}])
    with pytest.raises(ValueError, match='linear1.weight'):
        ReadoutBank.from_weights(model, [dict(cks[0], **{'linear1.weight': torch.zeros(F, C)})])
    with pytest.raises(ValueError, match='threshs'):
        evaluate_physion_vqa(model, ds, cks, threshs=(0.5, 1.0))


def test_the_flag_is_a_module_switch_not_a_policy_row():
    assert kern._VQA_FUSED is True and not any('VQA' in k for k in policy.SWITCHES)
    assert kern.vqa_score_covers(8, 192, 192, 50, 6, 8) and kern.vqa_score_covers(2, 32, 32, 1, 1, 1)
    assert kern.vqa_score_covers(16, 256, 256, 1, 32, 64)
    assert not kern.vqa_score_covers(8, 192, 192, 1, 33, 8) and not kern.vqa_score_covers(8, 192, 192, 1, 6, 65)
    assert not kern.vqa_score_covers(8, 48, 192, 1, 6, 8) and not kern.vqa_score_covers(8, 192, 192, 0, 6, 8)
