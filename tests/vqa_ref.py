"""Numpy restatement of the reference's Physion VQA test script (vp_vqa/test_physion_vqa.py), written independently of
slotdiffusion_amd/vqa.py: `_calc_acc` (lines 17-19), the per-weight `test()` (22-50), `main()` over the weights of one
threshold (53-85) and the loop over thresholds with the printed report (110-127) -- in the reference's loop order, on
logits that are given (the readout itself is restated in tests/readout_ref.py).  The decision rule is a parameter:
`rule_sigmoid` is the reference's `sigmoid(logit) > thresh` on float32 values, `rule_logit` the stage's
`logit > float32(log(t / (1 - t)))`."""
import warnings

import numpy as np


def rule_sigmoid(logits, thresh):
    x = np.asarray(logits, dtype=np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32))) > np.float32(thresh)


def rule_logit(logits, thresh):
    t = np.float64(np.float32(thresh))
    return np.asarray(logits, dtype=np.float32) > np.float32(np.log(t / (1.0 - t)))


def calc_acc(decision, gt):
    """_calc_acc: mean over float32 zeros and ones (nan for no sample, without numpy's warning)."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return (decision.astype(np.float32) == gt).astype(np.float32).mean()


def score_one(logits, gt, task_idx, all_tasks, thresh, rule):
    """test(): one weight at one threshold -> (all_acc, {task: acc})."""
    gt = np.asarray(gt, dtype=np.float32)
    task_idx = np.asarray(task_idx)
    dec = rule(logits, thresh)
    task_acc = {}
    for i, task in enumerate(all_tasks):
        sel = task_idx == i
        task_acc[task] = calc_acc(dec[sel], gt[sel])
    return calc_acc(dec, gt), task_acc


def main_one(all_logits, names, gt, task_idx, all_tasks, thresh, rule):
    """main(): every weight at one threshold, the first best one wins -> (name, acc, task_acc)."""
    accs, taccs = [], []
    for row in all_logits:
        a, t = score_one(row, gt, task_idx, all_tasks, thresh, rule)
        accs.append(a)
        taccs.append(t)
    idx = int(np.argmax(accs))
    return names[idx], accs[idx], taccs[idx]


def sweep(all_logits, names, gt, task_idx, all_tasks, threshs, rule=rule_logit):
    """The __main__ loop: -> dict(thresh, weight, acc, task_acc, lines)."""
    ws, accs, taccs = [], [], []
    for thresh in threshs:
        w, a, t = main_one(all_logits, names, gt, task_idx, all_tasks, thresh, rule)
        ws.append(w)
        accs.append(a)
        taccs.append(t)
    idx = int(np.argmax(accs))
    w, acc, task_acc = ws[idx], accs[idx], taccs[idx]
    lines = [f'Threshold {threshs[idx % len(threshs)]}, {w} achieves the best accuracy', f'All accuracy: {acc:.3f}']
    lines += [f'{task}: {a:.3f}' for task, a in task_acc.items()]
    return dict(thresh=threshs[idx], weight=w, acc=acc, task_acc=task_acc, lines=lines)


def table(all_logits, gt, task_idx, num_tasks, cuts):
    """Integer counts [W, K, J] of (logit > cut) == (gt != 0), from explicit loops."""
    all_logits = np.asarray(all_logits, dtype=np.float32)
    out = np.zeros((all_logits.shape[0], len(cuts), num_tasks), dtype=np.int64)
    for w in range(all_logits.shape[0]):
        for k, c in enumerate(cuts):
            for v in range(all_logits.shape[1]):
                if bool(all_logits[w, v] > np.float32(c)) == bool(gt[v] != 0):
                    out[w, k, int(task_idx[v])] += 1
    return out
