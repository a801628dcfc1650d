"""The Physion VQA test stage: from a trained readout to "the number we report in the paper" (the reference's
vp_vqa/test_physion_vqa.py and the test subset of vp_vqa/datasets/physion.py: PhysionSlotsLabelDataset).

    testset = PhysionVQATestSet('rollout_test_slots.pkl', 'PhysionTestMP4s/labels.csv', video_len=75,
                                splits='test_test.json', bad_stimuli='bad_stimuli.txt')
    result = evaluate_physion_vqa(model, testset, 'checkpoint/readout/models', batch_size=params.val_batch_size)
    print('\\n'.join(format_report(result)))

The reference reloads every checkpoint of the directory for every threshold and walks the whole test set through the
readout each time: K W passes for one table, although the logits do not depend on the threshold and the slots do not
depend on the checkpoint.  Here the test set is walked ONCE: per batch of videos one sdmi_vqa_score launch scores all W
checkpoints (a ReadoutBank) against all K thresholds and adds the correct decisions to one [W, K, J] integer table.
Outside the kernel's geometry (kern.vqa_score_covers), with fused=False or with kern._VQA_FUSED off, the composed stage
runs instead: per checkpoint the weights are loaded into the model and the test set goes through model.forward (W
passes), and the same decision rule is applied in torch.  CPU tensors take the composed stage with the readout written
in plain torch ops (the reference's arithmetic): the kernels need device tensors.

Decision rule.  The stage decides `logit > cut` with cut = float32(log(t / (1 - t))) (logit_cuts); the reference decides
`float32 sigmoid(logit) > float32(thresh)`.  Both are monotone in the logit and differ only for logits within a few
fp32 ulps of the cut -- where the reference's own answer is not well defined: torch.sigmoid on the CPU gives different
bits for the same value depending on its position in the tensor (the vectorised body and the scalar tail of the loop
are different code), so the same video can fall on either side of a threshold depending on the batch size."""
import json
import os

import numpy as np
import torch

from . import kern, ops
from .extract import load_slots
from .method import physion_label_key, read_physion_labels

__all__ = ['DEFAULT_THRESHS', 'logit_cuts', 'PhysionVQATestSet', 'ReadoutBank', 'evaluate_physion_vqa', 'format_report']

DEFAULT_THRESHS = (0.4, 0.45, 0.5, 0.55, 0.6, 0.65)           # test_physion_vqa.py:93-98


def logit_cuts(threshs):
    """Probability thresholds -> the same thresholds in logit space, fp32 [K]: cut = float32(log(t / (1 - t))) evaluated
    in float64 on t = float32(thresh) (the value the reference compares its float32 probabilities with).  `logit > cut`
    then equals `sigmoid(logit) > t` for every logit that is not within a few fp32 ulps of the cut; there the reference's
    answer depends on where in the batch the video sits (module docstring), this rule's does not.  A threshold outside
    (0, 1) is refused: it has no finite logit."""
    t = np.asarray(list(threshs) if not np.isscalar(threshs) else [threshs], dtype=np.float32).reshape(-1)
    if t.size == 0:
        raise ValueError('threshs: no threshold given')
    for v in t:
        if not 0.0 < float(v) < 1.0:
            raise ValueError(f'threshs: {float(v)!r} is outside (0, 1)')
    t64 = t.astype(np.float64)
    return torch.from_numpy(np.log(t64 / (1.0 - t64)).astype(np.float32))


def _read_lines(path):
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


class PhysionVQATestSet:
    """The reference's PhysionSlotsLabelDataset for subset='test', without images: the stored slots of every test video
    with its label and its task.

    slots_path: a file of extract.dump_slots / unroll.rollout_slots_file ({split: {name: [T, N, C]}}); labels_csv: the
    test subset's labels.csv; video_len: the frames taken from the front of every video.
    splits: {task: ['xxx.mp4', ...]} or a path to such a JSON (the user's copy of splits/Physion/test_test.json).  Files
      are taken task by task in the JSON's key order and in listed order (physion.py:129-143); the slots key is the
      basename without '.mp4' (a file stored under the name with '.mp4' is found too).  `all_tasks` is the sorted task
      names.  Without `splits` there is one task 'all' and every stored video of the split is taken, in sorted order.
    bad_stimuli: a list of strings or a path to the text file (one per line).  A file is dropped when any of them occurs
      in its name with '-redyellow' removed (physion.py:276-285).
    task_index: 'file' gives every kept file the task it is listed under.  'reference' reproduces the reference as
      written: its position -> task map is built before the bad-stimuli filter and is not re-indexed after it
      (physion.py:129-143, 276-285, 349), so file i of the FILTERED list gets the task of file i of the UNFILTERED list.
      The overall accuracy does not depend on the mode; the per-task accuracies do.  The per-task numbers the
      reference prints correspond to 'reference'; 'file' (the default) is what those numbers are meant to be.
    A video without a label, a listed video that is not stored, or one shorter than video_len raises by name."""

    def __init__(self, slots_path, labels_csv, video_len, split='test', splits=None, bad_stimuli=None, task_index='file'):
        if task_index not in ('file', 'reference'):
            raise ValueError(f"task_index={task_index!r}: 'file' or 'reference'")
        data = load_slots(slots_path)
        if split not in data:
            raise KeyError(f'{slots_path}: no split {split!r}')
        data = data[split]
        labels = read_physion_labels(labels_csv)
        if isinstance(splits, (str, os.PathLike)):
            with open(splits) as f:
                splits = json.load(f)
        if isinstance(bad_stimuli, (str, os.PathLike)):
            bad_stimuli = _read_lines(bad_stimuli)
        bad = [s for s in (bad_stimuli or []) if s]
        if splits is None:
            listed = {'all': sorted(data)}
        else:
            listed = {task: [os.path.basename(f)[:-4] if f.endswith('.mp4') else os.path.basename(f) for f in files]
                      for task, files in splits.items()}
        self.all_tasks = sorted(listed)
        self.task2num = {task: len(listed[task]) for task in self.all_tasks}
        unfiltered = [(name, self.all_tasks.index(task)) for task in listed for name in listed[task]]
        kept = [(name, t) for name, t in unfiltered if not any(s in name.replace('-redyellow', '') for s in bad)]
        self.num_removed = len(unfiltered) - len(kept)
        if not kept:
            raise ValueError(f'{slots_path} [{split}]: no videos')
        self.video_len, self.task_index_mode = int(video_len), task_index
        self.files, self.videos, self.labels, self.task_idx = [], [], [], []
        for i, (name, t) in enumerate(kept):
            key = name if name in data or name + '.mp4' not in data else name + '.mp4'
            if key not in data:
                raise KeyError(f'{slots_path} [{split}]: no slots for {name!r}')
            lkey = physion_label_key(name, 'test')
            if lkey not in labels:
                raise KeyError(f'{labels_csv}: no label for {name!r} (key {lkey!r})')
            if data[key].shape[0] < self.video_len:
                raise ValueError(f'{slots_path} [{split}]: {name!r} has {data[key].shape[0]} frames, video_len is '
                                 f'{self.video_len}')
            self.files.append(name)
            self.videos.append(torch.as_tensor(np.asarray(data[key][:self.video_len])).float())
            self.labels.append(float(labels[lkey]))
            self.task_idx.append(t if task_index == 'file' else unfiltered[i][1])

    def __len__(self):
        return len(self.files)

    def batches(self, batch_size):
        """{'slots': [b, video_len, N, C] fp32, 'label': [b] fp32, 'task_idx': [b] int64} in file order (host tensors);
        the last batch is ragged."""
        if batch_size < 1:
            raise ValueError(f'batch_size={batch_size}: must be at least 1')
        for s in range(0, len(self.files), batch_size):
            e = min(s + batch_size, len(self.files))
            yield {'slots': torch.stack(self.videos[s:e]), 'label': torch.tensor(self.labels[s:e], dtype=torch.float32),
                   'task_idx': torch.tensor(self.task_idx[s:e], dtype=torch.int64)}


def _state_dict_of(w):
    if isinstance(w, (str, os.PathLike)):
        w = torch.load(w, map_location='cpu')
    return w.get('state_dict', w)


class ReadoutBank:
    """W checkpoints of one PhysionReadout geometry, stacked: the operands of sdmi_vqa_score.
      w1p [W, F * 2C] in the model's compute dtype, every row packed as sdmi_readout_fwd's w1p (kern.readout_pack_index);
      b1 [W, F], w2 [W, F], b2 [W] fp32;  names [W]: the checkpoint paths (state dicts: 'state_dict[i]').
    The fp32 state dicts are kept on the host for the composed stage."""

    def __init__(self, names, states, dtype, device):
        self.names, self.states, self.dtype, self.device = list(names), list(states), dtype, device
        self._ops = None

    def __len__(self):
        return len(self.names)

    @classmethod
    def from_weights(cls, model, weights):
        """weights: a checkpoint file, a directory (its '*.pth' in sorted order, as the reference lists them), or a list
        of paths / state dicts ({'state_dict': ...} wrappers are accepted, as in load_weight).  The model gives geometry,
        compute dtype and device; its own weights are not touched."""
        if isinstance(weights, (str, os.PathLike)):
            if os.path.isdir(weights):
                items = [os.path.join(weights, w) for w in sorted(os.listdir(weights)) if w.endswith('.pth')]
                if not items:
                    raise ValueError(f'weights: no *.pth in {weights}')
            elif os.path.isfile(weights):
                items = [weights]
            else:
                raise FileNotFoundError(f'weights: {weights} is neither a file nor a directory')
        else:
            items = list(weights)
            if not items:
                raise ValueError('weights: empty list')
        names, states = [], []
        want = {k: tuple(v.shape) for k, v in model.state_dict().items() if k in kern.READOUT_NAMES}
        for i, w in enumerate(items):
            name = os.fspath(w) if isinstance(w, (str, os.PathLike)) else f'state_dict[{i}]'
            sd = _state_dict_of(w)
            st = {}
            for k, shape in want.items():
                if k not in sd:
                    raise KeyError(f'weights: {name} has no {k!r}')
                if tuple(sd[k].shape) != shape:
                    raise ValueError(f'weights: {name}: {k} is {tuple(sd[k].shape)}, the model has {shape}')
                st[k] = sd[k].detach().float().cpu().clone()
            names.append(name)
            states.append(st)
        return cls(names, states, model.compute_dtype, model.device)

    def operands(self):
        """(w1p, b1, w2, b2) on the device, made once."""
        if self._ops is None:
            k1, kb1, k2, kb2 = kern.READOUT_NAMES
            st = lambda k: torch.stack([s[k] for s in self.states]).to(self.device)
            w1 = st(k1)                                             # [W, F, 2C]
            W, F, C2 = w1.shape
            idx = kern.readout_pack_index(C2 // 2, F, self.dtype, w1.device)
            w1p = w1.to(self.dtype).reshape(W, -1)[:, idx].contiguous()
            self._ops = (w1p, st(kb1).contiguous(), st(k2).reshape(W, F).contiguous(), st(kb2).reshape(W).contiguous())
        return self._ops


def _torch_logits(model, slots):
    """PhysionReadout.forward in plain torch ops on the model's fp32 weights (readout.py:56-79), for host tensors."""
    B, T = slots.shape[:2]
    x = slots.float().flatten(0, 1)[:, model.comb_idx].unflatten(1, (-1, 2)).flatten(2, 3)      # [B T, P, 2C]
    rel = torch.nn.functional.linear(x, model.linear1.weight, model.linear1.bias)
    agg = model.agg_func
    m = rel.sum(1) if agg == 'sum' else (rel.mean(1) if agg == 'mean' else rel.max(1)[0])
    fr = torch.nn.functional.linear(m, model.linear2.weight, model.linear2.bias).squeeze(-1)
    return fr.unflatten(0, (B, T)).max(1)[0]


def _composed_logits(model, bank, testset, batch_size):
    """[W, videos] fp32: per checkpoint, the weights loaded into the model and the test set through its forward.  The
    model's own weights are put back afterwards."""
    own = {k: v.detach().clone() for k, v in model.state_dict().items()}
    dev = model.device
    rows = []
    try:
        for st in bank.states:
            model.load_state_dict({**own, **{k: v.to(dev) for k, v in st.items()}})
            out = []
            for batch in testset.batches(batch_size):
                slots = batch['slots'].to(dev)
                out.append(model({'slots': slots})['logits'].float() if slots.is_cuda else _torch_logits(model, slots))
            rows.append(torch.cat(out))
    finally:
        model.load_state_dict(own)
    return torch.stack(rows)


@torch.no_grad()
def evaluate_physion_vqa(model, testset, weights, threshs=DEFAULT_THRESHS, batch_size=None, fused=None,
                         return_logits=False):
    """test_physion_vqa.py in one pass over the test set.  model: a PhysionReadout (geometry, compute dtype, device);
    testset: a PhysionVQATestSet; weights: what ReadoutBank.from_weights takes, or a ReadoutBank; batch_size: pass
    params.val_batch_size (the reference's loader), 128 when None.  fused: None / True = sdmi_vqa_score wherever it
    covers the geometry, False = the composed stage (module docstring).  Returns a dict:
      table [W, K, J] int64: correct decisions of checkpoint w at threshold k among the videos of task j;
      task_total [J] int64;  acc [W, K], task_acc [W, K, J] float32 = float32(correct) / float32(total) -- what the
        reference's `.astype(np.float32).mean()` yields below 2^24 videos; a task without videos gives nan;
      k_index, w_index, thresh, weight, best_acc, best_task_acc {task: acc}: the reference's selection in its loop order,
        k* = first argmax_k max_w acc[w, k], then w* = first argmax_w acc[w, k*];
      weights [W] (names), threshs [K], tasks [J], fused (which stage ran);  logits [W, videos] float32 on request."""
    model.eval()
    bank = weights if isinstance(weights, ReadoutBank) else ReadoutBank.from_weights(model, weights)
    threshs = [float(t) for t in threshs]
    cuts = logit_cuts(threshs)
    batch_size = int(batch_size or 128)
    W, K, J = len(bank), len(threshs), len(testset.all_tasks)
    dev = model.device
    on_gpu = torch.device(dev).type == 'cuda'
    use_fused = (fused is None or bool(fused)) and kern._VQA_FUSED and on_gpu and \
        kern.vqa_score_covers(model.num_slots, model.slot_size, model.feats_dim, W, K, J)
    label = np.asarray(testset.labels, dtype=np.float32)
    task = np.asarray(testset.task_idx, dtype=np.int64)
    if use_fused:
        w1p, b1, w2, b2 = bank.operands()
        cut_d = cuts.to(dev)
        correct = torch.zeros((W, K, J), dtype=torch.int32, device=dev)
        parts = []
        for batch in testset.batches(batch_size):
            lg, _ = ops.vqa_score(batch['slots'].to(dev), w1p, b1, w2, b2, model.agg_func, bank.dtype,
                                  batch['label'].to(dev), batch['task_idx'].to(dev), cut_d, J, correct=correct)
            if return_logits:
                parts.append(lg)
        table = correct.cpu().numpy().astype(np.int64)
        logits = torch.cat(parts, 1).cpu().numpy() if return_logits else None
    else:
        lg = _composed_logits(model, bank, testset, batch_size).cpu()                     # [W, videos]
        ok = (lg[:, None, :] > cuts[None, :, None]) == torch.from_numpy(label != 0)[None, None, :]
        onehot = torch.nn.functional.one_hot(torch.from_numpy(task), J)                   # [videos, J] int64
        table = (ok.to(torch.int64) @ onehot).numpy()
        logits = lg.numpy() if return_logits else None
    task_total = np.bincount(task, minlength=J).astype(np.int64)
    with np.errstate(divide='ignore', invalid='ignore'):
        acc = table.sum(-1).astype(np.float32) / np.float32(len(testset))
        task_acc = table.astype(np.float32) / task_total.astype(np.float32)
    k_star = int(np.argmax(acc.max(0)))
    w_star = int(np.argmax(acc[:, k_star]))
    res = dict(table=table, task_total=task_total, acc=acc, task_acc=task_acc, k_index=k_star, w_index=w_star,
               thresh=threshs[k_star], weight=bank.names[w_star], best_acc=acc[w_star, k_star],
               best_task_acc={t: task_acc[w_star, k_star, j] for j, t in enumerate(testset.all_tasks)},
               weights=list(bank.names), threshs=threshs, tasks=list(testset.all_tasks), fused=bool(use_fused))
    if return_logits:
        res['logits'] = logits
    return res


def format_report(result):
    """The lines test_physion_vqa.py:123-127 prints for this result."""
    lines = [f"Threshold {result['thresh']}, {result['weight']} achieves the best accuracy",
             f"All accuracy: {result['best_acc']:.3f}"]
    return lines + [f'{task}: {acc:.3f}' for task, acc in result['best_task_acc'].items()]
