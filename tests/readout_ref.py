"""CPU restatement of the Physion VQA readout (torch only) and shared builders for the PhysionReadout tests.

Restated from the reference's vp_vqa/models/readout.py: all slot pairs in itertools.combinations order (lines 47-50),
linear1 on [s_i | s_j], the aggregate over pairs, linear2, the max over time (lines 56-79), BCE-with-logits (81-87) and
the thresholded accuracies (89-101).  Two forms of the same function: `forward_pairs` gathers the pairs as the
reference does; `forward_uv` uses linear1([s_i | s_j]) = W_a s_i + W_b s_j + b1 and never builds the pair tensor -- the
form the kernels compute.  Both work in the dtype of their inputs (fp32 like the reference, fp64 as the yardstick)."""
import gzip
import itertools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from slotdiffusion_amd import compat
from tests.detfill import det_fill_

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
AGGS = ('max', 'sum', 'mean')
KEYS = ('linear1.weight', 'linear1.bias', 'linear2.weight', 'linear2.bias')


def pairs(N):
    c = list(itertools.combinations(range(N), 2))
    return torch.tensor([a for a, _ in c]), torch.tensor([b for _, b in c])


def _agg(rel, agg):
    return rel.sum(2) if agg == 'sum' else (rel.mean(2) if agg == 'mean' else rel.max(2)[0])


def relation_pairs(W, slots):
    """[B, T, N, C] -> linear1 on every gathered pair, [B, T, P, F] (readout.py:58-66)."""
    B, T, N, C = slots.shape
    comb_idx = torch.tensor(list(itertools.combinations(range(N), 2))).long().flatten()
    x = slots.flatten(0, 1)[:, comb_idx].unflatten(1, (-1, 2)).flatten(2, 3).unflatten(0, (B, -1))
    return F.linear(x, W['linear1.weight'], W['linear1.bias'])


def relation_uv(W, slots):
    """The same [B, T, P, F] from U = S W_a^T, V = S W_b^T."""
    C = slots.shape[-1]
    w1 = W['linear1.weight']
    U, V = slots @ w1[:, :C].t(), slots @ w1[:, C:].t()
    i, j = pairs(slots.shape[2])
    return U[:, :, i] + V[:, :, j] + W['linear1.bias']


def frame_logits(W, slots, agg, form='pairs'):
    rel = relation_pairs(W, slots) if form == 'pairs' else relation_uv(W, slots)
    return F.linear(_agg(rel, agg), W['linear2.weight'], W['linear2.bias']).squeeze(-1)         # [B, T]


def forward_pairs(W, slots, agg):
    return frame_logits(W, slots, agg, 'pairs').max(1)[0]


def forward_uv(W, slots, agg):
    """Without the [B, T, P, F] tensor: max via a running prefix max of U, sum / mean via the fixed weights."""
    B, T, N, C = slots.shape
    w1 = W['linear1.weight']
    U, V = slots @ w1[:, :C].t(), slots @ w1[:, C:].t()                  # [B, T, N, F]
    P = N * (N - 1) // 2
    if agg == 'max':
        pm = torch.cummax(U, 2)[0]
        m = (pm[:, :, :-1] + V[:, :, 1:]).max(2)[0] + W['linear1.bias']
    else:
        wu = torch.arange(N - 1, -1, -1, dtype=U.dtype).view(1, 1, N, 1)
        wv = torch.arange(N, dtype=U.dtype).view(1, 1, N, 1)
        m = (wu * U).sum(2) + (wv * V).sum(2) + P * W['linear1.bias']
        m = m / P if agg == 'mean' else m
    return F.linear(m, W['linear2.weight'], W['linear2.bias']).squeeze(-1).max(1)[0]


def vqa_loss(logits, label):
    return F.binary_cross_entropy_with_logits(logits.flatten(), label.flatten().type_as(logits))


def eval_metrics(logits, label):
    """readout.py:89-101."""
    pred = logits.flatten()
    gt = label.flatten().type_as(pred)
    ret = {'vqa_loss': vqa_loss(pred, gt)}
    probs = torch.sigmoid(pred)
    for thresh in np.arange(0.1, 1, 0.2):
        ret[f'acc_{thresh:.2f}'] = (probs > thresh).eq(gt).float().mean()
    return ret


def grads(W, slots, label, agg, dlogit=None):
    """Autograd of the pair-gather form: the four parameter gradients of the loss (or of <dlogit, logits>)."""
    Wg = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    logits = forward_pairs(Wg, slots, agg)
    obj = vqa_loss(logits, label) if dlogit is None else (logits * dlogit).sum()
    g = torch.autograd.grad(obj, [Wg[k] for k in KEYS])
    return dict(zip(KEYS, g))


def gaps(W, slots, agg):
    """fp64: (smallest top-two gap of the max over time over the samples, smallest top-two gap of the max over pairs
    over the features of every sample's winning frame -- inf unless agg is max or there is one pair / one frame)."""
    W = {k: v.double() for k, v in W.items()}
    slots = slots.double()
    fr = frame_logits(W, slots, agg)
    tgap = float('inf')
    if fr.shape[1] > 1:
        top = fr.topk(2, dim=1)[0]
        tgap = float((top[:, 0] - top[:, 1]).min())
    pgap = float('inf')
    if agg == 'max' and slots.shape[2] > 2:
        rel = relation_pairs(W, slots)
        win = rel[torch.arange(fr.shape[0]), fr.argmax(1)]               # [B, P, F]
        top = win.topk(2, dim=1)[0]
        pgap = float((top[:, 0] - top[:, 1]).min())
    return tgap, pgap


def gapped_slots(W, shape, agg, seed, tmin=1e-3, pmin=1e-4, tries=200):
    """Seeded randn slots of `shape` for which the gap condition holds (searching seeds upward)."""
    for s in range(seed, seed + tries):
        slots = torch.randn(shape, generator=torch.Generator().manual_seed(s))
        t, p = gaps(W, slots, agg)
        if t >= tmin and p >= pmin:
            return slots
    raise AssertionError(f'no seed in [{seed}, {seed + tries}) meets the gap condition at {shape} / {agg}')


def det_weights(N, C, Fd):
    """Weights of a readout of this geometry, det-filled by state-dict position (comb_idx is position 0)."""
    shapes = [('comb_idx', (N * (N - 1),)), ('linear1.weight', (Fd, 2 * C)), ('linear1.bias', (Fd,)),
              ('linear2.weight', (1, Fd)), ('linear2.bias', (1,))]
    ts = [(n, torch.zeros(s)) for n, s in shapes]
    det_fill_(ts, skip=lambda n: n == 'comb_idx')
    return {n: t for n, t in ts if n != 'comb_idx'}


def shipped_values():
    return json.load(open(os.path.join(GOLD, 'vp_vqa', 'readout_physion_params.json')))


def shipped_params(**over):
    """Params of the shipped config (values dumped by tools/dump_ref_configs.py); over: readout_dict / top-level items."""
    d = shipped_values()
    for k, v in over.items():
        if k in d['readout_dict']:
            d['readout_dict'][k] = v
        else:
            d[k] = v
    return compat.Params(**d)


def key_fixture():
    with gzip.open(os.path.join(GOLD, 'vp_vqa', 'readout_keys.json.gz'), 'rt') as f:
        return json.load(f)


def build(**over):
    """PhysionReadout of the shipped config through the registry, det-filled like the fixture's reference model."""
    import importlib
    m = importlib.import_module('slotdiffusion.vp_vqa').build_model(shipped_params(**over))
    det_fill_(m.state_dict().items(), skip=lambda n: n == 'comb_idx')
    m.invalidate_weights()
    return m


def weights_of(m):
    return {k: v.detach().float().cpu().clone() for k, v in m.state_dict().items() if k != 'comb_idx'}
