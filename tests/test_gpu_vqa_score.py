"""sdmi_vqa_score through ops.vqa_score: logits bit-equal to sdmi_readout_fwd's per checkpoint and within the readout's
bar of the fp64 restatement (tests/readout_ref.py), the integer table cell for cell, accumulation, the strict compare,
identical checkpoints, empty tasks, repeatability and the refusals.

Bar on the logits: 1e-5 absolute against fp64 (the TOL of tests/test_gpu_readout.py, whose fp32 case measured 5.8e-6 at
the largest shape); with bf16 operands the fp64 side takes the inputs and linear1.weight rounded to bf16."""
import functools

import numpy as np
import pytest
import torch

from slotdiffusion_amd import _lib, kern, ops
from tests import readout_ref as R

pytestmark = pytest.mark.gpu

# (B, T, N, C, F, W, K, J): every minimum; N = 3 (whole frames do not fill a 32-row chunk); an odd N; the shipped
# dimensions; the shipped T (600 rows per video: many chunks and a tail); every upper bound
SHAPES = [(1, 1, 2, 32, 32, 1, 1, 1), (3, 5, 3, 64, 32, 2, 3, 2), (5, 7, 5, 96, 64, 3, 6, 4), (3, 5, 8, 192, 192, 3, 6, 8),
          (2, 75, 8, 192, 192, 2, 6, 8), (2, 33, 16, 256, 256, 2, 2, 3)]
OPS = [torch.float32, torch.bfloat16]
TOL = 1e-5


def checkpoints(N, C, F, W):
    """W distinct weight sets: det_weights with linear1's feature axis rolled against linear2's (rolling both would
    only permute the features) and everything scaled, per checkpoint."""
    base = R.det_weights(N, C, F)
    return [{k: (torch.roll(v, 5 * w, 0) if k.startswith('linear1') else v) * (1.0 + 0.125 * w) for k, v in base.items()}
            for w in range(W)]


def pack(W, op):
    w1 = W['linear1.weight']
    F, C2 = w1.shape
    idx = kern.readout_pack_index(C2 // 2, F, op, 'cuda')
    return w1.cuda().to(op).reshape(-1)[idx].contiguous()


def bank(Ws, op):
    f = lambda k: torch.stack([W[k].reshape(-1) for W in Ws]).cuda().contiguous()
    return torch.stack([pack(W, op) for W in Ws]).contiguous(), f('linear1.bias'), f('linear2.weight'), f('linear2.bias').reshape(-1)


def score(Ws, slots, agg, op, label, task, cut, J, correct=None):
    w1p, b1, w2, b2 = bank(Ws, op)
    return ops.vqa_score(slots, w1p, b1, w2, b2, agg, op, label.cuda(), task.cuda(), cut.cuda(), J, correct=correct)


def readout_logits(W, slots, agg, op):
    f = lambda k: W[k].cuda().reshape(-1).contiguous()
    return ops.readout_fwd(slots, pack(W, op), f('linear1.bias'), f('linear2.weight'), f('linear2.bias'), agg, op)['logits']


def count(logits, label, task, cut, J):
    """The table in numpy from given logits [W, B]."""
    logits, label, task, cut = (np.asarray(t) for t in (logits, label, task, cut))
    out = np.zeros((logits.shape[0], len(cut), J), dtype=np.int64)
    for w in range(logits.shape[0]):
        for k in range(len(cut)):
            for b in range(logits.shape[1]):
                if bool(logits[w, b] > cut[k]) == bool(label[b] != 0):
                    out[w, k, task[b]] += 1
    return out


@functools.lru_cache(maxsize=None)
def case(shape, agg):
    """Checkpoints, gap-conditioned slots (for checkpoint 0), labels, tasks, cuts and the fp64 logits for fp32 and for
    bf16 operands of one (shape, agg), computed once per session."""
    B, T, N, C, F, W, K, J = shape
    Ws = checkpoints(N, C, F, W)
    slots = R.gapped_slots(Ws[0], (B, T, N, C), agg, seed=100 * B + T)
    ref = {}
    for op in OPS:
        rows = []
        for Wt in Ws:
            W64 = {k: v.double() for k, v in Wt.items()}
            x = slots.double()
            if op == torch.bfloat16:
                W64['linear1.weight'] = Wt['linear1.weight'].bfloat16().double()
                x = slots.bfloat16().double()
            rows.append(R.frame_logits(W64, x, agg).max(1)[0])
        ref[op] = torch.stack(rows)
    lo, hi = float(ref[torch.float32].min()), float(ref[torch.float32].max())
    cut = torch.linspace(lo - 0.5, hi + 0.5, K + 2)[1:-1].float() if K > 1 else torch.tensor([(lo + hi) / 2]).float()
    label = (ref[torch.float32][0] > ref[torch.float32][0].median()).float()
    if B > 1:
        label[0] = 1.0 - label[1]                        # both labels occur
    task = (torch.arange(B) * 3 + 1) % J
    return Ws, slots, label, task.int(), cut, ref


@functools.lru_cache(maxsize=None)
def run(shape, agg, op):
    """One kernel call per (shape, agg, op), shared by the tests below: (logits [W, B], correct [W, K, J]) on the host."""
    Ws, slots, label, task, cut, _ = case(shape, agg)
    lg, tb = score(Ws, slots.cuda(), agg, op, label, task, cut, shape[7])
    torch.cuda.synchronize()
    return lg.cpu(), tb.cpu()


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('agg', R.AGGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_logits_have_the_bits_of_readout_fwd(shape, agg, op):
    Ws, slots, *_ = case(shape, agg)
    lg, _ = run(shape, agg, op)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (shape[5], shape[0])
    for w, W in enumerate(Ws):
        assert torch.equal(lg[w], readout_logits(W, slots.cuda(), agg, op).cpu()), w


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('agg', R.AGGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_logits_against_fp64(shape, agg, op):
    """fp32 operands: against the fp64 restatement.  bf16 operands: against fp64 on inputs and linear1.weight rounded to
    bf16.  Measured on one MI355X: 4.7e-6 (fp32) and 5.3e-6 (bf16) at (2, 33, 16, 256, 256) with agg = sum, where
    |logit| reaches 100 (one fp32 ulp is 7.6e-6); every other case within 3.7e-6."""
    ref = case(shape, agg)[5][op]
    lg, _ = run(shape, agg, op)
    e = float((lg.double() - ref).abs().max())
    print(f'{shape} {agg} {op}: logits {e:.2e} (|logit| <= {float(ref.abs().max()):.1f})')
    assert e <= TOL


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('agg', R.AGGS)
@pytest.mark.parametrize('shape', SHAPES)
def test_table_counts_cell_for_cell(shape, agg, op):
    _, _, label, task, cut, _ = case(shape, agg)
    lg, tb = run(shape, agg, op)
    assert tb.dtype == torch.int32 and tuple(tb.shape) == (shape[5], shape[6], shape[7])
    want = count(lg.numpy(), label.numpy(), task.numpy(), cut.numpy(), shape[7])
    assert np.array_equal(tb.numpy().astype(np.int64), want)
    assert int(tb.sum()) <= shape[5] * shape[6] * shape[0]
    for j in set(range(shape[7])) - set(task.tolist()):       # a task no sample has keeps a zero column
        assert int(tb[:, :, j].abs().sum()) == 0


@pytest.mark.parametrize('agg', R.AGGS)
def test_bf16_stored_slots(agg):
    shape = (3, 5, 8, 192, 192, 3, 6, 8)
    Ws, slots, label, task, cut, ref = case(shape, agg)
    xb = slots.cuda().bfloat16()
    lg, tb = score(Ws, xb, agg, torch.bfloat16, label, task, cut, 8)
    lg32, tb32 = run(shape, agg, torch.bfloat16)              # fp32-stored slots round to the same operands
    assert torch.equal(lg.cpu(), lg32) and torch.equal(tb.cpu(), tb32)
    for w, W in enumerate(Ws):
        assert torch.equal(lg[w], readout_logits(W, xb, agg, torch.bfloat16))
    assert float((lg.cpu().double() - ref[torch.bfloat16]).abs().max()) <= TOL
    # fp32 operands on bf16-stored slots: the stored values are the operands
    lgf, _ = score(Ws, xb, agg, torch.float32, label, task, cut, 8)
    for w, W in enumerate(Ws):
        assert torch.equal(lgf[w], readout_logits(W, xb, agg, torch.float32))


@pytest.mark.parametrize('op', OPS)
def test_the_table_accumulates(op):
    shape = (5, 7, 5, 96, 64, 3, 6, 4)
    Ws, slots, label, task, cut, _ = case(shape, 'max')
    lg, tb = run(shape, 'max', op)
    x = slots.cuda()
    la, acc = score(Ws, x[:2], 'max', op, label[:2], task[:2], cut, 4)
    lb, acc2 = score(Ws, x[2:], 'max', op, label[2:], task[2:], cut, 4, correct=acc)
    assert acc2 is acc and torch.equal(acc.cpu(), tb) and torch.equal(torch.cat([la, lb], 1).cpu(), lg)
    score(Ws, x, 'max', op, label, task, cut, 4, correct=acc)      # a second call on a non-zero table adds to it
    assert torch.equal(acc.cpu(), 2 * tb)


@pytest.mark.parametrize('op', OPS)
@pytest.mark.parametrize('agg', ['max', 'sum'])
def test_the_compare_is_strict(agg, op):
    """Exact-arithmetic operands: small-integer slots, linear1 / linear2 weights of +-1, zero biases -- every logit is an
    exact integer in both operand dtypes.  Cuts at those integers and just below them: a logit equal to its cut is not
    above it."""
    B, T, N, C, F = 8, 3, 4, 32, 32
    g = torch.Generator().manual_seed(5)
    slots = torch.randint(-2, 3, (B, T, N, C), generator=g).float()
    sign = lambda *s: (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
    W = {'linear1.weight': sign(F, 2 * C), 'linear1.bias': torch.zeros(F), 'linear2.weight': sign(1, F),
         'linear2.bias': torch.zeros(1)}
    exact = R.frame_logits({k: v.double() for k, v in W.items()}, slots.double(), agg).max(1)[0]
    assert torch.equal(exact, exact.round()) and float(exact.abs().max()) < 2 ** 20
    vals = torch.unique(exact)[:16].float()
    cut = torch.cat([vals, torch.nextafter(vals, torch.full_like(vals, -float('inf')))])
    label, task = torch.ones(B), torch.arange(B).int()            # every sample its own task: the table is the decisions
    lg, tb = score([W], slots.cuda(), agg, op, label, task, cut, B)
    assert torch.equal(lg[0].cpu().double(), exact)
    want = (exact.float()[None, :] > cut[:, None])                # [K, B]
    assert torch.equal(tb[0].cpu(), want.int())
    k = vals.numel()
    for i, v in enumerate(vals):
        hit = exact == v.double()
        assert not want[i, hit].any() and want[k + i, hit].all()
    lz, tz = score([W], slots.cuda(), agg, op, torch.zeros(B), task, cut, B)
    assert torch.equal(tz[0].cpu(), (~want).int())


@pytest.mark.parametrize('op', OPS)
def test_identical_checkpoints_give_identical_rows(op):
    shape = (3, 5, 8, 192, 192, 3, 6, 8)
    Ws, slots, label, task, cut, _ = case(shape, 'max')
    lg, tb = score([Ws[1], Ws[0], Ws[1], Ws[1]], slots.cuda(), 'max', op, label, task, cut, 8)
    ref_lg, ref_tb = run(shape, 'max', op)
    for w in (0, 2, 3):
        assert torch.equal(lg[w].cpu(), ref_lg[1]) and torch.equal(tb[w].cpu(), ref_tb[1])
    assert torch.equal(lg[1].cpu(), ref_lg[0]) and torch.equal(tb[1].cpu(), ref_tb[0])


@pytest.mark.parametrize('op', OPS)
def test_empty_tasks_keep_zero_columns(op):
    shape = (3, 5, 8, 192, 192, 3, 6, 8)
    Ws, slots, label, _, cut, _ = case(shape, 'mean')
    task = torch.tensor([6, 2, 6]).int()
    _, tb = score(Ws, slots.cuda(), 'mean', op, label, task, cut, 8)
    tb = tb.cpu()
    assert int(tb[:, :, [0, 1, 3, 4, 5, 7]].abs().sum()) == 0 and int(tb[:, :, [2, 6]].sum()) > 0
    assert int(tb[:, :, 6].max()) <= 2 and int(tb[:, :, 2].max()) <= 1


@pytest.mark.parametrize('op', OPS)
def test_two_runs_are_bit_equal(op):
    shape = (2, 75, 8, 192, 192, 2, 6, 8)
    Ws, slots, label, task, cut, _ = case(shape, 'max')
    lg, tb = score(Ws, slots.cuda(), 'max', op, label, task, cut, 8)
    ref_lg, ref_tb = run(shape, 'max', op)
    assert torch.equal(lg.cpu(), ref_lg) and torch.equal(tb.cpu(), ref_tb)


def test_refusals():
    shape = (3, 5, 8, 192, 192, 3, 6, 8)
    Ws, slots, label, task, cut, _ = case(shape, 'max')
    x = slots.cuda()
    with pytest.raises(_lib.SdmiError, match='K'):
        score(Ws, x, 'max', torch.float32, label, task, torch.linspace(-1, 1, 33), 8)
    with pytest.raises(_lib.SdmiError, match='J'):
        score(Ws, x, 'max', torch.float32, label, task, cut, 65)
    assert not kern.readout_covers(8, 48, 32) and not kern.vqa_score_covers(8, 48, 32, 1, 1, 1)
    W48 = checkpoints(8, 48, 32, 1)
    with pytest.raises(_lib.SdmiError, match='C must be'):
        ops.vqa_score(torch.zeros(2, 3, 8, 48).cuda(), torch.zeros(1, 32 * 96).cuda(), W48[0]['linear1.bias'][None].cuda(),
                      W48[0]['linear2.weight'].cuda(), W48[0]['linear2.bias'].cuda(), 'max', torch.float32,
                      label[:2].cuda(), task[:2].cuda(), cut.cuda(), 8)
    ok = score(Ws, x, 'max', torch.float32, label, task, torch.linspace(-1, 1, 32), 64)     # the bounds themselves pass
    assert tuple(ok[1].shape) == (3, 32, 64)
