"""Host side of the conv / linear backward (slotdiffusion_amd/bwd.py), no GPU: the launch planner against a table recorded
from GPU runs and against the library's own kernel selection; the ordering rules of GradSchedule against recorders.

tests/golden/bwd_plan_rows.json: the distinct rows of tools/trace_bwd_launches.py --rows / --table over one training
backward of the benchmark model (bf16, fp8 forward, and with the pair launches off), the small test model (fp32), the
plain SA model and a 3-frame video clip, recorded before the planner existed: what each layer's backward was given and
what it launched."""
import contextlib
import json
import os

import torch

from slotdiffusion_amd import _lib, bwd
from tests import common as C

T = json.load(open(os.path.join(C.GOLD, 'bwd_plan_rows.json')))
DT = {'bfloat16': torch.bfloat16, 'float32': torch.float32, _lib.BF16: torch.bfloat16, _lib.F32: torch.float32}
KERNEL = {'c64': _lib.ENUMS['SDMI_WGRAD_KERNEL_C64'], 'halo': _lib.ENUMS['SDMI_WGRAD_KERNEL_HALO']}


def _problem(w, is_conv, pad):
    """The LayerProblem behind a recorded SdmiWgradArgs (through the public constructors)."""
    dt = DT[w['dtype']]
    if is_conv:
        P = bwd.LayerProblem.conv(w['B'], w['H'], w['W'], w['Ho'], w['Wo'], w['Cin'], w['N'], w['ldy'], w['KH'], w['KW'],
                                  w['stride'], pad, dt, bool(w['ups']))
    else:
        P = bwd.LayerProblem(False, w['B'], 1, 1, 1, 1, w['Cin'], w['N'], w['Cin'], w['B'], 1, 1, 1, (0, 0, 0, 0), False,
                             w['lda'], w['ldy'], dt)
    return P


def _rows():
    for r in T['layers']:
        w = dict(zip(T['wgrad_keys'], r['wgrad']))
        if r['kind'] == 'deconv':
            yield r, w, None, _problem(w, True, (w['pad_t'],) * 4)
        else:
            ctx = dict(zip(T['ctx_keys'], r['ctx']))
            yield r, w, ctx, _problem(w, ctx['is_conv'], ctx['pad'])


def _plan(P, ctx):
    return bwd.plan_layer(P, **{k: ctx[k] for k in ('need_dx', 'direct', 'has_bias', 'bias_dst', 'dalias_cols', 'n_cus',
                                                   'pair_bwd', 'wgrad_halo')})


def test_planner_reproduces_the_recorded_launch_table():
    kinds = set()
    for r, w, ctx, P in _rows():
        assert P.wgrad_fields() == w, r
        if r['kind'] == 'deconv':
            assert bwd.standalone_splits(P) == r['splits'], r
            kinds.add('transposed convolution')
            continue
        plan = _plan(P, ctx)
        if r['kind'] == 'pair':
            assert plan.path == 'pair' and plan.pair == (r['wgrad_tile'], r['dgrad_cap'], r['splits']), (r, plan)
            kinds.add(f"pair, {r['wgrad_tile']}-wide dW tiles")
        else:
            assert (plan.path, plan.splits, plan.kernel, plan.pair) == ('side', r['splits'], r['kernel'], None), (r, plan)
            kinds.add('stand-alone, splits > 1' if r['splits'] > 1 else 'stand-alone, splits == 1')
            kinds.add({'c64': 'direct 64-channel', 'halo': 'direct channel-pair', 'gemm': 'gemm'}[r['kernel']])
        # the data gradient's launches (recorded for convolutions): one, or one per input-pixel parity
        parity = P.is_conv and P.stride > 1 and not P.ups
        mine = [f for _, _, f in P.parity_dgrads()[1]] if parity else [P.dgrad_fields()]
        if r['dgrad']:
            assert [[f.get(k, 0) for k in T['dgrad_keys']] for f in mine] == r['dgrad'], r
            kinds.update(['stride-2 data gradient by parity'] if parity and P.stride == 2 and len(mine) == 4 else [])
        kinds.update(['up-sampling convolution'] if P.ups else [])
        kinds.update(['non-direct destination'] if not ctx['direct'] and P.is_conv else [])
        kinds.update(['several fused names'] if ctx['n_names'] > 1 else [])
        kinds.update(['fp32'] if P.dt == torch.float32 else [])
    for g in T['groups']:
        ps = [(dict(zip(T['wgrad_keys'], p[:-1])), bool(p[-1])) for p in g['problems']]
        assert bwd.plan_group([(_problem(w, False, None), bias) for w, bias in ps]) == g['splits'], g
        kinds.update(['grouped launch of four'] if len(ps) == 4 else [])
    # the table cannot shrink unnoticed
    want = {'pair, 128-wide dW tiles', 'pair, 64-wide dW tiles', 'stand-alone, splits > 1', 'stand-alone, splits == 1',
            'direct 64-channel', 'direct channel-pair', 'stride-2 data gradient by parity', 'up-sampling convolution',
            'non-direct destination', 'several fused names', 'fp32', 'grouped launch of four', 'transposed convolution'}
    assert want <= kinds, want - kinds


def test_planner_agrees_with_the_library_dispatch():
    """Where the planner sizes `splits` for a direct kernel the library takes that kernel; with one split (the result is
    written straight into the arena, nothing folds partials) it never does."""
    direct = set(KERNEL.values())
    seen = set()
    for r, w, ctx, P in _rows():
        if ctx is None:
            splits, kernel = bwd.standalone_splits(P), 'gemm'
        else:
            plan = _plan(P, ctx)             # (pair rows: the stand-alone launch they take with the pair launches off)
            splits, kernel = plan.splits, plan.kernel
        got = _lib.query('sdmi_wgrad_kernel', splits=splits, **P.wgrad_fields())
        assert got >= 0, (r, _lib.lib().sdmi_last_error())
        if kernel in KERNEL:
            assert got == KERNEL[kernel], (r, got)
            seen.add(kernel)
        if splits == 1:
            assert got not in direct, r
            seen.add(1)
        assert (got in (_lib.ENUMS['SDMI_WGRAD_KERNEL_F32_T128'], _lib.ENUMS['SDMI_WGRAD_KERNEL_F32_T64'])) == \
            (P.dt == torch.float32), r
    assert seen == {'c64', 'halo', 1}
    # the rule by itself: the two direct kernels' own shapes with one split go to the implicit GEMM
    for N, Cin, H in ((64, 64, 128), (128, 128, 32)):
        P = bwd.LayerProblem.conv(64, H, H, H, H, Cin, N, N, 3, 3, 1, (1, 1, 1, 1), torch.bfloat16)
        plan = bwd.plan_layer(P, need_dx=False, direct=True, has_bias=False, bias_dst=False, dalias_cols=None, n_cus=256)
        assert _lib.query('sdmi_wgrad_kernel', splits=plan.splits, **P.wgrad_fields()) == KERNEL[plan.kernel]
        assert _lib.query('sdmi_wgrad_kernel', splits=1, **P.wgrad_fields()) == _lib.ENUMS['SDMI_WGRAD_KERNEL_IGEMM']


# ---- ordering rules ---------------------------------------------------------------------------------------------------
class _Recorder:
    """Stand-ins for torch.cuda's streams / events and _lib.call that log what would be enqueued where."""

    def __init__(self, monkeypatch):
        rec = self
        self.log, self.current, self.n = [], [], 0

        class Stream:
            def __init__(self, name=None):
                rec.n += name is None
                self.name = name or f'side{rec.n}'
                self.cuda_stream = self.name

            def wait_event(self, ev):
                rec.log.append(('wait_event', self.name, ev.on))

            def wait_stream(self, other):
                rec.log.append(('wait_stream', self.name, other.name))

        class Event:
            def record(self):
                self.on = rec.current[-1].name

        @contextlib.contextmanager
        def stream(s):
            rec.current.append(s)
            try:
                yield
            finally:
                rec.current.pop()

        def call(fname, st, **kw):
            dst = ()
            if fname in ('sdmi_wgrad_fold_group', 'sdmi_wgrad_group'):
                arr = (_lib.CSTRUCT['SdmiWgradArgs'] * kw['n']).from_address(kw['problems'])
                dst = tuple(a.dw for a in arr)
            elif fname == 'sdmi_bwd_pair':
                dst = (_lib.CSTRUCT['SdmiWgradArgs'].from_address(kw['wgrad']).dw,)
            rec.log.append((fname, st, dst or kw.get('dw')))

        self.current.append(Stream('main'))
        monkeypatch.setattr(torch.cuda, 'Stream', Stream)
        monkeypatch.setattr(torch.cuda, 'Event', Event)
        monkeypatch.setattr(torch.cuda, 'current_stream', lambda: rec.current[-1])
        monkeypatch.setattr(torch.cuda, 'stream', stream)
        monkeypatch.setattr(_lib, 'call', call)

    def index(self, *entry):
        hits = [i for i, e in enumerate(self.log) if e[:len(entry)] == entry]
        assert len(hits) == 1, (entry, self.log)
        return hits[0]


P_DW, P_DB, Q_DW = 0x1000, 0x2000, 0x3000        # gradient destinations (only compared, never dereferenced)
LIN = bwd.LayerProblem(False, 1024, 1, 1, 1, 1, 128, 128, 128, 1024, 1, 1, 1, (0, 0, 0, 0), False, 128, 128, torch.bfloat16)


def _sched(monkeypatch):
    rec = _Recorder(monkeypatch)
    s = bwd.GradSchedule(True)
    s.join_by_hand()                        # (no autograd pass to queue the join on)
    return rec, s


def _pair(s, dw=P_DW, db=P_DB):
    plan = bwd.plan_layer(LIN, need_dx=True, direct=True, has_bias=True, bias_dst=True, dalias_cols=None, n_cus=256)
    assert plan.path == 'pair' and plan.pair.splits > 1
    s.launch_pair(LIN, plan.pair, dict(LIN.dgrad_fields(), a=16, w=16, out=16, split_k=1),
                  dict(LIN.wgrad_fields(), a=16, dy=16, dw=dw, dbias=db, accumulate=1), 'cpu')


def _side(s, key='p.weight', dw=P_DW, db=P_DB):
    s.side_wgrad(key, (dw, db), lambda: _lib.call('sdmi_wgrad', bwd._st(), dw=dw), ())


def test_pending_fold_runs_before_a_side_stream_writer_of_the_same_parameter(monkeypatch):
    rec, s = _sched(monkeypatch)
    _pair(s)
    _side(s)
    pair, fold, side = rec.index('sdmi_bwd_pair'), rec.index('sdmi_wgrad_fold_group'), rec.index('sdmi_wgrad')
    assert rec.log[fold] == ('sdmi_wgrad_fold_group', 'main', (P_DW,)) and rec.log[side][1] == 'side1'
    # ... and the side stream picks up the main stream behind the fold
    assert pair < fold < rec.index('wait_event', 'side1', 'main') < side
    # another parameter's writer leaves the pending fold to the next pair launch
    rec2, s2 = _sched(monkeypatch)
    _pair(s2)
    _side(s2, 'q.weight', Q_DW, 0)
    assert not [e for e in rec2.log if e[0] == 'sdmi_wgrad_fold_group'] and s2._pfold is not None


def test_main_stream_writer_waits_for_the_side_stream_of_its_destination(monkeypatch):
    rec, s = _sched(monkeypatch)
    _side(s, db=0)
    _side(s, 'q.weight', Q_DW, 0)
    _pair(s)
    assert rec.index('sdmi_wgrad', 'side1') < rec.index('wait_stream', 'main', 'side1') < rec.index('sdmi_bwd_pair')
    assert not [e for e in rec.log if e[:3] == ('wait_stream', 'main', 'side2')]      # (q's stream is not waited for)


def test_a_parameter_keeps_its_side_stream(monkeypatch):
    rec, s = _sched(monkeypatch)
    _side(s)
    _side(s, 'q.weight', Q_DW, 0)
    _side(s)
    assert [e[1] for e in rec.log if e[0] == 'sdmi_wgrad'] == ['side1', 'side2', 'side1']


def test_grouped_launch_folds_a_pending_destination_first(monkeypatch):
    rec, s = _sched(monkeypatch)
    _pair(s)
    rows = [dict(LIN.wgrad_fields(), a=16, dy=16, dw=d, dbias=0, accumulate=1) for d in (Q_DW, P_DW)]
    s.launch_group(rows, bwd.plan_group([(LIN, False)] * 2), [], 'cpu')
    fold, group = rec.index('sdmi_wgrad_fold_group'), rec.index('sdmi_wgrad_group')
    assert rec.log[fold][2] == (P_DW,) and rec.log[group][2] == (Q_DW, P_DW) and rec.log[group][1].startswith('side')
    assert rec.index('sdmi_bwd_pair') < fold < group


def test_join_leaves_nothing_behind(monkeypatch):
    rec, s = _sched(monkeypatch)
    _side(s)
    _pair(s, Q_DW, 0)
    keep = torch.zeros(1)
    s.side_wgrad('r.weight', (0x4000, 0), lambda: None, (keep,))
    assert s._pfold is not None and s._side_dst and s._keep
    n = len(rec.log)
    s.join()
    tail = rec.log[n:]
    assert tail[0] == ('sdmi_wgrad_fold_group', 'main', (Q_DW,))
    assert {e[2] for e in tail if e[:2] == ('wait_stream', 'main')} == {f'side{i}' for i in range(1, bwd.GradSchedule.N_SIDE + 1)}
    assert s._pfold is None and not s._side_dst and not s._keep and not s._cq and not s._join_queued
