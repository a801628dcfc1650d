"""Launch trace of one training backward at the C ABI (GPU box): for every call the entry point, every scalar field,
every pointer field as null / non-null, the sub-structs of sdmi_bwd_pair / sdmi_wgrad_group / sdmi_wgrad_fold_group, and
the stream as an ordinal of first appearance (main = 0).  Two checkouts that launch the same work write byte-identical
files; the tool only wraps `_lib._call` and `_lib.struct_array`.

    python tools/trace_bwd_launches.py WORKLOAD OUT.txt [--rows ROWS.jsonl]

WORKLOAD: bench_bf16 | bench_fp8 (the benchmark model, B = 64) | bench_side (the same, bf16, without the pair launches:
every layer's stand-alone weight gradient) | test_fp32 (the small test model, B = 2) | sa_plain
(transposed convolutions, B = 2) | video (MOVi-E config, one 3-frame clip, fp32).  One eager step warms up, the
backward of the second is traced.

--rows also records, per conv / linear backward (GemmFn.core), what the launch planner is given and what was launched:
the source of tests/golden/bwd_plan_rows.json (`python tools/trace_bwd_launches.py --table ROWS.jsonl ... > fixture`)."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import _lib, kern            # noqa: E402

SUBS = {'SdmiBwdPairArgs': {'dgrad': 'SdmiGemmArgs', 'wgrad': 'SdmiWgradArgs', 'fold': 'SdmiWgradArgs'},
        'SdmiWgradGroupArgs': {'problems': 'SdmiWgradArgs'}}
GEOM = ('M', 'N', 'K', 'lda', 'ldy', 'B', 'H', 'W', 'Cin', 'Ho', 'Wo', 'KH', 'KW', 'stride', 'pad_t', 'pad_l', 'ups')


class Trace:
    def __init__(self):
        self.on = False
        self.calls, self.arrays, self.streams = [], {}, {}
        self.core = None            # the GemmFn.core call in progress (--rows)
        self.rows = []

    def fields(self, sname, get):
        """Scalar fields by value, pointer fields as 0 / 1."""
        return {f: (int(bool(get(f))) if ct is ctypes.c_void_p else get(f)) for f, ct in _lib.STRUCTS[sname]}

    def sub(self, sname, addr, n=1):
        name, arr = self.arrays[addr]
        assert name == sname and len(arr) >= n, (name, sname)
        return [self.fields(sname, lambda f, a=arr[i]: getattr(a, f)) for i in range(n)]

    def record(self, fname, stream, kw):
        sname = _lib.FUNCS[fname]
        rec = dict(entry=fname, stream=self.streams.setdefault(stream or 0, len(self.streams)),
                   args=self.fields(sname, lambda f: kw.get(f, 0)))
        for f, sub in SUBS.get(sname, {}).items():
            if kw.get(f):
                rec[f] = self.sub(sub, kw[f], kw.get('n', 1))
        self.calls.append(rec)
        if self.core is not None:
            self.core['calls'].append(rec)
        elif fname in ('sdmi_wgrad', 'sdmi_wgrad_group'):
            self.rows.append(dict(ctx=None, calls=[rec]))


def install(tr):
    raw_call, raw_array, raw_core = _lib._call, _lib.struct_array, kern.GemmFn.core

    def _call(fname, stream, **kw):
        if tr.on:
            tr.record(fname, stream, kw)
        return raw_call(fname, stream, **kw)

    def struct_array(struct_name, rows):
        arr = raw_array(struct_name, rows)
        tr.arrays[ctypes.addressof(arr)] = (struct_name, arr)
        return arr

    def core(wb, x, dy, wnames, bnames, geom, need_dx, dalias=None):
        if not tr.on or tr.core is not None:
            return raw_core(wb, x, dy, wnames, bnames, geom, need_dx, dalias)
        names = (wnames,) if isinstance(wnames, str) else tuple(wnames)
        dst = kern._grads_of(wb, names)
        kh, kw_ = geom[0], geom[1]
        is_conv = x.dim() == 4 and (kh, kw_) != (0, 0)
        taps = kh * kw_ if is_conv else 1
        k_true = wb.t[names[0]].numel() // wb.t[names[0]].shape[0]
        tr.core = dict(ctx=dict(
            is_conv=is_conv, dt=str(x.dtype).split('.')[-1], pad=(list(geom[3]) if is_conv else [0, 0, 0, 0]),
            need_dx=bool(need_dx), direct=bool(dst is not None and k_true == taps * x.shape[-1]),
            has_bias=bnames is not None, bias_dst=bool(bnames is not None and kern._grads_of(wb, bnames) is not None),
            dalias_cols=(dalias.shape[-1] if dalias is not None else None), n_names=len(names),
            n_cus=int(torch.cuda.get_device_properties(x.device).multi_processor_count),
            pair_bwd=bool(wb.pair_bwd), wgrad_halo=bool(kern._WGRAD_HALO)), calls=[])
        try:
            return raw_core(wb, x, dy, wnames, bnames, geom, need_dx, dalias)
        finally:
            tr.rows.append(tr.core)
            tr.core = None

    _lib._call, _lib.struct_array, kern.GemmFn.core = _call, struct_array, staticmethod(core)


def workload(name):
    """-> (model, batch dict)."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
    sys.path.insert(0, root)
    from tests import common as C
    from tests.detfill import det_fill_, is_buffer_name
    if name in ('bench_bf16', 'bench_fp8', 'bench_side'):
        import bench
        m, cfg, _ = bench.build_model(torch.bfloat16)
        m = m.cuda()
        if name == 'bench_fp8':
            m.set_compute_dtype('fp8')
        m.bank().pair_bwd = name != 'bench_side'
        return m, dict(img=bench.synth_batch(64, 0, 'cuda', cfg['resolution'][0]))
    from slotdiffusion_amd import models
    if name == 'test_fp32':
        cfg = C.clevrtex_cfg()
        m = models.SADiffusion(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['loss_dict'],
                               compute_dtype=torch.float32)
        img = C.make_inputs(2)[0]
    elif name == 'sa_plain':
        cfg = C.sa_plain_cfg()
        m = models.SA(cfg['resolution'], cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['loss_dict'],
                      compute_dtype=torch.float32)
        img = C.make_inputs(2)[0]
    elif name == 'video':
        cfg, T = C.movie_cfg(), 3
        m = models.SAViDiffusion(cfg['resolution'], T, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'],
                                 cfg['pred_dict'], cfg['loss_dict'], compute_dtype=torch.float32)
        img = C.make_inputs(T, seed=11)[0].view(1, T, 3, 128, 128)
    else:
        raise SystemExit(f'unknown workload {name}')
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    return m.cuda(), dict(img=img.cuda())


def run(name, out, rows_out):
    tr = Trace()
    install(tr)
    m, batch = workload(name)
    m.train()
    tr.streams[torch.cuda.current_stream().cuda_stream] = 0
    for step in range(2):
        m.grad_arena().zero_()
        losses = m.calc_train_loss(batch, m(batch))
        loss = sum(v for v in losses.values() if torch.is_tensor(v) and v.requires_grad)
        tr.on = step == 1
        loss.backward()
        tr.on = False
        torch.cuda.synchronize()
    assert torch.isfinite(m.grad_arena()).all()
    with open(out, 'w') as f:
        for rec in tr.calls:
            f.write(json.dumps(rec, sort_keys=True) + '\n')
    if rows_out:
        with open(rows_out, 'w') as f:
            for row in tr.rows:
                f.write(json.dumps(dict(row, workload=name), sort_keys=True) + '\n')
    print(f'{name}: {len(tr.calls)} calls on {len(tr.streams)} streams -> {out}')


WG_KEYS = ('dtype',) + GEOM
DG_KEYS = ('dtype', 'out_dtype', 'M', 'N', 'K', 'lda', 'ldw', 'ldc', 'B', 'H', 'W', 'Cin', 'Ho', 'Wo', 'KH', 'KW', 'stride',
           'pad_t', 'pad_l', 'ups', 'act', 'alpha', 'batch', 'zins', 'ldr', 'oH', 'oW', 'osy', 'osx', 'ooy', 'oox')
CTX_KEYS = ('is_conv', 'dt', 'pad', 'need_dx', 'direct', 'has_bias', 'bias_dst', 'dalias_cols', 'n_names', 'n_cus',
            'pair_bwd', 'wgrad_halo')


def _sized_for(a, ctx):
    """The kernel a recorded stand-alone launch was sized for.  The only M-splits that are not the plain workgroup-target
    formula are those chosen for one of the two direct 3x3 kernels: one slot per CU for the 64 -> 64 channel kernel,
    CUs // channel pairs for the channel-pair kernel."""
    mt = 64 if ctx['dt'] == 'bfloat16' else 32
    tiles = ((a['N'] + 127) // 128) * ((a['K'] + 127) // 128)
    plain = 1 if a['M'] <= 16 * mt else max(1, min((192 + tiles - 1) // tiles, a['M'] // (8 * mt), 512))
    if a['splits'] == plain or a['KH'] != 3:
        return 'gemm'
    return 'c64' if (a['N'], a['Cin'], a['splits']) == (64, 64, ctx['n_cus']) else 'halo'


def table(paths):
    """The distinct planner rows of --rows files, as the JSON fixture of tests/test_bwd_plan_cpu.py (to stdout): field
    values as lists in the order of the *_keys entries."""
    layers, groups = {}, {}
    vals = lambda a, keys: [a[k] for k in keys]
    for path in paths:
        for line in open(path):
            row = json.loads(line)
            ctx, calls = row['ctx'], row['calls']
            pair = [c for c in calls if c['entry'] == 'sdmi_bwd_pair']
            wg = [c for c in calls if c['entry'] == 'sdmi_wgrad']
            grp = [c for c in calls if c['entry'] == 'sdmi_wgrad_group']
            if grp:            # a grouped launch: every problem's fields and bias -> its splits
                ps = grp[0]['problems']
                out = dict(problems=[vals(p, WG_KEYS) + [p['dbias']] for p in ps], splits=[p['splits'] for p in ps])
                groups.setdefault(json.dumps(out), out)
                continue
            if ctx is None:    # a transposed convolution's weight gradient (DeconvFn)
                a = wg[0]['args']
                out = dict(kind='deconv', wgrad=vals(a, WG_KEYS), splits=a['splits'])
            elif pair:
                p = pair[0]
                out = dict(kind='pair', ctx=vals(ctx, CTX_KEYS), wgrad=vals(p['wgrad'][0], WG_KEYS),
                           dgrad=[vals(p['dgrad'][0], DG_KEYS)], wgrad_tile=p['args']['wgrad_tile'],
                           dgrad_cap=p['args']['dgrad_cap'], splits=p['wgrad'][0]['splits'])
            else:
                a = wg[0]['args']
                out = dict(kind='side', ctx=vals(ctx, CTX_KEYS), wgrad=vals(a, WG_KEYS), splits=a['splits'],
                           kernel=_sized_for(a, ctx),
                           dgrad=[vals(c['args'], DG_KEYS) for c in calls if c['entry'] == 'sdmi_igemm' and ctx['is_conv']])
            layers.setdefault(json.dumps(out), out)
    out = dict(wgrad_keys=WG_KEYS, dgrad_keys=DG_KEYS, ctx_keys=CTX_KEYS, layers=list(layers.values()),
               groups=list(groups.values()))
    sys.stdout.write(json.dumps(out, separators=(',', ':')).replace('{"', '\n{"') + '\n')


if __name__ == '__main__':
    if sys.argv[1] == '--table':
        table(sys.argv[2:])
    else:
        rows = sys.argv[sys.argv.index('--rows') + 1] if '--rows' in sys.argv else None
        run(sys.argv[1], sys.argv[2], rows)
