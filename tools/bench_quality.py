"""Time the image-quality stage at the MOVi-E shape -- 128 x 128 frames, 24-frame videos walked in chunks of 6 -- on a bf16
SAViDiffusion, batches of 1, 4 and 8 synthetic videos, in ONE process with the variants alternating inside every round
(same box, same session; medians over rounds, the spread reported):

    tail     the scoring of one chunk's frames (the decoder's NHWC-4 rows against the loader's NCHW frames), with and
             without the 8-bit frames:
               fused     metrics.image_quality -> ONE sdmi_img_quality launch + the sum over its band partials, then the
                         ONE host copy of the [F, 2] table the stage makes per batch
               composed  what the stage would be on the functions that existed before: ops.nhwc_to_nchw, to_rgb twice,
                         mse_metric, psnr_metric, ssim_metric (each ends in a host copy), and for the frames
                         round / cast / permute of both images
             reported: ms of wall time issued eagerly (host launches and synchronisations included), C-ABI calls (the
             call log, written while counting only), ATen operator calls (a TorchDispatchMode), bytes allocated during
             one pass and the peak above what was allocated before it
    kernel   sdmi_img_quality alone against sdmi_sqerr_rows + sdmi_ssim alone on ready to_rgb images (HIP events)
    stage    quality.evaluate_video_reconstruction on either tail (metrics._IMG_QUALITY_FUSED): videos / s and the peak
             memory above the model, --steps sampler steps (default 20: the reference's)

    python tools/bench_quality.py [--frames 24] [--chunk 6] [--rounds 7] [--reps 20] [--out profiles/quality_bench.json]

Also recorded: the largest |d ssim|, relative d se and whether the 8-bit frames are equal between the two tails on the
inputs timed (asserted against the bounds of tests/test_gpu_img_quality.py)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

_LOG = tempfile.NamedTemporaryFile(prefix='sdmi_calls_', suffix='.log', delete=False).name
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from slotdiffusion_amd import _lib, configs, extract, models, ops, quality      # noqa: E402
from slotdiffusion_amd import metrics as MT                                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=24)
ap.add_argument('--chunk', type=int, default=6)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--stage-rounds', type=int, default=3)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--out', default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit('bench_quality.py measures on the GPU; none found')

T, CH = args.frames, args.chunk
BATCHES = (1, 4, 8)
TAILS = ('fused', 'composed')
CHECK_SHAPES = [(2, 11, 11), (3, 37, 53), (2, 32, 32), (2, 24, 40), (1, 27, 16), (1, 128, 128), (1, 224, 224), (2, 45, 128),
                (1, 15, 128)]


class _CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def tail(rows, gt, which, u8):
    """One chunk's scoring -> (the batch's values on the host, pred_u8, gt_u8)."""
    n = 3 * gt.shape[2] * gt.shape[3]
    if which == 'fused':
        tab, p8, g8 = MT.image_quality(rows, gt, pred_nhwc4=True, want_u8=(u8, u8), fused=True)
        return MT.batch_quality(tab.cpu(), n), p8, g8
    pred = ops.nhwc_to_nchw(rows, 3)
    a, b = MT.to_rgb(pred), MT.to_rgb(gt)
    vals = {'mse': MT.mse_metric(a, b), 'psnr': MT.psnr_metric(a, b), 'ssim': MT.ssim_metric(a, b)}
    p8 = g8 = None
    if u8:
        p8 = torch.round(a * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        g8 = torch.round(b * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return vals, p8, g8


def kernels_alone(rows, gt, a, b, which):
    st = torch.cuda.current_stream().cuda_stream
    F_, _, H, W = gt.shape
    if which == 'fused':
        _, nb = MT.img_quality_bands(H, W)
        _lib.call('sdmi_img_quality', st, pred=rows.data_ptr(), gt=gt.data_ptr(), partial=_SCR['part'].data_ptr(), F=F_, H=H, W=W,
                  pred_nhwc4=1, gt_nhwc4=0, nbands=nb)
    else:
        n = 3 * H * W
        _lib.call('sdmi_sqerr_rows', st, x=a.data_ptr(), y=b.data_ptr(), partial=_SCR['sq'].data_ptr(), B=F_, n=n, nchunk=12, mode=0)
        _lib.call('sdmi_ssim', st, x=_SCR['xs'].data_ptr(), y=_SCR['ys'].data_ptr(), out=_SCR['planes'].data_ptr(), P=F_ * 3, H=H,
                  W=W, data_range=255.0)


_SCR = {}


def logged_calls(fn):
    n0 = sum(1 for _ in open(_LOG))
    _lib.set_call_log(_LOG)
    fn()
    _lib.set_call_log(None)                  # off while timing
    return [l.split('\t')[0] for l in open(_LOG)][n0:]


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def memory(fn):
    """-> (bytes allocated during one pass, peak above what was allocated before it)"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    s0 = torch.cuda.memory_stats()['allocated_bytes.all.allocated']
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    total = torch.cuda.memory_stats()['allocated_bytes.all.allocated'] - s0
    del out
    return int(total), int(peak)


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def build():
    cfg = configs.movie_cfg()
    m = models.SAViDiffusion(cfg['resolution'], CH, cfg['slot_dict'], cfg['enc_dict'], cfg['dec_dict'], cfg['pred_dict'],
                             cfg['loss_dict'], compute_dtype=torch.bfloat16)
    return m.cuda().eval(), cfg


def stage(m, ds, B, fused):
    old = MT._IMG_QUALITY_FUSED
    MT._IMG_QUALITY_FUSED = fused
    try:
        return quality.evaluate_video_reconstruction(m, ds, batch_size=B, chunk_len=CH, seed=1, dpm_steps=args.steps)
    finally:
        MT._IMG_QUALITY_FUSED = old


_lib.set_call_log(None)
m, cfg = build()
H, W = cfg['resolution']
res = dict(date=time.strftime('%Y-%m-%d'), device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps,
           stage_rounds=args.stage_rounds, sampler_steps=args.steps, frames=T, chunk_len=CH, resolution=[H, W],
           dtype='bf16 model; decoder rows, frames and the tail fp32 / fp64', bands_per_frame=MT.img_quality_bands(H, W)[1],
           batches=[])
with torch.no_grad():
    # the shapes and the input recipe of tests/test_gpu_img_quality.py: the observed maxima of fused against composed
    worst = dict(max_abs_d_ssim=0.0, max_rel_d_se=0.0, uint8_frames_equal=True)
    for F_, h_, w_ in CHECK_SHAPES:
        g = torch.Generator().manual_seed(4321 + 1000 * F_ + 10 * h_ + w_)
        y = 2.4 * torch.rand(F_, 3, h_, w_, generator=g) - 1.2
        x = (y + 0.2 * torch.randn(F_, 3, h_, w_, generator=g)).cuda()
        y = y.cuda()
        f, c = (MT.image_quality(x, y, want_u8=(True, True), fused=k) for k in (True, False))
        worst['max_abs_d_ssim'] = max(worst['max_abs_d_ssim'], float((f[0][:, 1] - c[0][:, 1]).abs().max()))
        worst['max_rel_d_se'] = max(worst['max_rel_d_se'], float(((f[0][:, 0] - c[0][:, 0]).abs() / c[0][:, 0]).max()))
        worst['uint8_frames_equal'] &= bool(torch.equal(f[1], c[1]) and torch.equal(f[2], c[2]))
    assert worst['max_abs_d_ssim'] <= 1e-9 and worst['max_rel_d_se'] <= 1e-10 and worst['uint8_frames_equal'], worst
    res['fused_vs_composed_on_the_test_shapes'] = dict(worst, shapes=[list(s) for s in CHECK_SHAPES],
                                                       bounds=dict(abs_d_ssim=1e-9, rel_d_se=1e-10))
    for B in BATCHES:
        ds = extract.SyntheticVideoDataset(dict(resolution=cfg['resolution']), num_videos=B, video_len=T, seed=B)
        video = torch.stack([ds.get_video(i)['video'] for i in range(B)]).cuda()
        gt = video[:, :CH].flatten(0, 1).contiguous()                                 # one chunk's frames, NCHW
        slots = m.encode_stream(video[:, :CH], None)
        x1 = torch.randn(1, 3, *m.latent_res, generator=torch.Generator().manual_seed(B)).cuda()
        rows, nhwc4 = m.dm_decoder.sample_rows({'slots': slots.flatten(0, 1).contiguous()}, use_dpm=True,
                                               x_T=x1.repeat(B * CH, 1, 1, 1), dpm_steps=args.steps)
        assert nhwc4 and rows.shape == (B * CH, H, W, 4)
        F_ = B * CH
        entry = dict(videos=B, frames_per_chunk=F_)
        # ---- agreement of the two tails on these inputs
        outs = {w: tail(rows, gt, w, True) for w in TAILS}
        tf = MT.image_quality(rows, gt, pred_nhwc4=True, fused=True)[0].cpu()
        tc = MT.image_quality(rows, gt, pred_nhwc4=True, fused=False)[0].cpu()
        d_ssim = float((tf[:, 1] - tc[:, 1]).abs().max())
        d_se = float(((tf[:, 0] - tc[:, 0]).abs() / tc[:, 0]).max())
        same_u8 = bool(torch.equal(outs['fused'][1], outs['composed'][1]) and torch.equal(outs['fused'][2], outs['composed'][2]))
        assert d_ssim <= 1e-9 and d_se <= 1e-10 and same_u8, (d_ssim, d_se, same_u8)
        entry['fused_vs_composed'] = dict(max_abs_d_ssim=d_ssim, max_rel_d_se=d_se, uint8_frames_equal=same_u8,
                                          values={w: outs[w][0] for w in TAILS})
        # ---- the tail: calls, operators, memory, wall time
        for u8 in (False, True):
            key = 'tail_with_uint8' if u8 else 'tail'
            t = {w: [] for w in TAILS}
            info = {}
            for w in TAILS:
                fn = lambda w=w: tail(rows, gt, w, u8)
                fn()
                names = logged_calls(fn)
                with _CountOps() as c:
                    fn()
                total, peak = memory(fn)
                info[w] = dict(c_abi_calls=len(names), by_entry={n: names.count(n) for n in sorted(set(names))}, aten_ops=c.n,
                               bytes_allocated=total, peak_bytes_above_start=peak)
            for _ in range(args.rounds):
                for w in TAILS:
                    t[w].append(wall_ms(lambda w=w: tail(rows, gt, w, u8), args.reps))
            for w in TAILS:
                info[w]['wall_ms'] = stats(t[w])
            info['composed_over_fused'] = statistics.median(t['composed']) / statistics.median(t['fused'])
            info['fp32_frame_bytes'] = F_ * 3 * H * W * 4
            entry[key] = info
        # ---- the kernels alone
        a, b = MT.to_rgb(ops.nhwc_to_nchw(rows, 3)).contiguous(), MT.to_rgb(gt).contiguous()
        _SCR.update(part=torch.empty((F_, MT.img_quality_bands(H, W)[1], 2), dtype=torch.float64, device='cuda'),
                    sq=torch.empty((F_, 12), dtype=torch.float64, device='cuda'), xs=(a * 255.0).contiguous(),
                    ys=(b * 255.0).contiguous(), planes=torch.empty((F_ * 3,), dtype=torch.float64, device='cuda'))
        tk = {w: [] for w in TAILS}
        for w in TAILS:
            kernels_alone(rows, gt, a, b, w)
        for _ in range(args.rounds):
            for w in TAILS:
                tk[w].append(event_ms(lambda w=w: kernels_alone(rows, gt, a, b, w), args.reps))
        entry['kernels_alone_ms'] = dict(sdmi_img_quality=stats(tk['fused']), sdmi_sqerr_rows_plus_sdmi_ssim=stats(tk['composed']))
        # ---- the whole stage
        for f in (True, False):
            stage(m, ds, B, f)                                                   # warm-up: graphs, code objects
        ts = {w: [] for w in TAILS}
        mem = {}
        for w, f in (('fused', True), ('composed', False)):
            mem[w] = memory(lambda f=f: stage(m, ds, B, f))[1]
        for _ in range(args.stage_rounds):
            for w, f in (('fused', True), ('composed', False)):
                ts[w].append(wall_ms(lambda f=f: stage(m, ds, B, f), 1))
        entry['stage'] = dict(ms_per_video_batch={w: stats(ts[w]) for w in TAILS},
                              videos_per_s={w: B / statistics.median(ts[w]) * 1e3 for w in TAILS},
                              peak_bytes_above_model=mem)
        res['batches'].append(entry)
        print(f'B{B}: tail fused {entry["tail"]["fused"]["wall_ms"]["median"]:.3f} ms / composed '
              f'{entry["tail"]["composed"]["wall_ms"]["median"]:.3f} ms; with uint8 {entry["tail_with_uint8"]["fused"]["wall_ms"]["median"]:.3f} / '
              f'{entry["tail_with_uint8"]["composed"]["wall_ms"]["median"]:.3f} ms; kernels alone {statistics.median(tk["fused"]):.3f} / '
              f'{statistics.median(tk["composed"]):.3f} ms; stage ' +
              ', '.join(f'{w} {entry["stage"]["videos_per_s"][w]:.3f} videos/s' for w in TAILS), file=sys.stderr)
os.unlink(_LOG)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, 'w'), indent=1)
