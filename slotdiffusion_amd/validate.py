"""The validation half of the training loop (SlotBaseMethod.validation_epoch and the `_sample_img` / `_sample_video` of
img_based/method.py and video_based/method.py): the averaged evaluation losses, the epoch-end DPM reconstruction loss and
the slot-decomposition panels (vis.slot_panel), logged through `Method.log_fn`.

Data protocol.  `datamodule.val_loader()` is an iterable of batches; `datamodule.val_set` is, for images, `__len__` and
`__getitem__ -> {'img' [3, H, W], ['masks' [H, W]]}`, for videos `files` and `get_video(i) -> {'video' [T, 3, H, W],
['masks' [T, H, W]]}` (the protocol extract.py uses).  `WithValidation` gives any datamodule both from a set.

Validation does not move training: the torch CPU / CUDA generator states and the model's `training` / `testing` flags are
saved and restored around it, and the samplers' initial noise comes from a generator seeded by (seed, iteration).  The
model's `eval_seed` stream (LDM._draw_tn) is made for validation and advances.
"""
import numpy as np
import torch

from . import vis

__all__ = ['sample_indices', 'WithValidation', 'SyntheticImageSegDataset', 'run_validation', 'num_cls']


def sample_indices(n, length):
    """`_get_sample_idx` (img_based/method.py:46-53, video_based/method.py:59-66), quirks included: n is capped at the
    length, lowered by one when it does not divide the length, and the indices are arange(0, length, length // n) -- so
    (8, 10) gives all ten indices and (2, 3) gives one."""
    n, length = int(n), int(length)
    if n > length:
        n = length
    n = n - 1 if length % n != 0 else n
    return np.arange(0, length, length // n)


class SyntheticImageSegDataset:
    """The image twin of extract.SyntheticVideoSegDataset: `len`, `[i] -> {'img' [3, H, W] in [-1, 1], 'masks' [H, W]
    int64}`, id 0 the background and ids 1 .. num_objects rectangles (later ids cover earlier ones), a function of
    (seed, i) alone.  The masks are unrelated to the pixels, as random pixels are to any scene."""

    def __init__(self, params, num_images=8, seed=1234, num_objects=4):
        res = params.get('resolution') if hasattr(params, 'get') else params.resolution
        self.H, self.W = (res, res) if isinstance(res, int) else tuple(res)
        self.num_images, self.seed, self.num_objects = num_images, seed, num_objects

    def __len__(self):
        return self.num_images

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < self.num_images:
            raise IndexError(i)
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        img = (torch.randn((3, self.H, self.W), generator=g) * 0.5).clamp_(-1, 1)
        masks = torch.zeros((self.H, self.W), dtype=torch.int64)
        for k in range(1, self.num_objects + 1):
            hh = int(torch.randint(max(1, self.H // 8), max(2, self.H // 2), (1,), generator=g))
            ww = int(torch.randint(max(1, self.W // 8), max(2, self.W // 2), (1,), generator=g))
            y0 = int(torch.randint(0, self.H - hh + 1, (1,), generator=g))
            x0 = int(torch.randint(0, self.W - ww + 1, (1,), generator=g))
            masks[y0:y0 + hh, x0:x0 + ww] = k
        return {'img': img, 'masks': masks, 'data_idx': i}


def _is_video_set(val_set):
    return hasattr(val_set, 'get_video')


def _set_len(val_set):
    return len(val_set.files) if _is_video_set(val_set) else len(val_set)


def _pget(params, key, default=None):
    return params.get(key, default) if hasattr(params, 'get') else getattr(params, key, default)


def _collate(items, device, keys=('img', 'masks')):
    return {k: torch.stack([torch.as_tensor(it[k]) for it in items]).to(device) for k in keys if k in items[0]}


def _clip(val_set, i, frames):
    """The first `frames` frames of video i as a loader item {'img' [T, 3, H, W], ['masks' [T, H, W]]}."""
    d = val_set.get_video(int(i))
    out = {'img': torch.as_tensor(d['video'])[:frames].float()}
    if 'masks' in d:
        out['masks'] = torch.as_tensor(d['masks'])[:frames]
    return out


class WithValidation:
    """A datamodule with a validation side: `len`, `train_loader` and every other attribute are the wrapped
    datamodule's; `val_set` is the given set and `val_loader()` walks it in order -- images in consecutive batches of
    `batch_size` (default params.val_batch_size), of videos the first params.n_sample_frames frames each.  `shard` is
    None (every batch) or (rank, world): rank r then takes batches r, r + world, ...; Method.validate sets it from its
    own use_ddp, so the sharding and the reduction of the sums always go together."""

    def __init__(self, datamodule, val_set, batch_size=None):
        self._dm = datamodule
        self.val_set = val_set
        self.val_batch_size = int(batch_size or _pget(datamodule.params, 'val_batch_size'))
        self.shard = None

    def __len__(self):
        return len(self._dm)

    def __getattr__(self, name):
        return getattr(self._dm, name)

    def train_loader(self, epoch=0):
        return self._dm.train_loader(epoch)

    def val_item(self, i):
        if _is_video_set(self.val_set):
            return _clip(self.val_set, i, _pget(self._dm.params, 'n_sample_frames'))
        return self.val_set[int(i)]

    def val_loader(self):
        n, bs = _set_len(self.val_set), self.val_batch_size
        device = getattr(self._dm, 'device', 'cpu')
        rank, world = self.shard or (0, 1)
        for bi, start in enumerate(range(0, n, bs)):
            if bi % world != rank:
                continue
            yield _collate([self.val_item(i) for i in range(start, min(start + bs, n))], device)


def num_cls(params, model):
    """The class count of the ground-truth panel (video_based/method.py:30-39): 11 on MOVi-C, 20 on MOVi-D / E (the
    palette's size), else the number of slots."""
    if 'movi' in str(_pget(params, 'dataset', '')).lower():
        level = str(_pget(params, 'movi_level', '')).lower()
        if level == 'c':
            return 11
        if level in ('d', 'e'):
            return 20
    return _pget(params, 'slot_dict')['num_slots']


# ------------------------------------------------------------------------------------------
# state kept away from training
# ------------------------------------------------------------------------------------------
class _Untouched:
    """Save / restore what validation must not move: torch's CPU and CUDA generator states, model.training and
    model.testing."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m = self.model
        self.cpu = torch.get_rng_state()
        self.cuda = None
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            self.cuda = torch.cuda.get_rng_state()              # (the current device's: the one the model runs on)
        self.training = m.training
        self.has_testing = hasattr(m, 'testing')
        self.testing = getattr(m, 'testing', None)
        return self

    def __exit__(self, *exc):
        m = self.model
        if self.has_testing:
            m.testing = self.testing
        elif hasattr(m, 'testing'):
            del m.testing
        m.train(self.training)
        torch.set_rng_state(self.cpu)
        if self.cuda is not None:
            torch.cuda.set_rng_state(self.cuda)
        return False


def _noise_gen(method, device, salt=0):
    g = torch.Generator(device=device)
    g.manual_seed((int(getattr(method.model, 'seed', 0)) * 1000003 + int(method.it)) * 31 + salt)
    return g


def _x_T(method, model, B, same_noise=False, salt=0):
    """The samplers' initial state [B, 3, h, w] from the validation generator (cond_ddpm.py:143-149: same_noise repeats
    one draw over the batch)."""
    dm = model.dm_decoder
    h, w = model.latent_res if hasattr(model, 'latent_res') else model.resolution
    g = _noise_gen(method, model.device, salt)
    if same_noise:
        return torch.randn((1, 3, h, w), generator=g, device=model.device).repeat(B, 1, 1, 1), dm
    return torch.randn((B, 3, h, w), generator=g, device=model.device), dm


def _np_image(pic):
    """uint8 [1, 3, GH, GW] -> numpy [GH, GW, 3] (wandb.Image)."""
    return pic[0].permute(1, 2, 0).contiguous().cpu().numpy()


def _stack_videos(T, n, GH, GW, device, k=1):
    """k uint8 buffers [T, 3, n * GH, GW] and, per video v, the band of rows its panel is written into:
    `_convert_video` stacks the sampled videos along the height."""
    bufs = [torch.empty((T, 3, n * GH, GW), dtype=torch.uint8, device=device) for _ in range(k)]
    return bufs, (lambda v: [b[:, :, v * GH:(v + 1) * GH] for b in bufs])


# ------------------------------------------------------------------------------------------
# samples per model
# ------------------------------------------------------------------------------------------
def _sample_sa(method, model, dm, log):
    """SAMethod._sample_img (img_based/method.py:110-127): val/imgs = [img, recon_combined, slots]."""
    vs = dm.val_set
    idx = sample_indices(_pget(method.params, 'n_samples'), len(vs))
    batch = _collate([vs[int(i)] for i in idx], model.device)
    out = model({'img': batch['img']})
    pic = vis.slot_panel(batch['img'], masks=out['masks'].squeeze(2), recon=out['recon_img'], slot_img=out['recons'],
                         tiles=('img', 'recon'), G=len(idx))
    log['val/imgs'] = _np_image(pic)


def _sample_savi(method, model, dm, log):
    """SAViMethod._sample_video (video_based/method.py:132-151): val/video = [img, recon, color, overlay, slots]."""
    vs = dm.val_set
    idx = sample_indices(_pget(method.params, 'n_samples'), len(vs.files))
    buf = band = None
    for v, i in enumerate(idx):
        video = torch.as_tensor(vs.get_video(int(i))['video']).float().to(model.device)
        out = {k: t[0] for k, t in model({'img': video[None]}).items()}
        T, N = out['masks'].shape[:2]
        if buf is None:
            _, GH, GW = vis.panel_geometry(T, N, 4, video.shape[2], video.shape[3], 1)
            buf, band = _stack_videos(T, len(idx), GH, GW, model.device)
        vis.slot_panel(video, masks=out['masks'].squeeze(2), recon=out['recon_img'], slot_img=out['recons'],
                       tiles=('img', 'recon', 'color', 'overlay'), G=1, out=band(v)[0])
    log['val/video'] = buf[0].cpu().numpy()


def _attention(model, img):
    """Slot Attention's slots and last attention map of a batch of images: [B, N, D], [B, h*w, N]."""
    from . import engine
    K = model.K()
    tok = engine.encoder_out(K, model._to_nhwc(img), model.rplan)
    return engine.slot_attention(K, tok, model.init_latents[0], model.num_iterations, model.eps)


def _sample_sa_diffusion(method, model, dm, log, epoch_end):
    """SADiffusionMethod._sample_img (img_based/method.py:320-376) without the intermediate-row grids."""
    vs, P = dm.val_set, method.params
    kw = dict(_pget(P, 'val_sampler_kwargs', None) or {})
    if epoch_end:
        idx = sample_indices(_pget(P, 'val_batch_size'), len(vs))
        batch = _collate([vs[int(i)] for i in idx], model.device, keys=('img',))
        x_T, _ = _x_T(method, model, len(idx), salt=1)
        samples = model.log_images(batch, use_dpm=True, x_T=x_T, **kw)['samples']
        log['val/dpm_sample_img_recon_loss'] = float(torch.nn.functional.mse_loss(samples.float(), batch['img'].float()))
    idx = sample_indices(_pget(P, 'n_samples'), len(vs))
    batch = _collate([vs[int(i)] for i in idx], model.device)
    img = batch['img'].float()
    slots, seg = _attention(model, img)
    x_T, dec = _x_T(method, model, len(idx), salt=2)
    rows, nhwc4 = dec.sample_rows({'img': img, 'slots': slots}, use_dpm=True, x_T=x_T, **kw)
    gt = batch.get('masks')
    tiles = ('img', 'recon') + (('gtcolor',) if gt is not None else ()) + ('color', 'overlay')
    pic = vis.slot_panel(img, seg=seg, hw=model.visual_resolution, recon=rows, recon_nhwc4=nhwc4, gt=gt, tiles=tiles,
                         G=len(idx))
    log['val/recon'] = _np_image(pic)


def _sample_savi_diffusion(method, model, dm, log, epoch_end, last_epoch):
    """SAViDiffusionMethod._sample_video (video_based/method.py:371-485) without the intermediate-row grids.  The slots
    are walked with encode_stream, so they carry across the chunks of val_batch_size * 4 frames (the reference restarts
    the recurrence at every chunk, only to bound memory)."""
    vs, P = dm.val_set, method.params
    kw = dict(_pget(P, 'val_sampler_kwargs', None) or {})
    n_frames = _pget(P, 'n_sample_frames')
    with_recon = epoch_end or last_epoch
    if with_recon:
        idx = sample_indices(_pget(P, 'val_batch_size'), len(vs.files))
        batch = _collate([_clip(vs, i, n_frames) for i in idx], model.device, keys=('img',))
        B, T = batch['img'].shape[:2]
        x_T, _ = _x_T(method, model, B * T, salt=1)
        samples = model.log_images(batch, use_dpm=True, x_T=x_T, **kw)['samples']
        log['val/dpm_sample_video_recon_loss'] = float(torch.nn.functional.mse_loss(samples.float(),
                                                                                    batch['img'].float()))
    idx = sample_indices(_pget(P, 'n_samples'), len(vs.files))
    clip_len = int(_pget(P, 'val_batch_size')) * 4
    hw = model.visual_resolution
    ncls = num_cls(P, model)
    bufs = band = gbuf = gband = rbuf = rband = None
    for v, i in enumerate(idx):
        d = vs.get_video(int(i))
        video = torch.as_tensor(d['video']).float().to(model.device)              # [T, 3, H, W]
        T, _, H, W = video.shape
        prev, segs, recons = None, [], []
        for t0 in range(0, T, clip_len):
            chunk = video[None, t0:t0 + clip_len]
            slots, seg = model.encode_stream(chunk, prev, want_seg=True)          # [1, Tc, N, D], [Tc, 1, h*w, N]
            prev = slots[:, -1]
            segs.append(seg[:, 0])
            if with_recon:                       # the same initial noise for all frames (temporal consistency)
                x_T, dec = _x_T(method, model, slots.shape[1], same_noise=True, salt=2)
                rows, nhwc4 = dec.sample_rows({'img': chunk[0], 'slots': slots[0]}, use_dpm=True, x_T=x_T, **kw)
                recons.append(rows)
        seg = torch.cat(segs, 0).contiguous()
        N = seg.shape[2]
        if bufs is None:
            _, GH, GW = vis.panel_geometry(T, N, 3, H, W, 1)
            bufs, band = _stack_videos(T, len(idx), GH, GW, model.device, 2)
        vis.slot_panel(video, seg=seg, hw=hw, tiles=('img', 'color', 'overlay'), G=1, hard=True, out=band(v))
        if 'masks' in d:
            if gbuf is None:
                _, GH, GW = vis.panel_geometry(T, ncls, 3, H, W, 1)
                gbuf, gband = _stack_videos(T, len(idx), GH, GW, model.device)
            vis.slot_panel(video, ids=torch.as_tensor(d['masks']).to(model.device), num_classes=ncls,
                           tiles=('img', 'color', 'overlay'), G=1, out=gband(v)[0])
        if with_recon:
            if rbuf is None:
                _, GH, GW = vis.panel_geometry(T, N, 4, H, W, 1)
                rbuf, rband = _stack_videos(T, len(idx), GH, GW, model.device)
            vis.slot_panel(video, seg=seg, hw=hw, recon=torch.cat(recons, 0), recon_nhwc4=nhwc4,
                           tiles=('img', 'recon', 'color', 'overlay'), G=1, out=rband(v)[0])
    log['val/masked_video'] = bufs[0].cpu().numpy()
    log['val/hard_masked_video'] = bufs[1].cpu().numpy()
    if gbuf is not None:
        log['val/gt_masked_video'] = gbuf[0].cpu().numpy()
    if rbuf is not None:
        log['val/video'] = rbuf[0].cpu().numpy()


def _samples(method, model, dm, log, epoch_end, last_epoch):
    from . import models as M
    if isinstance(model, getattr(M, 'LDMSlotFormer', ())):
        return                                      # metric averages only
    if isinstance(model, M.SAViDiffusion):
        model.testing = True
        _sample_savi_diffusion(method, model, dm, log, epoch_end, last_epoch)
    elif isinstance(model, M.SADiffusion):
        model.testing = True
        _sample_sa_diffusion(method, model, dm, log, epoch_end)
    elif isinstance(model, M.SAVi):
        _sample_savi(method, model, dm, log)
    elif isinstance(model, M.SA):
        _sample_sa(method, model, dm, log)


# ------------------------------------------------------------------------------------------
# the pass
# ------------------------------------------------------------------------------------------
def _batch_size(batch):
    for v in batch.values():
        if torch.is_tensor(v):
            return int(v.shape[0])
    return 1


def run_validation(method, san_check_step=-1, sample=True):
    """Method.validate's body: see there."""
    model, dm = method.model, method.datamodule
    epoch_end = san_check_step <= 0
    last_epoch = getattr(method, 'epoch', 0) == _pget(method.params, 'max_epochs')
    log = {}
    with _Untouched(model), torch.no_grad():
        model.eval()
        fresh = getattr(model, 'weights_updated', None)
        if fresh is not None:       # the inference operands are made from the weights of the step just taken
            if method.optimizer is not None:
                fresh(shadow_fresh=True)        # (the fused update keeps the bf16 shadow current itself)
            else:
                fresh()
        dist = torch.distributed
        if 'shard' in getattr(dm, '__dict__', {}):      # (WithValidation: sharded exactly when the sums are reduced)
            dm.shard = (dist.get_rank(), dist.get_world_size()) if method.use_ddp else None
        sums, count = {}, 0
        for bi, batch in enumerate(dm.val_loader()):
            if san_check_step > 0 and bi >= san_check_step:
                break
            losses = model.calc_eval_loss(batch, model(batch))
            bs = _batch_size(batch)
            for k, v in losses.items():
                v = torch.as_tensor(v).detach().double().reshape(())
                sums[k] = v * bs if k not in sums else sums[k] + v * bs
            count += bs
        keys = sorted(sums)
        dev = sums[keys[0]].device if keys else getattr(model, 'device', 'cpu')
        if method.use_ddp:
            # a rank may have seen fewer batches than another, or none (fewer batches than ranks, a san check): all
            # ranks first agree on the union of the keys, and a rank adds zero for a key it did not see
            seen = [None] * dist.get_world_size()
            dist.all_gather_object(seen, keys)
            keys = sorted(set().union(*seen))
        if keys:
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            packed = torch.stack([sums[k].to(dev) if k in sums else zero for k in keys] +
                                 [torch.tensor(float(count), dtype=torch.float64, device=dev)])
            if method.use_ddp:       # the per-key sums and the count in one tensor
                dist.all_reduce(packed)
            packed = packed.cpu()
            total = float(packed[-1])
            for j, k in enumerate(keys):
                log[f'val/{k}'] = float(packed[j]) / total if total > 0 else float('nan')
        if sample and method.local_rank == 0 and getattr(dm, 'val_set', None) is not None:
            _samples(method, model, dm, log, epoch_end, last_epoch)
    method.log_fn(log, step=method.it)
    return log
