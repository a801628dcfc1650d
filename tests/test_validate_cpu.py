"""The validation pass without a GPU: the sample-index rule, the palette, the composed panel builder byte for byte
against numpy restatements of the reference's four builders (make_grid and the truncating byte conversion included), the
argument refusals of sdmi_slot_panel and its Python gate, and Method.validate / the hooks of Method.fit on a stub model
and datamodule (averaging, san-check stop, schedule, log keys and shapes, restored flags and RNG states), with a 2-rank
gloo run of the metric reduction."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from slotdiffusion_amd import _lib, vis
from slotdiffusion_amd import validate as V
from slotdiffusion_amd.method import Method
from tests import common as C


# ----------------------------------------------------------------------------------------------------------------------
# sample_indices, palette
# ----------------------------------------------------------------------------------------------------------------------
def _ref_sample_idx(N, dst_len):            # img_based/method.py:46-53 with len(dst) = dst_len
    if N > dst_len:
        N = dst_len
    N = N - 1 if dst_len % N != 0 else N
    return np.arange(0, dst_len, dst_len // N)


def test_sample_indices_is_the_reference_rule():
    for n in range(1, 10):
        for length in range(1, 41):
            assert np.array_equal(V.sample_indices(n, length), _ref_sample_idx(n, length)), (n, length)
    assert len(V.sample_indices(8, 10)) == 10 and len(V.sample_indices(2, 3)) == 1


def test_palette_equals_the_fixture():
    with open(os.path.join(C.GOLD, 'vis_palette.json')) as f:
        fix = json.load(f)['palette']
    assert vis.PALETTE == fix and len(fix) == 20
    ref = torch.from_numpy(np.array(fix) / 255.0).float() * 2. - 1.
    assert torch.equal(vis.torch_palette(), ref) and vis.torch_palette().dtype == torch.float32


# ----------------------------------------------------------------------------------------------------------------------
# numpy restatements of the reference's builders
# ----------------------------------------------------------------------------------------------------------------------
def _np_palette():
    return (np.array(vis.PALETTE) / 255.0).astype(np.float32) * np.float32(2.) - np.float32(1.)


def _np_make_grid(tiles, nrow, padding=2, pad_value=-1.):
    n, Cc, H, W = tiles.shape
    xmaps = min(nrow, n)
    ymaps = int(np.ceil(n / xmaps))
    hh, ww = H + padding, W + padding
    grid = np.full((Cc, hh * ymaps + padding, ww * xmaps + padding), pad_value, dtype=np.float32)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= n:
                break
            grid[:, y * hh + padding:y * hh + padding + H, x * ww + padding:x * ww + padding + W] = tiles[k]
            k += 1
    return grid


def _np_convert(x):
    return ((x * np.float32(0.5) + np.float32(0.5)).clip(0, 1) * np.float32(255.)).astype(np.uint8)


def _np_draw_rgb_mask(rgb, mask, alpha=0.7):
    col = np.moveaxis(_np_palette()[mask], -1, 1)
    return rgb * np.float32(alpha) + col * np.float32(1. - alpha), col


def _np_make_img_grid(imgs, recon_combined, recons, masks):          # SAMethod._make_img_grid
    out = np.concatenate([imgs[:, None], recon_combined[:, None], recons * masks + (np.float32(1.) - masks)], axis=1)
    return _np_make_grid(out.reshape((-1,) + out.shape[2:]), nrow=out.shape[1])


def _np_make_video_grid(imgs, recon_combined, recons, masks):        # SAViMethod._make_video_grid
    rgb_mask, colored = _np_draw_rgb_mask(imgs, masks[:, :, 0].argmax(1))
    out = np.concatenate([imgs[:, None], recon_combined[:, None], colored[:, None], rgb_mask[:, None],
                          recons * masks + (np.float32(1.) - masks)], axis=1)
    return np.stack([_np_make_grid(out[i], nrow=out.shape[1]) for i in range(out.shape[0])])


def _np_slot_list(imgs, recon, masks):
    rgb_mask, colored = _np_draw_rgb_mask(imgs, masks.argmax(1))
    masked = imgs[:, None] * masks[:, :, None] + (np.float32(1.) - masks[:, :, None])
    lst = [imgs[:, None], colored[:, None], rgb_mask[:, None], masked]
    if recon is not None:
        lst.insert(1, recon[:, None])
    return lst


def _np_make_slots_img(imgs, recon, masks, gt_masks=None):           # SADiffusionMethod._make_slots_img
    lst = _np_slot_list(imgs, recon, masks)
    if gt_masks is not None:
        lst.insert(2, _np_draw_rgb_mask(imgs, gt_masks)[1][:, None])
    out = np.concatenate(lst, axis=1)
    return _np_make_grid(out.reshape((-1,) + out.shape[2:]), nrow=out.shape[1])


def _np_make_slots_video(video, recon, masks):                       # SAViDiffusionMethod._make_slots_video
    out = np.concatenate(_np_slot_list(video, recon, masks), axis=1)
    return np.stack([_np_make_grid(out[i], nrow=out.shape[1]) for i in range(out.shape[0])])


def _np_one_hot(masks):
    idx = masks.argmax(1)
    return np.moveaxis(np.eye(masks.shape[1], dtype=np.float32)[idx], -1, 1)


F_, N_, H_, W_ = 3, 4, 6, 10


def _data(seed=0):
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(F_, 3, H_, W_, generator=g) * 2.4 - 1.2            # some values beyond [-1, 1]: the clamp
    recon = torch.rand(F_, 3, H_, W_, generator=g) * 2 - 1
    masks = torch.softmax(torch.randn(F_, N_, H_, W_, generator=g) * 2, 1)
    masks[0, :, 0, 0] = 0.25                                             # a tie: the lowest index wins
    recons = torch.rand(F_, N_, 3, H_, W_, generator=g) * 2 - 1
    gt = torch.randint(0, 20, (F_, H_, W_), generator=g)
    return img, recon, masks, recons, gt


def test_panel_bytes_sa_image_grid():
    img, recon, masks, recons, _ = _data(1)
    got = vis.slot_panel_composed(img, masks=masks, recon=recon, slot_img=recons, tiles=('img', 'recon'), G=F_)
    ref = _np_convert(_np_make_img_grid(img.numpy(), recon.numpy(), recons.numpy(), masks.unsqueeze(2).numpy()))
    assert got.shape == (1, 3, F_ * (H_ + 2) + 2, (2 + N_) * (W_ + 2) + 2) and got.dtype == torch.uint8
    assert np.array_equal(got[0].numpy(), ref)
    assert vis.panel_geometry(F_, N_, 2, H_, W_, F_) == tuple(got.shape[:1]) + tuple(got.shape[2:])


def test_panel_bytes_savi_video_grid():
    img, recon, masks, recons, _ = _data(2)
    got = vis.slot_panel_composed(img, masks=masks, recon=recon, slot_img=recons,
                                  tiles=('img', 'recon', 'color', 'overlay'), G=1)
    ref = _np_convert(_np_make_video_grid(img.numpy(), recon.numpy(), recons.numpy(), masks.unsqueeze(2).numpy()))
    assert got.shape == (F_, 3, H_ + 4, (4 + N_) * (W_ + 2) + 2)
    assert np.array_equal(got.numpy(), ref)


@pytest.mark.parametrize('with_recon', [False, True])
@pytest.mark.parametrize('with_gt', [False, True])
def test_panel_bytes_slots_img(with_recon, with_gt):
    img, recon, masks, _, gt = _data(3)
    # the reference inserts the GT tile at index 2 AFTER the recon tile went in at index 1
    tiles = ('img', 'recon') if with_recon else ('img',)
    tiles += (('gtcolor', 'color') if with_recon else ('color', 'gtcolor')) if with_gt else ('color',)
    tiles += ('overlay',)
    got = vis.slot_panel_composed(img, masks=masks, recon=recon if with_recon else None, gt=gt if with_gt else None,
                                  tiles=tiles, G=F_)
    ref = _np_convert(_np_make_slots_img(img.numpy(), recon.numpy() if with_recon else None, masks.numpy(),
                                         gt.numpy() if with_gt else None))
    assert got.shape == (1, 3, F_ * (H_ + 2) + 2, (len(tiles) + N_) * (W_ + 2) + 2)
    assert np.array_equal(got[0].numpy(), ref)
    # the wrapper on host tensors is the composed path
    assert torch.equal(vis.slot_panel(img, masks=masks, recon=recon if with_recon else None,
                                      gt=gt if with_gt else None, tiles=tiles, G=F_), got)


@pytest.mark.parametrize('with_recon', [False, True])
def test_panel_bytes_slots_video_soft_hard_and_gt(with_recon):
    img, recon, masks, _, gt = _data(4)
    tiles = ('img', 'recon', 'color', 'overlay') if with_recon else ('img', 'color', 'overlay')
    r = recon if with_recon else None
    soft, hard = vis.slot_panel_composed(img, masks=masks, recon=r, tiles=tiles, G=1, hard=True)
    rn = recon.numpy() if with_recon else None
    assert soft.shape == (F_, 3, H_ + 4, (len(tiles) + N_) * (W_ + 2) + 2)
    assert np.array_equal(soft.numpy(), _np_convert(_np_make_slots_video(img.numpy(), rn, masks.numpy())))
    assert np.array_equal(hard.numpy(), _np_convert(_np_make_slots_video(img.numpy(), rn, _np_one_hot(masks.numpy()))))
    # the ground-truth panel: F.one_hot(gt, num_cls) as the masks
    got = vis.slot_panel_composed(img, ids=gt, num_classes=20, recon=r, tiles=tiles, G=1)
    onehot = np.moveaxis(np.eye(20, dtype=np.float32)[gt.numpy()], -1, 1)
    assert np.array_equal(got.numpy(), _np_convert(_np_make_slots_video(img.numpy(), rn, onehot)))
    # an attention map [F, h*w, N] at h == H is the same panel as its planar form: the upsample returns the source
    seg = masks.flatten(2).permute(0, 2, 1).contiguous()
    assert torch.equal(vis.slot_panel_composed(img, seg=seg, hw=(H_, W_), recon=r, tiles=tiles, G=1), soft)


def test_out_of_range_ids_draw_byte_zero_and_no_slot():
    img, _, _, _, gt = _data(5)
    ids = gt.clone() % 5
    ids[0, 0, 0], ids[1, 2, 3] = 7, -1
    gt2 = gt.clone()
    gt2[2, 1, 1] = 20
    got = vis.slot_panel_composed(img, ids=ids, num_classes=5, gt=gt2, tiles=('color', 'overlay', 'gtcolor'), G=1)
    for f, y, x in ((0, 0, 0), (1, 2, 3)):
        for j in range(2):
            assert (got[f, :, 2 + y, 2 + j * (W_ + 2) + x] == 0).all()
        for k in range(5):                                    # white in every slot tile: s * 0 + 1
            assert (got[f, :, 2 + y, 2 + (3 + k) * (W_ + 2) + x] == 255).all()
    assert (got[2, :, 2 + 1, 2 + 2 * (W_ + 2) + 1] == 0).all()


def test_save_panels_writes_pngs(tmp_path):
    from PIL import Image
    log = {'val/imgs': np.full((5, 7, 3), 9, np.uint8), 'val/video': np.zeros((2, 3, 4, 6), np.uint8), 'val/loss': 0.5}
    files = vis.save_panels(str(tmp_path), log)
    assert sorted(os.path.relpath(f, tmp_path) for f in files) == ['val_imgs.png', 'val_video/0000.png', 'val_video/0001.png']
    assert Image.open(files[0]).size == (7, 5) and Image.open(files[1]).size == (6, 4)


# ----------------------------------------------------------------------------------------------------------------------
# the entry point refuses bad arguments before any launch; the Python gate mirrors it
# ----------------------------------------------------------------------------------------------------------------------
def test_slot_panel_rejects_bad_arguments_without_launch():
    GW, GH = (3 + 5) * 26 + 2, 18 + 2
    ok = dict(img=64, recon=128, seg=256, gt=320, palette=384, soft=448, hard=512, F=6, G=1, N=5, P=20, H=16, W=24, h=4,
              w=6, nprefix=3, tiles=0x320, img_stride=3 * GH * GW, ch_stride=GH * GW, row_stride=GW)
    bad = [dict(img=0), dict(soft=0), dict(seg=0), dict(ids=64),                      # pointers; none / both mask sources
           dict(N=0), dict(H=0), dict(W=0), dict(h=0), dict(w=0), dict(F=0), dict(G=0), dict(G=4),
           dict(nprefix=9), dict(nprefix=-1), dict(tiles=0x325), dict(tiles=0x321, recon=0), dict(tiles=0x324, gt=0),
           dict(palette=0), dict(P=4), dict(P=0), dict(img_nhwc4=2), dict(seg_planar=-1), dict(seg=260),
           dict(row_stride=GW - 1), dict(ch_stride=GH * GW - 1), dict(img_stride=3 * GH * GW - 1), dict(img_stride=-1)]
    for over in bad:
        with pytest.raises(_lib.SdmiError, match='sdmi_slot_panel'):
            _lib.call('sdmi_slot_panel', None, **dict(ok, **over))
        assert b'sdmi_slot_panel' in _lib.lib().sdmi_last_error(), over
    # panel rows too wide for the LDS copy of even one band row: refused as unsupported
    W = 8192
    GW = 8 * (W + 2) + 2
    with pytest.raises(_lib.SdmiError, match=r'sdmi_slot_panel failed \(-3\)'):
        _lib.call('sdmi_slot_panel', None, **dict(ok, W=W, img_stride=3 * GH * GW, ch_stride=GH * GW, row_stride=GW))
    assert not vis.slot_panel_covers(5, 3, 16, W, 4, 6)


@pytest.mark.parametrize('args,want', [
    ((15, 3, 128, 128, 32, 32), 8), ((15, 4, 128, 128, 32, 32), 8),          # MOVi-E
    ((24, 5, 128, 128, 128, 128), 4), ((24, 8, 224, 224, 28, 28), 4),        # the widest configured shapes
    ((24, 8, 224, 224, 128, 128), 4), ((5, 3, 16, 24, 4, 6), 8), ((3, 2, 11, 13, 11, 13), 8), ((5, 3, 3, 24, 4, 6), 2),
    ((5, 3, 16, 4096, 4, 6), 1), ((5, 3, 16, 8192, 4, 6), 0), ((4000, 0, 8, 8, 64, 64), 0)])
def test_slot_panel_band_and_gate(args, want):
    assert vis.slot_panel_band(*args) == want
    assert vis.slot_panel_covers(*args, colour=False) is (want > 0)


def test_slot_panel_covers_argument_rules():
    assert vis.slot_panel_covers(20, 3, 16, 16, 16, 16, False) and not vis.slot_panel_covers(21, 3, 16, 16, 16, 16, False)
    assert vis.slot_panel_covers(21, 1, 16, 16, 16, 16, False, colour=False)
    assert not vis.slot_panel_covers(0, 3, 16, 16, 4, 4) and not vis.slot_panel_covers(5, 9, 16, 16, 4, 4)
    assert not vis.slot_panel_covers(5, 3, 0, 16, 4, 4) and not vis.slot_panel_covers(5, 3, 16, 16, 4, 0)


# ----------------------------------------------------------------------------------------------------------------------
# Method.validate and the hooks of Method.fit on a stub model and datamodule
# ----------------------------------------------------------------------------------------------------------------------
class StubModel:
    """eval loss of a batch = the mean of its 'x'; records what validation did to it."""

    def __init__(self):
        self.training, self.testing, self.calls, self.refreshed, self.modes = True, False, 0, [], []

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def __call__(self, batch):
        self.calls += 1
        self.modes.append((self.training, torch.is_grad_enabled()))
        torch.rand(3)                                           # a model that draws from the global generator
        return {'y': batch['x']}

    def calc_eval_loss(self, batch, out):
        return {'loss_a': out['y'].mean(), 'loss_b': out['y'].sum()}

    def weights_updated(self, shadow_fresh=False):
        self.refreshed.append(shadow_fresh)

    def _training_step_end(self, method=None):
        pass


class StubData:
    def __init__(self, params, sizes=(4, 4, 2), steps=2):
        self.params, self.sizes, self.steps = params, sizes, steps

    def __len__(self):
        return self.steps

    def train_loader(self, epoch=0):
        for i in range(self.steps):
            yield {'x': torch.full((2,), float(i))}

    def batches(self):
        return [torch.arange(n, dtype=torch.float32) + 10 * i for i, n in enumerate(self.sizes)]

    def val_loader(self):
        for x in self.batches():
            yield {'x': x}


class StubTrainOnly(StubData):
    val_loader = property()            # no validation side: hasattr(dm, 'val_loader') is False


class StubMethod(Method):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.use_graph = False
        self.validated = []

    def _configure_optimizers(self):
        return object()

    def _eager_step(self, batch):
        return torch.zeros(())

    def validate(self, san_check_step=-1, sample=True):
        self.validated.append((self.it, self.epoch, san_check_step))
        return super().validate(san_check_step, sample)


def _params(**kw):
    return C.Params(**dict(dict(max_epochs=4, eval_interval=2, n_samples=2, val_batch_size=4), **kw))


def test_validate_averages_weighted_by_batch_size_and_stops_at_san_check():
    p = _params()
    dm = StubData(p)
    m = StubMethod(StubModel(), dm, p)
    log = m.validate()
    xs = dm.batches()
    n = sum(len(x) for x in xs)
    assert log['val/loss_a'] == pytest.approx(sum(float(x.mean()) * len(x) for x in xs) / n, abs=1e-12)
    assert log['val/loss_b'] == pytest.approx(sum(float(x.sum()) * len(x) for x in xs) / n, abs=1e-12)
    assert log['val/loss_a'] != pytest.approx(sum(float(x.mean()) for x in xs) / len(xs))      # not the plain mean
    assert m.val_history == [(0, log)] and m.model.calls == 3
    assert m.model.modes == [(False, False)] * 3                       # eval mode, no gradients
    log2 = m.validate(san_check_step=2)
    assert m.model.calls == 5
    assert log2['val/loss_a'] == pytest.approx(sum(float(x.mean()) * len(x) for x in xs[:2]) / 8, abs=1e-12)
    got = []
    m.log_fn = lambda d, step: got.append((step, d))
    m.it = 7
    m.validate()
    assert got[0][0] == 7 and set(got[0][1]) == {'val/loss_a', 'val/loss_b'} and len(m.val_history) == 2


def test_validate_restores_flags_and_rng_states():
    p = _params()
    m = StubMethod(StubModel(), StubData(p), p)
    for training, testing in ((True, False), (False, True)):
        m.model.training, m.model.testing = training, testing
        torch.manual_seed(5)
        want = torch.rand(4)
        torch.manual_seed(5)
        m.validate()
        assert torch.equal(torch.rand(4), want)
        assert (m.model.training, m.model.testing) == (training, testing)
    assert m.model.refreshed == [False, False]                  # no optimiser yet: a full refresh of the operands
    m.optimizer = object()
    m.validate()
    assert m.model.refreshed[-1] is True


def test_fit_schedule_follows_eval_interval_last_epoch_and_max_steps():
    p = _params(max_epochs=5, eval_interval=2)
    m = StubMethod(StubModel(), StubData(p), p).fit()
    assert m.validated == [(4, 2, -1), (8, 4, -1), (10, 5, -1)]          # epochs 2, 4 and the last one
    m = StubMethod(StubModel(), StubData(p), p).fit(san_check_val_step=2)
    assert m.validated[0] == (0, 0, 2) and len(m.validated) == 4 and m.model.calls == 2 + 3 * 3
    m = StubMethod(StubModel(), StubData(p), p).fit(max_steps=4)          # returns inside epoch 2: nothing validated
    assert m.validated == [] and m.it == 4
    m = StubMethod(StubModel(), StubData(p), p).fit(max_steps=5)
    assert m.validated == [(4, 2, -1)]
    p1 = _params(max_epochs=2, eval_interval=1)
    assert StubMethod(StubModel(), StubData(p1), p1).fit().validated == [(2, 1, -1), (4, 2, -1)]


def test_datamodule_without_val_loader_is_never_validated():
    p = _params(max_epochs=2, eval_interval=1)
    dm = StubTrainOnly(p)
    assert not hasattr(dm, 'val_loader')
    m = StubMethod(StubModel(), dm, p).fit(san_check_val_step=3)
    assert m.validated == [] and m.val_history == [] and m.it == 4 and m.model.calls == 0


class _ImgStubModel(StubModel):
    def __call__(self, batch):
        self.calls += 1
        return {'y': batch['img']}


def test_with_validation_wraps_a_datamodule():
    p = _params(resolution=(8, 12), val_batch_size=3, n_sample_frames=2, train_batch_size=2)
    inner = StubData(p)
    inner.device = 'cpu'
    vs = V.SyntheticImageSegDataset(p, num_images=7)
    dm = V.WithValidation(inner, vs)
    assert len(dm) == len(inner) and dm.params is p and dm.val_set is vs
    assert [b['x'].tolist() for b in dm.train_loader(0)] == [b['x'].tolist() for b in inner.train_loader(0)]
    sizes = [(tuple(b['img'].shape), tuple(b['masks'].shape)) for b in dm.val_loader()]
    assert sizes == [((3, 3, 8, 12), (3, 8, 12)), ((3, 3, 8, 12), (3, 8, 12)), ((1, 3, 8, 12), (1, 8, 12))]
    first = next(iter(dm.val_loader()))
    assert torch.equal(first['img'][1], vs[1]['img']) and int(first['masks'].max()) <= 4
    assert torch.equal(vs[3]['img'], vs[3]['img']) and not torch.equal(vs[3]['img'], vs[4]['img'])
    # videos: the first n_sample_frames frames of each, batch_size videos per batch
    from slotdiffusion_amd.extract import SyntheticVideoSegDataset
    vv = SyntheticVideoSegDataset(p, num_videos=3, video_len=5)
    dv = V.WithValidation(inner, vv, batch_size=2)
    shapes = [(tuple(b['img'].shape), tuple(b['masks'].shape)) for b in dv.val_loader()]
    assert shapes == [((2, 2, 3, 8, 12), (2, 2, 8, 12)), ((1, 2, 3, 8, 12), (1, 2, 8, 12))]
    m = StubMethod(_ImgStubModel(), dm, p)
    log = m.validate()                    # a stub model is no slot model: metric averages only, val_set or not
    assert set(log) == {'val/loss_a', 'val/loss_b'} and m.model.calls == 3


# ----------------------------------------------------------------------------------------------------------------------
# two gloo ranks: the sums and the count are reduced, not the per-rank averages
# ----------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _val_worker(rank, world, port, ret):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        p = _params()
        dm = StubData(p, sizes=(4, 1) if rank == 0 else (3,))
        m = StubMethod(StubModel(), dm, p, local_rank=rank, use_ddp=True)
        a = m.validate()
        # fewer batches than ranks: rank 1 sees none and still joins the reduction with the other rank's keys
        m = StubMethod(StubModel(), StubData(p, sizes=(4,) if rank == 0 else ()), p, local_rank=rank, use_ddp=True)
        b = m.validate()
        # WithValidation is sharded by the validating method: rank r takes batches r, r + world, ... of 3 + 3 + 1 images
        pi = _params(resolution=(8, 12), val_batch_size=3)
        inner = StubData(pi)
        inner.device = 'cpu'
        dm = V.WithValidation(inner, V.SyntheticImageSegDataset(pi, num_images=7))
        m = StubMethod(_ImgStubModel(), dm, pi, local_rank=rank, use_ddp=True)
        c = m.validate()
        ret[rank] = (a, b, c, m.model.calls, dm.shard)
    finally:
        dist.destroy_process_group()


def test_metric_reduction_two_ranks_gloo():
    world, port = 2, _free_port()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_val_worker, args=(world, port, ret), nprocs=world, join=True)
        r = dict(ret)
    p = _params()
    xs = StubData(p, sizes=(4, 1)).batches() + StubData(p, sizes=(3,)).batches()
    want = sum(float(x.mean()) * len(x) for x in xs) / 8
    assert r[0][0] == r[1][0] and r[0][0]['val/loss_a'] == pytest.approx(want, abs=1e-12)
    x = StubData(p, sizes=(4,)).batches()[0]
    assert r[0][1] == r[1][1] and r[0][1] == {'val/loss_a': pytest.approx(float(x.mean())), 'val/loss_b': pytest.approx(float(x.sum()))}
    # the sharded pass equals the unsharded one of a single process (whose shard stays None), and the ranks split 2 + 1
    pi = _params(resolution=(8, 12), val_batch_size=3)
    inner = StubData(pi)
    inner.device = 'cpu'
    dm = V.WithValidation(inner, V.SyntheticImageSegDataset(pi, num_images=7))
    alone = StubMethod(_ImgStubModel(), dm, pi).validate()
    assert dm.shard is None and (r[0][3], r[1][3]) == (2, 1) and (r[0][4], r[1][4]) == ((0, 2), (1, 2))
    assert r[0][2] == r[1][2] and set(alone) == set(r[0][2])
    for k in alone:
        assert r[0][2][k] == pytest.approx(alone[k], rel=1e-12)
