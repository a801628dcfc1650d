"""Method.validate and the validation hooks of Method.fit on the GPU: the logged dictionaries with the fused panel
launch and with the composed path are identical, floats and bytes alike (SA, SAVi, SADiffusion, SAViDiffusion); validating
while training leaves the weight arena and the loss history bit for bit what training alone leaves (eager and graphed
steps); and a validation pass sees the weights of the step just taken (it equals that of a fresh model loaded from the
checkpoint).  128 x 128 is the smallest configuration tests/common.py offers; the samplers run 2 steps."""
import numpy as np
import pytest
import torch

from slotdiffusion_amd import validate as V
from slotdiffusion_amd import vis
from slotdiffusion_amd.extract import SyntheticVideoSegDataset
from slotdiffusion_amd.method import Method, SyntheticDataModule
from tests import common as C
from tests.detfill import det_fill_, is_buffer_name

pytestmark = pytest.mark.gpu
SAMPLER = dict(dpm_steps=2)


def _params(model, **kw):
    if model == 'SAVi':
        P = C.Params(model=model, optimizer='Adam', weight_decay=0.0, max_epochs=1, train_batch_size=1, dataset='clevrtex',
                     san_check_val_step=0, lr=2e-4, clip_grad=0.05, warmup_steps_pct=0.025, img_recon_loss_w=1.,
                     input_frames=2, n_sample_frames=2, **{k: v for k, v in C.savi_cfg().items() if k != 'clip_len'})
    elif model == 'SAViDiffusion':
        P = C.Params(model=model, optimizer='Adam', weight_decay=0.0, max_epochs=1, train_batch_size=1, dataset='clevrtex',
                     san_check_val_step=0, lr=1e-4, dec_lr=2e-4, clip_grad=0.05, warmup_steps_pct=0.05, denoise_loss_w=1.,
                     input_frames=2, n_sample_frames=2, **C.movie_cfg())
        kw = dict(dict(val_batch_size=1), **kw)          # sampled videos walk in chunks of 4 frames: 6 = 4 + 2
    else:
        P = C.make_params(model, batch=2)
    P.__dict__.update(dict(dict(n_samples=2, val_batch_size=2, eval_interval=1, val_sampler_kwargs=SAMPLER), **kw))
    return P


def _method(model, dtype='fp32', **kw):
    from slotdiffusion_amd.models import build_model
    P = _params(model, **kw)
    m = build_model(P)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    m = m.cuda()
    m.set_compute_dtype(dtype)
    if model in ('SAVi', 'SAViDiffusion'):
        dm = V.WithValidation(SyntheticDataModule(P, steps_per_epoch=2, frames=2),
                              SyntheticVideoSegDataset(P, num_videos=2, video_len=6), batch_size=1)
    else:
        dm = V.WithValidation(SyntheticDataModule(P, steps_per_epoch=2), V.SyntheticImageSegDataset(P, num_images=4))
    return Method(m, dm, P)


def _same_logs(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == np.uint8 and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        else:
            assert isinstance(a[k], float) and a[k] == b[k], (k, a[k], b[k])


WANT = {
    'SA': ({'val/img_recon_loss', 'val/ari', 'val/fari', 'val/miou', 'val/fmiou', 'val/mbo', 'val/imgs'},
           {'val/imgs': (2 * 130 + 2, (2 + 7) * 130 + 2, 3)}),
    'SAVi': ({'val/img_recon_loss', 'val/ari', 'val/fari', 'val/miou', 'val/fmiou', 'val/mbo', 'val/video'},
             {'val/video': (6, 3, 2 * 132, (4 + 15) * 130 + 2)}),
    'SADiffusion': ({'val/denoise_loss', 'val/dpm_sample_img_recon_loss', 'val/recon'},
                    {'val/recon': (2 * 130 + 2, (5 + 7) * 130 + 2, 3)}),
    'SAViDiffusion': ({'val/denoise_loss', 'val/dpm_sample_video_recon_loss', 'val/masked_video',
                       'val/hard_masked_video', 'val/gt_masked_video', 'val/video'},
                      {'val/masked_video': (6, 3, 2 * 132, (3 + 15) * 130 + 2),
                       'val/hard_masked_video': (6, 3, 2 * 132, (3 + 15) * 130 + 2),
                       'val/gt_masked_video': (6, 3, 2 * 132, (3 + 15) * 130 + 2),
                       'val/video': (6, 3, 2 * 132, (4 + 15) * 130 + 2)}),
}


@pytest.mark.parametrize('model', ['SA', 'SAVi', 'SADiffusion', 'SAViDiffusion'])
def test_validate_fused_and_composed_give_identical_logs(model, monkeypatch):
    meth = _method(model)
    composed = []
    orig = vis.slot_panel_composed
    monkeypatch.setattr(vis, 'slot_panel_composed', lambda *a, **k: (composed.append(1), orig(*a, **k))[1])
    logs = []
    for fused in (True, False):
        monkeypatch.setattr(vis, '_PANEL_FUSED', fused)
        meth.model.eval_seed = None                       # both passes draw the same evaluation t / noise
        n0 = len(composed)
        logs.append(meth.validate())
        assert (len(composed) > n0) is (not fused)         # every panel inside the gate: one launch each
    keys, shapes = WANT[model]
    assert set(logs[0]) == keys
    for k, s in shapes.items():
        assert logs[0][k].shape == s, (k, logs[0][k].shape)
        assert int(logs[0][k].min()) == 0 and int(logs[0][k].max()) > 0              # padding is byte 0; not blank
    _same_logs(logs[0], logs[1])
    assert [s for s, _ in meth.val_history] == [0, 0] and meth.model.training and not meth.model.testing


@pytest.mark.parametrize('graph', [False, True])
def test_fit_with_validation_leaves_training_bit_for_bit(graph):
    runs = []
    for validating in (False, True):
        meth = _method('SADiffusion', dtype='bf16', max_epochs=2)
        meth.use_graph = graph
        if not validating:
            meth.datamodule = meth.datamodule._dm          # the bare datamodule: no val_loader
        meth.fit(san_check_val_step=1 if validating else 0)
        torch.cuda.synchronize()
        runs.append((meth.model.arena().detach().clone(), torch.stack([h.detach().float().reshape(()) for h in meth.history]),
                     meth))
    assert runs[0][2].it == runs[1][2].it == 4 and runs[0][2].val_history == []
    assert [s for s, _ in runs[1][2].val_history] == [0, 2, 4]
    assert 'val/recon' in runs[1][2].val_history[-1][1]
    assert torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][0], runs[1][0])


@pytest.mark.parametrize('graph', [False, True])
def test_validation_sees_the_weights_of_the_step_just_taken(graph, tmp_path):
    meth = _method('SADiffusion', dtype='bf16', max_epochs=1)
    meth.use_graph = graph
    meth.validate(sample=False)                            # builds the inference operands of the INITIAL weights
    first = meth.val_history[-1][1]['val/denoise_loss']
    meth.datamodule, dm = meth.datamodule._dm, meth.datamodule
    meth.fit()                                             # 2 steps, no validation
    meth.datamodule = dm
    meth.model.eval_seed = None
    after = meth.validate(sample=False)['val/denoise_loss']
    path = str(tmp_path / 'ckp.pth')
    meth.save(path)
    fresh = _method('SADiffusion', dtype='bf16', max_epochs=1)
    fresh.model.load_weight(path)
    fresh.model.eval_seed = None
    alone = fresh.validate(sample=False)['val/denoise_loss']
    assert after == alone and after != first
