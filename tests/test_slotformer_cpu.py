"""LDMSlotFormer (vp_vqa) without a GPU: registry, checkpoint keys, refusals, the CPU restatement against the
reference's fixture, and the C ABI's argument checks of sdmi_rollout_layer.  No kernel is launched here."""
import importlib

import pytest
import torch

from slotdiffusion_amd import _lib
from tests import common as C
from tests import slotformer_ref as R


@pytest.fixture(scope='module')
def shipped_model():
    return importlib.import_module('slotdiffusion.vp_vqa').build_model(R.shipped_params())


def test_build_model_keys_shapes_and_frozen_set(shipped_model):
    m = shipped_model
    assert type(m).__name__ == 'LDMSlotFormer'
    want = R.key_fixture()
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == want['state']        # names, shapes, order
    frozen = [k for k, p in m.named_parameters() if not p.requires_grad]
    assert frozen == want['frozen']
    assert 'rollouter.enc_t_pe' in frozen
    assert all(not p.requires_grad for k, p in m.named_parameters() if k.startswith('dm_decoder.'))
    assert all(p.requires_grad for k, p in m.named_parameters()
               if k.startswith('rollouter.') and k != 'rollouter.enc_t_pe')
    assert torch.equal(m.state_dict()['rollouter.enc_t_pe'], R.sin_pos_enc(15, 256))          # bit for bit
    assert m.history_len == 15 and m.rollout_len == 10 and m.num_slots == 8 and m.pred_dropout == 0.1
    m.train()
    assert m.training and not m.dm_decoder.training          # the decoder stays in eval mode
    m.eval()


def test_registry_surface_and_refusals():
    task = importlib.import_module('slotdiffusion.vp_vqa')
    P = R.shipped_params()
    P.train_batch_size = 2
    dm = task.build_dataset(P)
    assert len(dm) > 0
    batch = next(iter(type(dm)(P, device='cpu').train_loader()))
    assert tuple(batch['slots'].shape) == (2, 25, 8, 192)
    assert callable(task.build_method)
    P.model = 'PhysionReadout'
    with pytest.raises(NotImplementedError, match='PhysionReadout is not on the MI355X hot path yet'):
        task.build_model(P)
    for key in ('use_denoise_loss', 'use_img_recon_loss'):
        P = R.shipped_params(**{key: True})
        with pytest.raises(ValueError, match=key):
            task.build_model(P)
    from slotdiffusion_amd import policy
    assert policy.SWITCHES['ROLLOUT_FUSED'][0] in (0, 1)


def test_cpu_restatement_reproduces_the_reference_fixture():
    """Same torch CPU arithmetic as the reference's SlotRollouter: any difference is a restatement error (1e-5)."""
    G = C.load_golden('ldmslotformer_b2.npz')
    m = R.build()
    W = R.rollouter_weights(m)
    slots = G['slots']
    assert tuple(slots.shape) == (2, 18, 8, 192)
    with torch.no_grad():
        pred = R.rollouter_forward(W, slots[:, :15], R.ROLLOUT_LEN, 8, R.LAYERS, 8)
    loss = torch.nn.functional.mse_loss(pred, slots[:, 15:])
    assert float((pred - G['pred_slots']).abs().max()) <= 1e-5
    assert abs(float(loss) - float(G['slot_recon_loss'])) <= 1e-5
    # the fixture's gradient norms name exactly the trainable tensors
    assert [str(n) for n in G['grad_norms_names']] == sorted(k for k, p in m.named_parameters() if p.requires_grad)


def test_rollout_layer_rejects_bad_arguments_without_launch():
    ok = dict(x=16, qkv=32, out=48, wstream_a=64, vec_a=80, wstream_b=96, vec_b=112, B=2, L=120, Lp=128, C=256, heads=8,
              ffn_dim=1024, phase=0, ln_eps=1e-5, attn_scale=32.0 ** -0.5)
    bad = [dict(x=0), dict(qkv=0), dict(out=0), dict(wstream_a=0), dict(vec_b=0),       # null pointers
           dict(C=384), dict(C=128), dict(L=129), dict(Lp=320, L=300), dict(Lp=96, L=90), dict(L=0),
           dict(ffn_dim=1000), dict(ffn_dim=2048), dict(heads=4), dict(phase=3), dict(out=16)]
    for over in bad:
        kw = dict(ok, **over)
        with pytest.raises(_lib.SdmiError, match='sdmi_rollout_layer'):
            _lib.call('sdmi_rollout_layer', None, **kw)
        assert len(_lib.lib().sdmi_last_error()) > 0, over
