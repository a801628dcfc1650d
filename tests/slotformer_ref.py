"""CPU restatement of the SlotFormer rollouter (torch only) and shared builders for the LDMSlotFormer tests.

Restated from the reference's vp_vqa/models/slotformer.py: the reversed-position sinusoid (lines 8-14), the in / out
projections and the sliding window of SlotRollouter.forward (lines 83-126).  The layers are
oracle.transformer_predictor, which already is nn.TransformerEncoder(norm_first=True, activation=relu)."""
import functools
import gzip
import json
import os

import torch
import torch.nn.functional as F

from slotdiffusion_amd import compat
from tests.detfill import det_fill_, is_buffer_name

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LAYERS, ROLLOUT_LEN = 2, 3              # the fixture's reductions of the shipped config (tools/gen_golden.py slotformer)


def sin_pos_enc(seq_len, d_model):
    """slotformer.py:8-14: [1, L, D], positions L-1 .. 0."""
    inv_freq = 1. / (10000 ** (torch.arange(0.0, d_model, 2.0) / d_model))
    pos_seq = torch.arange(seq_len - 1, -1, -1).type_as(inv_freq)
    sinusoid_inp = torch.outer(pos_seq, inv_freq)
    return torch.cat([sinusoid_inp.sin(), sinusoid_inp.cos()], dim=-1).unsqueeze(0)


def rollouter_forward(W, x, pred_len, num_slots, num_layers, num_heads, name='rollouter'):
    """slotformer.py:83-126.  W: {key: fp32 tensor}; x [B, T, N, Ds] -> [B, pred_len, N, Ds]."""
    from oracle import slotdiff_oracle as O
    B, T = x.shape[:2]
    in_x = x.flatten(1, 2)
    enc_pe = W[f'{name}.enc_t_pe'].unsqueeze(2).repeat(B, 1, num_slots, 1).flatten(1, 2)
    if f'{name}.enc_slots_pe' in W:
        enc_pe = enc_pe + W[f'{name}.enc_slots_pe'].unsqueeze(1).repeat(B, T, 1, 1).flatten(1, 2)
    out = []
    for _ in range(pred_len):
        h = F.linear(in_x, W[f'{name}.in_proj.weight'], W[f'{name}.in_proj.bias']) + enc_pe
        h = O.transformer_predictor(W, h, num_layers, num_heads, name=name)
        out.append(F.linear(h[:, -num_slots:], W[f'{name}.out_proj.weight'], W[f'{name}.out_proj.bias']))
        in_x = torch.cat([in_x[:, num_slots:], out[-1]], dim=1)
    return torch.stack(out, dim=1)


def encoder_layer(W, x, l, num_heads):
    """One layer `l` = '<name>.transformer_encoder.layers.<i>' on x [B, L, D] (oracle.transformer_predictor's body)."""
    from oracle import slotdiff_oracle as O
    name, i = l.split('.transformer_encoder.layers.')
    Wl = {k.replace(f'.layers.{i}.', '.layers.0.'): v for k, v in W.items() if k.startswith(l + '.')}
    return O.transformer_predictor(Wl, x, 1, num_heads, name=name)


def shipped_values():
    return json.load(open(os.path.join(GOLD, 'vp_vqa', 'ldmslotformer_physion_params-res128.json')))


def shipped_params(**over):
    """Params of the shipped config (values dumped by tools/dump_ref_configs.py); over: rollout_dict / loss_dict items."""
    d = shipped_values()
    for k, v in over.items():
        (d['rollout_dict'] if k in d['rollout_dict'] else d['loss_dict'])[k] = v
    return compat.Params(**d)


def key_fixture():
    with gzip.open(os.path.join(GOLD, 'vp_vqa', 'ldmslotformer_keys.json.gz'), 'rt') as f:
        return json.load(f)


def _skip(n):
    return is_buffer_name(n) or n.endswith('enc_t_pe')


def build(history_len=15, num_slots=8, decoder=False, num_layers=LAYERS, rollout_len=ROLLOUT_LEN):
    """LDMSlotFormer of the shipped config with `num_layers` layers, det-filled like the fixture's reference model
    (position in state_dict order seeds each tensor; the decoder's 150 M values only when asked for)."""
    import importlib
    P = shipped_params(num_layers=num_layers, rollout_len=rollout_len, history_len=history_len)
    P.rollout_dict['num_slots'] = P.slot_dict['num_slots'] = num_slots
    P.dec_dict['dec_ckp_path'] = ''
    m = importlib.import_module('slotdiffusion.vp_vqa').build_model(P)
    det_fill_(m.state_dict().items(), skip=(_skip if decoder else (lambda n: _skip(n) or n.startswith('dm_decoder.'))))
    m.pred_dropout = 0.0
    return m


@functools.lru_cache(maxsize=None)
def gpu_model(history_len=15, num_slots=8, decoder=False):
    """One model per geometry for a whole test session (building the 150 M-parameter decoder takes seconds)."""
    return build(history_len, num_slots, decoder).cuda().eval()


def rollouter_weights(m):
    return {k: v.detach().float().cpu() for k, v in m.state_dict().items() if k.startswith('rollouter.')}
