"""CPU restatement of the SAVi slot transition families (torch only) and shared builders for the predictor tests.

Restated from the reference's video_based/models/predictor.py: ResidualMLPPredictor.forward (lines 65-73) and
RNNPredictorWrapper.forward / reset (lines 102-120, 132-135) around nn.LSTM's cell (gate order i, f, g, o); the choice
between the families is savi.py:320-347.  The transformer base predictor is oracle.transformer_predictor.  Everything
runs in the dtype of its inputs, so the tests compute fp64 references from it; `rnd` is applied to every tensor that
feeds a matrix product (identity by default; the bf16 tests round there, as sdmi_pred_step does)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = 'savi_pred_family.npz'
VARIANTS = {                                        # fixture case -> pred_dict items
    'mlp': dict(pred_type='mlp', pred_rnn=False, pred_norm_first=True),
    'mlp_post': dict(pred_type='mlp', pred_rnn=False, pred_norm_first=False),
    'mlp_rnn': dict(pred_type='mlp', pred_rnn=True, pred_norm_first=True),
    'transformer_rnn': dict(pred_type='transformer', pred_rnn=True, pred_norm_first=True),
}
D, H, LAYERS, HEADS, FFN = 32, 64, 1, 1, 64        # the fixture's geometry (tools/gen_golden_pred.py)


def pred_dict(case, sg_every=None):
    return dict(VARIANTS[case], pred_num_layers=LAYERS, pred_num_heads=HEADS, pred_ffn_dim=FFN, pred_sg_every=sg_every)


def ident(t):
    return t


def bf16(t):
    """Round to bf16 (nearest even), keep the dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def residual_mlp(W, x, name, norm_first=True, rnd=ident):
    """predictor.py:65-73.  x [..., D]."""
    xn = F.layer_norm(x, x.shape[-1:], W[f'{name}.ln.weight'], W[f'{name}.ln.bias'], 1e-5)
    res = xn if norm_first else x
    hid = F.relu(F.linear(rnd(xn), W[f'{name}.mlp.0.weight'], W[f'{name}.mlp.0.bias']))
    return F.linear(rnd(hid), W[f'{name}.mlp.2.weight'], W[f'{name}.mlp.2.bias']) + res


def lstm_cell(z, c_prev):
    """nn.LSTM's cell on pre-activations z [R, 4H] (i, f, g, o) -> (h, c, activated gates)."""
    i, f, g, o = z.chunk(4, -1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat([i, f, g, o], -1)


def lstm_step(W, u, state, name, rnd=ident):
    """predictor.py:113-118 on rows u [R, D]; state (h, c) or None -> (y [R, D], (h, c))."""
    Hh = W[f'{name}.rnn.weight_hh_l0'].shape[1]
    h, c = state if state is not None else (u.new_zeros(u.shape[0], Hh), u.new_zeros(u.shape[0], Hh))
    z = F.linear(rnd(u), W[f'{name}.rnn.weight_ih_l0'], W[f'{name}.rnn.bias_ih_l0']) + \
        F.linear(rnd(h), W[f'{name}.rnn.weight_hh_l0'], W[f'{name}.rnn.bias_hh_l0'])
    h, c, _ = lstm_cell(z, c)
    return F.linear(rnd(h), W[f'{name}.out_projector.weight'], W[f'{name}.out_projector.bias']), (h, c)


class Predictor:
    """The transition as the reference's module tree behaves: callable on slots [B, N, D], with reset()."""

    def __init__(self, W, pd, name='predictor', rnd=ident):
        self.W, self.pd, self.name, self.rnd = W, pd, name, rnd
        self.rnn = bool(pd.get('pred_rnn', False))
        self.base = f'{name}.base_predictor' if self.rnn else name
        self.reset()

    def reset(self):
        self.step, self.hidden = 0, None

    def __call__(self, x):
        sg = self.pd.get('pred_sg_every')
        if self.rnn and sg is not None and self.step % sg == 0 and self.step > 0:
            x = x.detach()
            self.hidden = tuple(h.detach() for h in self.hidden)
        if self.pd.get('pred_type', 'transformer') == 'mlp':
            out = residual_mlp(self.W, x, self.base, self.pd.get('pred_norm_first', True), self.rnd)
        else:
            from oracle import slotdiff_oracle as O
            out = O.transformer_predictor(self.W, x, self.pd['pred_num_layers'], self.pd['pred_num_heads'], name=self.base)
        if not self.rnn:
            return out
        y, self.hidden = lstm_step(self.W, out.reshape(-1, out.shape[-1]), self.hidden, self.name, self.rnd)
        self.step += 1
        return y.view(out.shape)


def clip_slots(W, img, plan, num_iterations, pd, eps=1e-6):
    """The video models' encode (savi.py:366-397) with this transition: img [B, T, 3, H, W] -> slots [B, T, N, D]."""
    from oracle import slotdiff_oracle as O
    B, T = img.shape[:2]
    x = O.encoder_out(W, img.flatten(0, 1), plan).unflatten(0, (B, T))
    init = W['init_latents'].repeat(B, 1, 1)
    pred, prev, out = Predictor(W, pd), None, []
    for t in range(T):
        lat = init if prev is None else pred(prev)
        prev, _ = O.slot_attention(W, x[:, t], lat, num_iterations, eps)
        out.append(prev)
    return torch.stack(out, 1)


def tiny_cfg(model, case, sg_every=None):
    """Smallest video model around the fixture's transition geometry: 32 x 32 frames, 3 slots of D = 32, H = 64.
    model: 'SAVi' | 'SAViDiffusion'.  -> dict with the constructor's keyword arguments (+ 'model', 'input_frames')."""
    from slotdiffusion_amd import configs
    cfg = configs.savi_cfg() if model == 'SAVi' else configs.movie_cfg()
    cfg['resolution'] = (32, 32)
    cfg['slot_dict'] = dict(num_slots=3, slot_size=D, slot_mlp_size=H, num_iterations=2)
    cfg['enc_dict']['enc_out_channels'] = D
    if model == 'SAVi':
        cfg['dec_dict'] = dict(dec_channels=(D, 16, 16, 16, 16), dec_resolution=(8, 8), dec_ks=5, dec_norm='')
    else:
        dd = cfg['dec_dict']
        dd['resolution'] = (8, 8)
        dd['vae_dict']['enc_dec_dict']['resolution'] = 32
        dd['unet_dict']['context_dim'] = D
    cfg['pred_dict'] = pred_dict(case, sg_every)
    cfg.pop('clip_len', None)
    return dict(cfg, model=model, input_frames=4)


def build_tiny(model, case, sg_every=None, **kw):
    """Our model for tiny_cfg, det-filled by position in state_dict order (buffers keep their computed values)."""
    from slotdiffusion_amd import models
    from tests.detfill import det_fill_, is_buffer_name
    cfg = tiny_cfg(model, case, sg_every)
    cls = getattr(models, cfg.pop('model'))
    m = cls(clip_len=cfg.pop('input_frames'), **cfg, **kw)
    det_fill_(m.state_dict().items(), skip=is_buffer_name)
    return m


def load_fixture():
    z = np.load(os.path.join(GOLD, FIXTURE))
    return {k: z[k] for k in z.files}


def fixture_weights(G, case, dtype=torch.float32, prefix='predictor.'):
    """{prefix + key: tensor} of a fixture case, det-filled by position in its key list like the reference module was
    (the fixture's keys are those of the predictor module itself)."""
    from tests.detfill import det_value
    keys = [str(k) for k in G[f'{case}/keys']]
    shapes = [tuple(int(v) for v in s if v >= 0) for s in G[f'{case}/shapes']]
    return {prefix + k: det_value(k, s, i).to(dtype) for i, (k, s) in enumerate(zip(keys, shapes))}
