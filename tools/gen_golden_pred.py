"""Record tests/golden/savi_pred_family.npz from the reference's slot transition modules (build container only; never
imported by a test).

    python tools/gen_golden_pred.py --reference <checkout of the reference>

Loads video_based/models/predictor.py by file path (it needs only torch), builds the three families the video models
can select besides the plain transformer (savi.py:320-347) -- residual MLP (norm_first both ways), residual MLP inside
the LSTM wrapper, transformer inside the LSTM wrapper -- fills them with tests/detfill values by position in
state_dict order and records, per case: the state_dict key list and shapes, four inputs [B=2, N=3, D=32] (H = 64), the
outputs of four consecutive calls, and the output of a call on the second input after reset().  Data only."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import predictor_ref as R                    # noqa: E402
from tests.detfill import det_fill_                     # noqa: E402


def build(P, case):
    pd = R.pred_dict(case)
    if pd['pred_type'] == 'mlp':
        m = P.ResidualMLPPredictor([R.D, 2 * R.D, R.D], norm_first=pd['pred_norm_first'])
    else:
        m = P.TransformerPredictor(R.D, R.LAYERS, R.HEADS, R.FFN, norm_first=pd['pred_norm_first'])
    if pd['pred_rnn']:
        m = P.RNNPredictorWrapper(m, R.D, R.H, num_layers=1, rnn_cell='LSTM', sg_every=None)
    return m.eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='root of the reference checkout')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', R.FIXTURE))
    a = ap.parse_args()
    path = os.path.join(a.reference, 'slotdiffusion', 'video_based', 'models', 'predictor.py')
    sp = importlib.util.spec_from_file_location('ref_predictor', path)
    P = importlib.util.module_from_spec(sp)
    sp.loader.exec_module(P)
    out = {}
    g = torch.Generator().manual_seed(31)
    x = torch.randn(4, 2, 3, R.D, generator=g)
    for case in R.VARIANTS:
        m = build(P, case)
        det_fill_(m.state_dict().items())
        sd = m.state_dict()
        out[f'{case}/keys'] = np.array(list(sd.keys()))
        out[f'{case}/shapes'] = np.array([(list(v.shape) + [-1, -1])[:2] for v in sd.values()], dtype=np.int64)
        out[f'{case}/x'] = x.numpy()
        with torch.no_grad():
            m.reset()
            out[f'{case}/y'] = torch.stack([m(x[t]) for t in range(4)]).numpy()
            m.reset()
            out[f'{case}/y_reset'] = m(x[1]).numpy()
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), 'bytes')


if __name__ == '__main__':
    main()
