"""Container-only: golden G29 -- the Map-free aggregator and its gradients, produced by the reference's own class:

    mapfree_6dreg/lib/models/regression/aggregator.py: CorrelationVolumeWarping (:6-116), unmodified, in FAR's configuration
    (config/regression/mapfree/rot6d_trans_with_loftr.yaml: POSITION_ENCODER, MAX_SCORE_CHANNEL; tests/mapfree_reg_inputs.py: config)

differentiated by torch autograd on the CPU, twice: in fp32 as the reference ships, and under torch.set_default_dtype(torch.float64)
(inputs cast to float64; the module builds its grid in the default dtype).  B = 2, 32 channels on a 7 x 5 grid; the inputs and the
fixed upstream gradient come from one seeded numpy generator.  The fixture holds data only: the inputs, dagg, and agg / dvol0 / dvol1
in both forms.  The input condition of the training tests (tests/cvw_train_ref.py: MIN_GAP between each row's two largest float64
scores) is asserted here and printed.
Usage: python tools/make_golden_cvw_train.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'g29_cvw_train.npz')
REF = '/root/reference/mapfree_6dreg'
SEED, SHAPE, AMP = 29, (2, 32, 7, 5), 0.5


def main():
    from tests import cvw_train_ref as cr
    from tests import mapfree_reg_inputs as mi
    sys.path.insert(0, REF)
    from lib.models.regression.aggregator import CorrelationVolumeWarping
    rng = np.random.default_rng(SEED)
    vol0 = (AMP * rng.standard_normal(SHAPE)).astype(np.float32)
    vol1 = (AMP * rng.standard_normal(SHAPE)).astype(np.float32)
    dagg = rng.standard_normal((SHAPE[0], 67) + SHAPE[2:]).astype(np.float32)
    dagg[:, 66] *= 4
    gap = cr.min_gap(torch.from_numpy(vol0), torch.from_numpy(vol1))
    print(f'[g29] smallest top-2 score gap {gap:.3e} (condition: >= {cr.MIN_GAP:g})')
    assert gap >= cr.MIN_GAP
    out = {'vol0': vol0, 'vol1': vol1, 'dagg': dagg}
    for tag, dtype in (('32', torch.float32), ('64', torch.float64)):
        torch.set_default_dtype(dtype)
        try:
            m = CorrelationVolumeWarping(mi.config().AGGREGATOR, SHAPE[1])
            assert m.num_out_layers == 67 and not m.state_dict()
            v0 = torch.from_numpy(vol0).to(dtype).requires_grad_(True)
            v1 = torch.from_numpy(vol1).to(dtype).requires_grad_(True)
            agg = m(v0, v1)
            assert agg.dtype == dtype and agg.shape == (SHAPE[0], 67) + SHAPE[2:]
            d0, d1 = torch.autograd.grad(agg, (v0, v1), torch.from_numpy(dagg).to(dtype))
        finally:
            torch.set_default_dtype(torch.float32)
        out[f'agg{tag}'], out[f'dvol0_{tag}'], out[f'dvol1_{tag}'] = agg.detach().numpy(), d0.numpy(), d1.numpy()
    for k in ('agg', 'dvol0_', 'dvol1_'):
        d = np.abs(out[k + '32'] - out[k + '64']).max()
        print(f'[g29] {k.rstrip("_")}: fp32-vs-float64 {d:.3e}  max |float64| {np.abs(out[k + "64"]).max():.3e}')
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
